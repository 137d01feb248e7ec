"""The decode cross-attention of a rollout that draws G samples per prompt: the existing kernel on the
expanded keys / values against the grouped kernel on the one shared copy.

  a_expanded        t5_decode_cross_attention on K / V repeat_interleave'd to [P*G, nH, S, d], contiguous
  b_grouped         t5_decode_cross_attention_grouped on the shared contiguous [P, nH, S, d]
  c_grouped_inplace t5_decode_cross_attention_grouped on the projection output [P, S, nH*d], in place

b and c run once per built query tile (trlx_t5_decode_attn_group_tile 4 and 8; a G below the tile
takes the smallest built tile that holds it, so at G <= 4 the two are the same kernel and differ by
noise only).  Route a does not depend on the tile; it is timed beside each, in the same run.

All routes run interleaved in one process on the same values, their order shuffled per repetition,
each call between two HIP events after warm-up; medians of --reps (default 20) with min and max.
Byte models (live = the unmasked keys per prompt, summed): a 2 * G * live * nH * d * e, b and c
2 * live * nH * d * e, each + q + out (+ the mask, per row for a, per prompt for b and c).  Device
memory held by K / V: a 2 * P * G * S * nH * d * e, b and c 2 * P * S * nH * d * e.  No speed-up is
assumed: every shape where a grouped route does not beat a is listed under `grouped_does_not_win`.

Shapes: T5-base (nH 12, d 64) with P * G = 256 at G 1, 2, 4, 8, S 512, full and padded; P 2 x G 4
(the 8-row case); nH 32, d 128, P * G = 128 at G 4.  The entry's default tile is the built tile with
the lower b median at T5-base P 64 x G 4, S 512, full: `tile_decision` holds both numbers.

--parent-lib PATH: the A/B of the entries that existed before (trlx_t5_decode_attn, cross at B 256
S 512 with the key mask and self at B 256 t 47, T5-base) against another build of the library, in
alternating child processes, four runs each: this tree's median must lie inside the other build's
own min-max spread, else it is reported as a regression with both spreads.

    python tools/t5_cross_group_bench.py [--reps N] [--out FILE] [--parent-lib other/libtrlx_t5_amd.so]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
_lib = P._lib

S = 512
TILES = (4, 8)
# name, P, G, nH, d
SHAPES = [(f"t5base_P{256 // g}_G{g}", 256 // g, g, 12, 64) for g in (1, 2, 4, 8)] + \
         [("t5base_P2_G4", 2, 4, 12, 64), ("nH32_d128_P32_G4", 32, 4, 32, 128)]
DECISION_SHAPE = "t5base_P64_G4_S512"


def kernel_tile(cap, G):
    """The tile the entry takes: the smallest built tile that holds G, at most `cap`."""
    t = 1
    while t < cap and t < G:
        t *= 2
    return t


def tile_decision(shapes):
    """Both caps' b medians at the decision shape, and at G 8, the only G here at which the two caps
    launch different kernels (at G <= 4 either cap takes the smallest built tile that holds G)."""
    out = {"shape": DECISION_SHAPE, "route": "b_grouped"}
    for key in (DECISION_SHAPE, "t5base_P32_G8_S512"):
        sh = shapes[key]
        kernels = {t: kernel_tile(t, sh["G"]) for t in TILES}
        out[key] = {**{f"cap{t}_median_us": sh[f"b_grouped_tile{t}"]["median_us"] for t in TILES},
                    **{f"cap{t}_spread_us": [sh[f"b_grouped_tile{t}"]["min_us"], sh[f"b_grouped_tile{t}"]["max_us"]] for t in TILES},
                    "kernel_tile_launched": {f"cap{t}": kernels[t] for t in TILES},
                    "same_kernel_under_both_caps": len(set(kernels.values())) == 1,
                    "lower_median": min(TILES, key=lambda t: sh[f"b_grouped_tile{t}"]["median_us"])}
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def bench_shape(Pn, G, nH, d, padded, dev, reps, warmup, rng):
    g = torch.Generator(device=dev).manual_seed(S + Pn + G)
    s, B, inner, e = d ** -0.25, Pn * G, nH * d, 2
    q = (torch.randn(B, 1, inner, generator=g, device=dev) * s).to(torch.bfloat16)
    k3 = (torch.randn(Pn, S, inner, generator=g, device=dev) * s).to(torch.bfloat16)    # the projection output
    v3 = torch.randn(Pn, S, inner, generator=g, device=dev).to(torch.bfloat16)
    K = k3.view(Pn, S, nH, d).transpose(1, 2).contiguous()
    V = v3.view(Pn, S, nH, d).transpose(1, 2).contiguous()
    Kx, Vx = K.repeat_interleave(G, 0).contiguous(), V.repeat_interleave(G, 0).contiguous()
    mask, maskx, live = None, None, Pn * S
    if padded:
        lengths = torch.randint(S // 4, S + 1, (Pn,), generator=g, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] < lengths[:, None]).long()
        maskx = mask.repeat_interleave(G, 0).contiguous()
        live = int(mask.sum())
    keep = {}
    tile = P.t5_decode.t5_decode_cross_attention_group_tile

    def grouped(name, k, v, **kw):
        return lambda: keep.__setitem__(name, P.t5_decode_cross_attention_grouped(q, k, v, mask, **kw))

    fns, tile_of = {}, {}
    for t in TILES:
        fns[f"a_expanded_beside_tile{t}"] = lambda: keep.__setitem__("a", P.t5_decode_cross_attention(q, Kx, Vx, maskx))
        fns[f"b_grouped_tile{t}"] = grouped(f"b{t}", K, V)
        fns[f"c_grouped_inplace_tile{t}"] = grouped(f"c{t}", k3, v3, n_heads=nH)
        tile_of.update({k: t for k in fns if k.endswith(f"tile{t}")})
    try:
        with torch.no_grad():
            for _ in range(warmup):
                for k, fn in fns.items():
                    tile(tile_of[k])
                    fn()
            torch.cuda.synchronize()
            bit_equal = all(torch.equal(keep["a"].view(torch.int16), keep[f"{r}{t}"].view(torch.int16))
                            for r in "bc" for t in TILES)
            assert bit_equal, "a grouped route differs from the existing kernel on the expanded tensors"
            evs = {k: [] for k in fns}
            order = list(fns)
            for _ in range(reps):
                rng.shuffle(order)
                for k in order:
                    tile(tile_of[k])                               # outside the timed pair
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[k]()
                    e1.record()
                    evs[k].append((e0, e1))
            torch.cuda.synchronize()
    finally:
        tile(0)
    us = {k: [a.elapsed_time(b) * 1000.0 for a, b in v] for k, v in evs.items()}
    small = 2 * B * inner * e
    model_a = 2 * G * live * inner * e + small + (B * S * 8 if padded else 0)
    model_g = 2 * live * inner * e + small + (Pn * S * 8 if padded else 0)
    held_a, held_g = 2 * B * S * inner * e, 2 * Pn * S * inner * e
    rec = {"P": Pn, "G": G, "B": B, "nH": nH, "d_kv": d, "S": S, "padded": padded, "live_keys_per_prompt_summed": live,
           "bit_equal_to_a": bit_equal, "kv_bytes_held": {"a_expanded": held_a, "b_and_c_grouped": held_g}}
    for k in fns:
        model = model_a if k.startswith("a_") else model_g
        med = statistics.median(us[k])
        rec[k] = {**stats(us[k]), "bytes_model": model, "TB_per_s_over_model": round(model / (med * 1e-6) / 1e12, 3),
                  "workgroups": B * nH if k.startswith("a_") else Pn * nH * -(-G // kernel_tile(tile_of[k], G))}
    a_med = statistics.median(us["a_expanded_beside_tile4"] + us["a_expanded_beside_tile8"])
    rec["a_expanded_median_us_both_series"] = round(a_med, 2)
    for t in TILES:
        for r in ("b_grouped", "c_grouped_inplace"):
            rec[f"a_over_{r}_tile{t}"] = round(a_med / rec[f"{r}_tile{t}"]["median_us"], 3)
    return rec


# ------------------------------------------------------------------ the entries that existed before
def ab_child():
    """Per-call us of trlx_t5_decode_attn (cross B 256 S 512 masked, self B 256 t 47) on whatever library
    TRLX_T5_AMD_LIB names."""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:   # an older build lacks the newer entries
        del _lib.SIGNATURES[n]
    dev = torch.device("cuda:0")
    B, nH, d, T, t = 256, 12, 64, 48, 47
    inner = nH * d
    g = torch.Generator(device=dev).manual_seed(3)
    cache = P.T5DecodeKVCache(B, nH, d, T, torch.bfloat16, dev)
    cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev) * d ** -0.25)
    cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
    qkv = (torch.randn(B, 3 * inner, generator=g, device=dev) * d ** -0.25).to(torch.bfloat16)
    q, kn, vn = (qkv[:, j * inner:(j + 1) * inner] for j in range(3))
    table = P.t5_relative_bias_table(torch.randn(32, nH, generator=g, device=dev), T)
    k_enc = (torch.randn(B, nH, S, d, generator=g, device=dev) * d ** -0.25).to(torch.bfloat16)
    v_enc = torch.randn(B, nH, S, d, generator=g, device=dev).to(torch.bfloat16)
    mask = torch.ones(B, S, dtype=torch.int64, device=dev)
    mask[:, S - 37:] = 0
    res = {}
    for name, fn in (("t5_decode_attn_cross_B256_S512", lambda: P.t5_decode_cross_attention(q, k_enc, v_enc, mask)),
                     ("t5_decode_attn_self_B256_t47", lambda: P.t5_decode_self_attention(q, kn, vn, cache, t, table))):
        for _ in range(20):
            fn()
        per = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1000.0 / 20)
        res[name] = statistics.median(per)
    print("AB_CHILD " + json.dumps(res))


def existing_entries_ab(parent_lib, runs=4):
    sides = {"parent": os.path.abspath(parent_lib), "this_tree": _lib.LIB_PATH}
    got = {s: {} for s in sides}
    for _ in range(runs):
        for side, lib in sides.items():   # alternating child processes
            env = dict(os.environ, TRLX_T5_AMD_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child"], env=env, capture_output=True,
                               text=True, timeout=300, check=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_CHILD ")][-1]
            for k, v in json.loads(line[len("AB_CHILD "):]).items():
                got[side].setdefault(k, []).append(v)
    out = {"unit": "us per call (HIP events around 20 calls, median of 30), one figure per child process",
           "criterion": "this tree's median inside the parent's own min-max spread"}
    for k in got["parent"]:
        p, c = got["parent"][k], got["this_tree"][k]
        med = statistics.median(c)
        out[k] = {"parent": p, "this_tree": c, "parent_spread": [min(p), max(p)], "this_tree_spread": [min(c), max(c)],
                  "this_tree_median": med, "inside_parent_spread": min(p) <= med <= max(p),
                  "verdict": "inside" if min(p) <= med <= max(p) else ("faster" if med < min(p) else "REGRESSION")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_cross_group_bench.json"))
    args = ap.parse_args()
    if args.ab_child:
        return ab_child()
    rec = {"tool": "tools/t5_cross_group_bench.py", "reps": args.reps,
           "timing": "HIP events around single calls, all routes interleaved, order shuffled per repetition",
           "shapes": {}}
    if args.parent_lib:   # first: no GPU context in this process while the children run
        rec["existing_entries_ab"] = existing_entries_ab(args.parent_lib)
        print(json.dumps(rec["existing_entries_ab"]), flush=True)
    dev = torch.device("cuda:0")
    rec["device"] = torch.cuda.get_device_name(0)
    rng = random.Random(8)
    for name, Pn, G, nH, d in SHAPES:
        for padded in (False, True):
            key = f"{name}_S{S}" + ("_padded" if padded else "")
            rec["shapes"][key] = bench_shape(Pn, G, nH, d, padded, dev, args.reps, args.warmup, rng)
            print(key, json.dumps(rec["shapes"][key]), flush=True)
    rec["tile_decision"] = tile_decision(rec["shapes"])
    rec["grouped_does_not_win"] = [f"{key}: {r}_tile{t} {sh[f'{r}_tile{t}']['median_us']} us vs a "
                                   f"{sh['a_expanded_median_us_both_series']} us"
                                   for key, sh in rec["shapes"].items() for t in TILES
                                   for r in ("b_grouped", "c_grouped_inplace") if sh[f"a_over_{r}_tile{t}"] <= 1.0]
    print("tile_decision", json.dumps(rec["tile_decision"]), flush=True)
    print("grouped_does_not_win", json.dumps(rec["grouped_does_not_win"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
