"""The grouped decode cross-attention on MFMA at d_kv 256 (t5_decode_cross_attention_grouped_mma_d256)
against the routes that exist, built like tools/t5_cross_group_mma_bench.py.

  eager        torch's op order (matmul, mask, softmax, matmul) on K / V repeat_interleave'd to [P*G, nH, S, d]
  sdpa         torch.nn.functional.scaled_dot_product_attention (scale 1) on the same expanded operands
  a_expanded   t5_decode_cross_attention on the expanded K / V: the route the grouped calls took at
               d_kv 256 before this kernel, and the yardstick
  d256_x1 .. d256_x8   the new call on the shared [P, nH, S, d] at splits 1, 2, 4 and 8

All routes run interleaved in one process on the same values, their order shuffled per repetition,
each call between two HIP events after warm-up; medians of --reps (default 20) with min and max.
Before anything is timed every kernel route's result is held to the rule of the GPU test: max|route
- float64| <= 2 * e_torch + one bf16 ulp of max|float64|.  Byte models (live = the unmasked keys per
prompt, summed; e = 2): expanded routes 2 * G * live * nH * d * e, the new call 2 * ceil(G / 16) *
live * nH * d * e, each + q + out (+ the fp32 states written and read at splits > 1).  A difference
between two routes counts only when the medians differ by more than the slower route's own max -
min.  `plan_evidence` lists, per shape, every split that beats splits 1 by more than the spread of
the splits 1 samples: trlx_t5_decode_attn_group_d256_plan is set from it.  kv_bytes_per_layer is the
K / V memory of one decoder layer, shared and expanded (the grouped call divides it by G).

    python tools/t5_cross_group_d256_bench.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
BF = torch.bfloat16
NH, D = 16, 256
XS = (1, 2, 4, 8)
# name, P, G, S, padded variants
SHAPES = [(f"ul2_P{p}_G{g}_S512", p, g, 512, (False, True)) for p, g in ((128, 1), (32, 4), (16, 8), (8, 16), (2, 64))] + \
         [("ul2_P8_G16_S2048", 8, 16, 2048, (False,))] + \
         [(f"ul2_P{p}_G{g}_S512", p, g, 512, (False, True)) for p, g in ((8, 1), (1, 8))]
KERNEL_ROUTES = ("a_expanded",) + tuple(f"d256_x{x}" for x in XS)


def bf16_ulp(x):
    return 0.0 if x <= 0 else 2.0 ** (torch.tensor(x).log2().floor().item() - 7)


def oracle(q, K, V, mask, G):
    """float64 softmax(q·K^T)·V per prompt on the device, masked keys excluded; [P*G, nH*d]."""
    Pn, nH, Sn, d = K.shape
    s = torch.einsum("pgnd,pnsd->pgns", q.view(Pn, G, nH, d).double(), K.double())
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    return torch.einsum("pgns,pnsd->pgnd", torch.softmax(s, -1), V.double()).reshape(Pn * G, nH * d)


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def verdict(x, y):
    """x against y by the spread rule: 'faster', 'slower' or 'no difference'."""
    slow = x if x["median_us"] >= y["median_us"] else y
    if abs(x["median_us"] - y["median_us"]) <= slow["max_us"] - slow["min_us"]:
        return "no difference"
    return "faster" if x["median_us"] < y["median_us"] else "slower"


def bench_shape(Pn, G, S, padded, dev, reps, warmup, rng):
    g = torch.Generator(device=dev).manual_seed(S + Pn + G)
    s, B, inner, e = D ** -0.25, Pn * G, NH * D, 2
    q = (torch.randn(B, inner, generator=g, device=dev) * s).to(BF)
    K = (torch.randn(Pn, NH, S, D, generator=g, device=dev) * s).to(BF)
    V = torch.randn(Pn, NH, S, D, generator=g, device=dev).to(BF)
    Kx, Vx = K.repeat_interleave(G, 0).contiguous(), V.repeat_interleave(G, 0).contiguous()
    mask, maskx, addx, live = None, None, None, Pn * S
    if padded:
        lengths = torch.randint(S // 4, S + 1, (Pn,), generator=g, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] < lengths[:, None]).long()
        maskx = mask.repeat_interleave(G, 0).contiguous()
        addx = torch.zeros(B, 1, 1, S, dtype=BF, device=dev).masked_fill(maskx[:, None, None, :] == 0, float("-inf"))
        live = int(mask.sum())
    q4 = q.view(B, NH, 1, D)
    keep = {}
    fns = {"eager": lambda: P.t5_decode._torch_cross_attention(q, Kx, Vx, maskx),
           "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q4, Kx, Vx, attn_mask=addx, scale=1.0),
           "a_expanded": lambda: keep.__setitem__("a_expanded", P.t5_decode_cross_attention(q, Kx, Vx, maskx))}
    for x in XS:
        fns[f"d256_x{x}"] = lambda x=x: keep.__setitem__(
            f"d256_x{x}", P.t5_decode_cross_attention_grouped_mma_d256(q, K, V, mask, splits=x))
    with torch.no_grad():
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        want = oracle(q, K, V, mask, G)
        e_t = float((P.t5_decode._torch_cross_attention(q, Kx, Vx, maskx).double() - want).abs().max())
        lim = 2.0 * e_t + bf16_ulp(float(want.abs().max()))
        errs = {r: float((keep[r].double() - want).abs().max()) for r in KERNEL_ROUTES}
        for r in KERNEL_ROUTES:
            assert errs[r] <= lim, f"{r}: error {errs[r]} above the bound {lim}"
        evs = {k: [] for k in fns}
        order = list(fns)
        for _ in range(reps):
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[k]()
                e1.record()
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1000.0 for a, b in v] for k, v in evs.items()}
    small, tiles = 2 * B * inner * e, -(-G // 16)
    expanded = 2 * G * live * inner * e + small + (B * S * 8 if padded else 0)
    model = {"eager": expanded, "sdpa": expanded, "a_expanded": expanded}
    groups = {"eager": None, "sdpa": None, "a_expanded": B * NH}
    for x in XS:
        geo = P.t5_decode_cross_attention_grouped_mma_d256_geometry(S, x)
        states = 0 if x == 1 else 2 * P.t5_decode_cross_attention_grouped_mma_d256_workspace_bytes(B, NH, S, x)
        model[f"d256_x{x}"] = 2 * tiles * live * inner * e + small + states + (Pn * tiles * S * 8 if padded else 0)
        groups[f"d256_x{x}"] = Pn * NH * tiles * geo["ranges"]
    rec = {"P": Pn, "G": G, "B": B, "nH": NH, "d_kv": D, "S": S, "padded": padded, "live_keys_per_prompt_summed": live,
           "kv_bytes_per_layer": {"shared": 2 * Pn * S * inner * e, "expanded": 2 * B * S * inner * e},
           "e_torch": e_t, "bound": lim, "e_route": errs}
    for k in fns:
        med = statistics.median(us[k])
        rec[k] = {**stats(us[k]), "bytes_model": model[k], "TB_per_s_over_model": round(model[k] / (med * 1e-6) / 1e12, 3),
                  "workgroups": groups[k]}
    x1 = rec["d256_x1"]
    rec["fastest"] = min(fns, key=lambda r: rec[r]["median_us"])
    rec["splits_faster_than_x1_by_more_than_its_spread"] = [
        x for x in XS[1:] if x1["median_us"] - rec[f"d256_x{x}"]["median_us"] > x1["max_us"] - x1["min_us"]]
    best = min((f"d256_x{x}" for x in XS), key=lambda r: rec[r]["median_us"])
    rec["verdicts"] = {"best_d256": best, "best_d256_vs_a_expanded": verdict(rec[best], rec["a_expanded"]),
                       "best_d256_vs_eager": verdict(rec[best], rec["eager"]),
                       "best_d256_vs_sdpa": verdict(rec[best], rec["sdpa"]),
                       "plan": P.t5_decode_cross_attention_grouped_mma_d256_plan(Pn, G, NH, S)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/t5_cross_group_d256_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around single calls, all routes interleaved, order shuffled per repetition",
           "shapes": {}}
    rng = random.Random(8)
    for name, Pn, G, S, pads in SHAPES:
        for padded in pads:
            key = name + ("_padded" if padded else "")
            rec["shapes"][key] = bench_shape(Pn, G, S, padded, dev, args.reps, args.warmup, rng)
            print(key, json.dumps(rec["shapes"][key]), flush=True)
    rec["plan_evidence"] = {k: sh["splits_faster_than_x1_by_more_than_its_spread"] for k, sh in rec["shapes"].items()}
    rec["d256_does_not_win"] = [f"{k}: {sh['verdicts']['best_d256']} {sh[sh['verdicts']['best_d256']]['median_us']} us, "
                                f"{sh['fastest']} {sh[sh['fastest']]['median_us']} us"
                                for k, sh in rec["shapes"].items() if not sh["fastest"].startswith("d256")]
    print("plan_evidence", json.dumps(rec["plan_evidence"]), flush=True)
    print("d256_does_not_win", json.dumps(rec["d256_does_not_win"]), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "t5_cross_group_d256_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
