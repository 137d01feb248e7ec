"""The decode cross-attention with the encoder keys split across workgroups against the two calls
that existed before it.

  a_plain     t5_decode_cross_attention on K / V repeat_interleave'd to [P*G, nH, S, d] (at G 1: as they are)
  b_grouped   t5_decode_cross_attention_grouped on the shared [P, nH, S, d]
  s2, s4, s8  t5_decode_cross_attention_split on the shared [P, nH, S, d] at 2, 4 and 8 ranges

All routes run in one process on the same values.  Before any timing every split result is held to
the oracle rule of tests/t5_decode_attn_checks.py (float64 oracle, torch's eager route on the device
as the yardstick: bf16 e <= e_torch + one bf16 ulp of max|oracle|); a miss aborts the shape.

Two timings per route, medians of --reps (default 20) with min and max, routes interleaved and their
order shuffled per repetition:
  eager   HIP events around one call (the host's launch cost is inside)
  graph   one captured graph of CALLS back-to-back calls rotating over COPIES copies of q, K and V
          (a layer's keys are not L2-hot when its turn comes), HIP events around one replay / CALLS:
          what a token of a captured rollout pays, the second launch of the split route included

The plan (trlx_t5_decode_attn_split_plan) is set from the graph timing: per shape, the best existing
route is the lower median of a and b; an X qualifies when its median is below that median by more
than that route's own max - min; `decision` is the qualifying X with the lowest median, else 1.
`split_does_not_win` lists every shape where no X qualifies, `library_plan` what the built library
returns for the shape.

Shapes (bf16): T5-base (nH 12, d 64) B 8; P 2 x G 4; P 64 x G 4; P 32 x G 8; B 256; B 256 with a quarter
of the rows live; nH 32, d 128 at B 8 and B 128; each at S 512 and S 2048.

--parent-lib PATH: the A/B of the entries that existed before against another build of the library
(tools/t5_cross_group_bench.py existing_entries_ab, unchanged), recorded under `existing_entries_ab`.

    python tools/t5_cross_split_bench.py [--reps N] [--out FILE] [--shapes a,b] [--parent-lib other/libtrlx_t5_amd.so]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
_lib = P._lib

XS = (2, 4, 8)
CALLS, COPIES = 16, 4
# name, P, G, nH, d, live fraction (None: no live=)
SHAPES = [("t5base_B8", 8, 1, 12, 64, None), ("t5base_P2_G4", 2, 4, 12, 64, None), ("t5base_P64_G4", 64, 4, 12, 64, None),
          ("t5base_P32_G8", 32, 8, 12, 64, None), ("t5base_B256", 256, 1, 12, 64, None),
          ("t5base_B256_live25", 256, 1, 12, 64, 0.25), ("nH32_d128_B8", 8, 1, 32, 128, None),
          ("nH32_d128_B128", 128, 1, 32, 128, None)]
SS = (512, 2048)


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def oracle_check(q, Kx, Vx, outs, chunk=16):
    """The rule of tests/t5_decode_attn_checks.py on the device, `chunk` rows at a time: e_torch, the
    bound and every route's error."""
    import t5_decode_attn_checks as A
    B, nH, _, d = Kx.shape
    e_t, ref_max, e_k = 0.0, 0.0, {k: 0.0 for k in outs}
    for r in range(0, B, chunk):
        q3 = q[r:r + chunk].reshape(-1, nH, d)
        want = A.oracle_cross(q3, Kx[r:r + chunk], Vx[r:r + chunk])
        eager = A.eager_cross(q3, Kx[r:r + chunk], Vx[r:r + chunk])
        e_t = max(e_t, float((eager.double() - want).abs().max()))
        ref_max = max(ref_max, float(want.abs().max()))
        for k, o in outs.items():
            e_k[k] = max(e_k[k], float((o[r:r + chunk].double() - want).abs().max()))
    lim = e_t + A.bf16_ulp(ref_max)
    return {"e_torch": e_t, "bound": lim, "e_kernel": e_k, "within": all(v <= lim for v in e_k.values())}


def bench_shape(Pn, G, nH, d, S, live_frac, dev, reps, rng):
    g = torch.Generator(device=dev).manual_seed(S + Pn + G)
    s, B, inner, e = d ** -0.25, Pn * G, nH * d, 2
    qs = [(torch.randn(B, inner, generator=g, device=dev) * s).to(torch.bfloat16) for _ in range(COPIES)]
    Ks = [(torch.randn(Pn, nH, S, d, generator=g, device=dev) * s).to(torch.bfloat16) for _ in range(COPIES)]
    Vs = [torch.randn(Pn, nH, S, d, generator=g, device=dev).to(torch.bfloat16) for _ in range(COPIES)]
    Kxs = Ks if G == 1 else [k.repeat_interleave(G, 0).contiguous() for k in Ks]
    Vxs = Vs if G == 1 else [v.repeat_interleave(G, 0).contiguous() for v in Vs]
    live = None
    if live_frac is not None:
        live = (torch.rand(B, generator=g, device=dev) < live_frac).long()
    fns = {"a_plain": lambda i: P.t5_decode_cross_attention(qs[i], Kxs[i], Vxs[i], None, live),
           "b_grouped": lambda i: P.t5_decode_cross_attention_grouped(qs[i], Ks[i], Vs[i], None, live)}
    for X in XS:
        fns[f"s{X}"] = lambda i, X=X: P.t5_decode_cross_attention_split(qs[i], Ks[i], Vs[i], None, live, groups=G, splits=X)
    rec = {"P": Pn, "G": G, "B": B, "nH": nH, "d_kv": d, "S": S, "live_rows": None if live is None else int(live.sum()),
           "library_plan": P.t5_decode_cross_attention_split_plan(torch.bfloat16, Pn, G, nH, d, S)}
    tile = 1
    while tile < 4 and tile < G:
        tile *= 2
    geo = {X: P.t5_decode_cross_attention_split_geometry(torch.bfloat16, d, S, X) for X in XS}
    wgs = Pn * nH * -(-G // tile)
    rec["workgroups"] = {"a_plain": B * nH, "b_grouped": wgs, **{f"s{X}": wgs * geo[X]["ranges"] for X in XS}}
    with torch.no_grad():
        outs = {k: fn(0) for k, fn in fns.items()}                   # also the warm-up
        torch.cuda.synchronize()
        assert torch.equal(outs["a_plain"].view(torch.int16), outs["b_grouped"].view(torch.int16))
        if live is not None:                                          # dead rows: zeros on every route; the rule on the live ones
            for k, o in outs.items():
                assert not o[live == 0].any(), k
            on = live != 0
            rec["oracle"] = oracle_check(qs[0][on], Kxs[0][on], Vxs[0][on], {k: o[on] for k, o in outs.items()})
        else:
            rec["oracle"] = oracle_check(qs[0], Kxs[0], Vxs[0], outs)
        assert rec["oracle"]["within"], rec["oracle"]
        # eager
        for _ in range(3):
            for fn in fns.values():
                fn(1)
        evs, order = {k: [] for k in fns}, list(fns)
        for r in range(reps):
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[k](r % COPIES)
                e1.record()
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
        eager = {k: [a.elapsed_time(b) * 1000.0 for a, b in v] for k, v in evs.items()}
        # graphs
        graphs = {}
        for k, fn in fns.items():
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                             # one stream, a linear chain of launches
                keep = [fn(i % COPIES) for i in range(CALLS)]
            graphs[k] = (graph, keep)
        for graph, _ in graphs.values():
            graph.replay()
        torch.cuda.synchronize()
        samples = {k: [] for k in fns}
        for _ in range(reps):
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[k][0].replay()
                e1.record()
                e1.synchronize()
                samples[k].append(e0.elapsed_time(e1) * 1000.0 / CALLS)
        # a replayed split graph computes what the eager call computes
        for X in XS:
            assert torch.equal(graphs[f"s{X}"][1][0].view(torch.int16), outs[f"s{X}"].view(torch.int16)), X
    kv = 2 * Pn * S * inner * e
    if live is not None:
        kv = 2 * int(live.sum()) * S * inner * e
    for k in fns:
        model = (kv * G if k == "a_plain" else kv) + 2 * B * inner * e
        med = statistics.median(samples[k])
        rec[k] = {"graph": {**stats(samples[k]), "bytes_model": model, "TB_per_s_over_model": round(model / (med * 1e-6) / 1e12, 3)},
                  "eager": stats(eager[k])}
    best = min(("a_plain", "b_grouped"), key=lambda k: rec[k]["graph"]["median_us"])
    bg = rec[best]["graph"]
    spread = round(bg["max_us"] - bg["min_us"], 2)
    ok = [X for X in XS if rec[f"s{X}"]["graph"]["median_us"] < bg["median_us"] - spread]
    rec["best_existing"] = {"route": best, "median_us": bg["median_us"], "spread_us": spread}
    rec["qualifying_splits"] = ok
    rec["decision"] = min(ok, key=lambda X: rec[f"s{X}"]["graph"]["median_us"]) if ok else 1
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shapes", default=",".join(n for n, *_ in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_cross_split_bench.json"))
    args = ap.parse_args()
    rec = {"tool": "tools/t5_cross_split_bench.py", "reps": args.reps, "dtype": "bf16",
           "timing": f"graph: one captured graph of {CALLS} back-to-back calls per route rotating over {COPIES} copies of q, K "
                     f"and V, HIP events around one replay / {CALLS}; eager: HIP events around one call; routes interleaved, "
                     f"order shuffled per repetition; medians with min-max, microseconds per call",
           "criterion": "an X qualifies when its graph median is below the best existing route's graph median by more than "
                        "that route's own max - min",
           "shapes": {}}
    if args.parent_lib:   # first: no GPU context in this process while the children run
        import t5_cross_group_bench as GB
        rec["existing_entries_ab"] = GB.existing_entries_ab(args.parent_lib)
        print(json.dumps(rec["existing_entries_ab"]), flush=True)
    dev = torch.device("cuda:0")
    rec["device"] = torch.cuda.get_device_name(0)
    rng = random.Random(8)
    want = set(args.shapes.split(","))
    for name, Pn, G, nH, d, live_frac in SHAPES:
        if name not in want:
            continue
        for S in SS:
            key = f"{name}_S{S}"
            rec["shapes"][key] = bench_shape(Pn, G, nH, d, S, live_frac, dev, args.reps, rng)
            print(key, json.dumps(rec["shapes"][key]), flush=True)
            torch.cuda.empty_cache()
    rec["plan_from_table"] = {k: sh["decision"] for k, sh in rec["shapes"].items()}
    rec["split_does_not_win"] = [
        f"{k}: best split s{min(XS, key=lambda X: sh[f's{X}']['graph']['median_us'])} "
        f"{min(sh[f's{X}']['graph']['median_us'] for X in XS)} us vs {sh['best_existing']['route']} "
        f"{sh['best_existing']['median_us']} us (spread {sh['best_existing']['spread_us']} us)"
        for k, sh in rec["shapes"].items() if sh["decision"] == 1]
    print("plan_from_table", json.dumps(rec["plan_from_table"]), flush=True)
    print("split_does_not_win", json.dumps(rec["split_does_not_win"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
