"""t5_decode_linear against the launches it replaces, per fused call, inside replayed graphs.

Three routes per call: `fused` (trlx_t5_decode_linear: every row in each workgroup), `rows`
(split_rows=True, trlx_t5_decode_linear_rows: the rows spread over workgroups) and `unfused`
(hipBLASLt and its neighbours).  At M 256 the rows route also runs with live=: a fixed scattered
pattern of live fractions 1.0 / 0.52 / 0.25 (`rows_live_1.0` ...), the finished rows skipped on the device.

Calls (K -> N), each at M 8, 32, 64, 128 and 256, for T5-base (D 768, inner 768, F 2048 gated) and a d_model
4096 shape (inner 4096, F 10240 gated, T5-XXL's):

  norm_qkv        [norm -> qkv]         against t5_rmsnorm + torch.matmul
  o_residual      [o + residual -> h]   against torch.matmul + the bf16 add (h.add_)
  norm_cq         [norm -> cq]          against t5_rmsnorm + torch.matmul
  norm_wi_act     [norm -> wi -> act]   against t5_rmsnorm + torch.matmul + t5_ff_act_packed
  wo_residual     [wo + residual -> h]  against torch.matmul + the add
  layer_chain     the six projections of a layer back to back with their neighbours (the attentions
                  left out: their outputs are stand-in buffers): 6 launches against the 10 of the
                  12-launch layer (6 torch.matmul, 3 t5_add_rmsnorm, t5_ff_act_packed)
  lm_head         N 32128 without neighbours (T5-base only): a real GEMM, not this kernel's target

Eager decode calls measure the host, so each route is ONE captured graph (torch.cuda.graph) of 64
back-to-back calls that rotate over 8 copies of the weights and of the buffers (a layer's weights are
not L2-hot when its turn comes: 12 layers of them cycle between two visits).  Routes are interleaved,
their order shuffled per repetition; a sample is one replay between two HIP events divided by 64; the
figure is the median of --reps with min-max, in microseconds per call, and the weight bytes of the
call over the median.  No speed-up is assumed: every row says which route is faster.

--parity: instead, the accuracy sweep of tests/t5_decode_linear_checks.py (the shapes, the float64
oracle, the unfused route) and the worst ratio e_kernel / (2 e_unfused + one bf16 ulp) per
combination, written to profiles/t5_decode_linear_parity.json.

    python tools/t5_decode_linear_bench.py [--parity] [--reps 20]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

P = entry.load_package()
DT = torch.bfloat16
CALLS, COPIES = 64, 8
SHAPES = {"t5_base": dict(D=768, inner=768, F=2048), "d_model_4096": dict(D=4096, inner=4096, F=10240)}
ACT = "gelu_new"


LIVE_FRACTIONS = (1.0, 0.52, 0.25)
LIVE_AT_M = 256


def live_pattern(M, frac, dev):
    """round(M * frac) live rows at fixed, scattered places (tools/t5_rollout_bench.py's pattern)."""
    n = max(1, round(M * frac))
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(17))
    live = torch.zeros(M, dtype=torch.int64)
    live[perm[:n]] = 1
    return live.to(dev)


def sides_of(M):
    """route name -> the keywords t5_decode_linear takes on it (None: the unfused route)."""
    sides = {"fused": {}, "rows": dict(split_rows=True), "unfused": None}
    if M == LIVE_AT_M:
        for f in LIVE_FRACTIONS:
            sides[f"rows_live_{f}"] = dict(split_rows=True, live=f)
    return sides


def build_routes(shape, M, dev, with_lm_head, kw):
    """{call: {"fused": fn(i), "unfused": fn(i), "weight_bytes": n, "launches": (fused, unfused)}}; fn(i)
    issues call number i on copy i % COPIES.  kw: what every t5_decode_linear call of "fused" takes on top
    (split_rows, live)."""
    D, inner, F = shape["D"], shape["inner"], shape["F"]
    g = torch.Generator(device=dev).manual_seed(M + D)

    def w(n, k):
        return [(torch.randn(n, k, generator=g, device=dev) * k ** -0.5).to(DT) for _ in range(COPIES)]

    def buf(n):
        return [torch.randn(M, n, generator=g, device=dev).to(DT) for _ in range(COPIES)]

    W = dict(qkv=w(3 * inner, D), o=w(D, inner), cq=w(inner, D), co=w(D, inner), wi=w(2 * F, D), wo=w(D, F))
    ln = [(1.0 + 0.1 * torch.randn(D, generator=g, device=dev)).to(DT) for _ in range(COPIES)]
    h, a, f = buf(D), buf(inner), buf(F)
    o_qkv, o_cq, o_ff, o_d = buf(3 * inner), buf(inner), buf(F), buf(D)
    def lin(*a, **k):
        return P.t5_decode_linear(*a, **k, **kw)

    nbytes = {k: v[0].numel() * 2 for k, v in W.items()}
    R = {}

    def norm_proj(name, key, out):
        R[name] = dict(
            fused=lambda i: lin(h[i % COPIES], W[key][i % COPIES], norm_weight=ln[i % COPIES], out=out[i % COPIES]),
            unfused=lambda i: torch.matmul(P.t5_rmsnorm(h[i % COPIES], ln[i % COPIES]), W[key][i % COPIES].t(),
                                           out=out[i % COPIES]),
            weight_bytes=nbytes[key], launches=(1, 2))

    def proj_res(name, key, src):
        # the in-place stream update: out = h.  The unfused route adds into h as well (matmul, add_).
        R[name] = dict(fused=lambda i: lin(src[i % COPIES], W[key][i % COPIES], residual=h[i % COPIES], out=h[i % COPIES]),
                       unfused=lambda i: h[i % COPIES].add_(torch.matmul(src[i % COPIES], W[key][i % COPIES].t())),
                       weight_bytes=nbytes[key], launches=(1, 2))

    norm_proj("norm_qkv", "qkv", o_qkv)
    proj_res("o_residual", "o", a)
    norm_proj("norm_cq", "cq", o_cq)
    R["norm_wi_act"] = dict(
        fused=lambda i: lin(h[i % COPIES], W["wi"][i % COPIES], norm_weight=ln[i % COPIES], act=ACT, gated=True,
                            out=o_ff[i % COPIES]),
        unfused=lambda i: P.t5_ff_act_packed(torch.matmul(P.t5_rmsnorm(h[i % COPIES], ln[i % COPIES]), W["wi"][i % COPIES].t()), ACT),
        weight_bytes=nbytes["wi"], launches=(1, 3))
    proj_res("wo_residual", "wo", f)

    def chain_fused(i):
        c = i % COPIES
        lin(h[c], W["qkv"][c], norm_weight=ln[c], out=o_qkv[c])
        lin(a[c], W["o"][c], residual=h[c], out=h[c])
        lin(h[c], W["cq"][c], norm_weight=ln[c], out=o_cq[c])
        lin(a[c], W["co"][c], residual=h[c], out=h[c])
        lin(h[c], W["wi"][c], norm_weight=ln[c], act=ACT, gated=True, out=o_ff[c])
        lin(o_ff[c], W["wo"][c], residual=h[c], out=h[c])

    def chain_unfused(i):
        c = i % COPIES
        y = P.t5_rmsnorm(h[c], ln[c]) if i == 0 else chain_unfused.y
        torch.matmul(y, W["qkv"][c].t(), out=o_qkv[c])
        hh, y = P.t5_add_rmsnorm(torch.matmul(a[c], W["o"][c].t()), h[c], ln[c])
        torch.matmul(y, W["cq"][c].t(), out=o_cq[c])
        hh, y = P.t5_add_rmsnorm(torch.matmul(a[c], W["co"][c].t()), hh, ln[c])
        ff = P.t5_ff_act_packed(torch.matmul(y, W["wi"][c].t()), ACT)
        hh, chain_unfused.y = P.t5_add_rmsnorm(torch.matmul(ff, W["wo"][c].t()), hh, ln[(c + 1) % COPIES])

    R["layer_chain"] = dict(fused=chain_fused, unfused=chain_unfused, weight_bytes=sum(nbytes.values()), launches=(6, 10))
    if with_lm_head:
        Vn = 32128
        lm = w(Vn, D)[:2]
        o_lm = [torch.empty(M, Vn, dtype=DT, device=dev) for _ in range(2)]
        R["lm_head"] = dict(fused=lambda i: lin(h[i % COPIES], lm[i % 2], out=o_lm[i % 2]),
                            unfused=lambda i: torch.matmul(h[i % COPIES], lm[i % 2].t(), out=o_lm[i % 2]),
                            weight_bytes=Vn * D * 2, launches=(1, 1))
    return R


def capture(fn):
    for i in range(2):
        fn(i)                                                     # warm-up: lazy initialisation, hipBLASLt's choice
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # one stream, a linear chain of launches
        for i in range(CALLS):
            fn(i)
    return graph


def run_shape(name, M, dev, reps):
    sides = sides_of(M)
    graphs, alive = {}, []
    with torch.no_grad():
        # every side on tensors of its own, built from the same seed: the same values
        for side, kw in sides.items():
            if kw is not None and "live" in kw:
                kw = dict(kw, live=live_pattern(M, kw["live"], dev))
            routes = build_routes(SHAPES[name], M, dev, with_lm_head=name == "t5_base" and side in ("fused", "rows", "unfused"),
                                  kw=kw or {})
            alive.append(routes)       # a graph holds addresses, not tensors: every side's tensors live until the last replay
            if side == "fused":
                calls = routes                                    # the calls, their bytes and launch counts
            for call, r in routes.items():
                graphs[(call, side)] = capture(r["unfused" if kw is None else "fused"])
        keys = list(graphs)
        samples = {k: [] for k in keys}
        rng = random.Random(M)
        for k in keys:
            graphs[k].replay()
        torch.cuda.synchronize()
        for _ in range(reps):
            rng.shuffle(keys)
            for k in keys:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[k].replay()
                e1.record()
                e1.synchronize()
                samples[k].append(e0.elapsed_time(e1) * 1000.0 / CALLS)
    out = {}
    for call, r in calls.items():
        row = {"weight_bytes": r["weight_bytes"], "launches_fused": r["launches"][0], "launches_unfused": r["launches"][1]}
        for side in sides:
            if (call, side) not in samples:
                continue
            s = samples[(call, side)]
            med = statistics.median(s)
            row[side] = {"us_per_call_median": med, "min": min(s), "max": max(s),
                         "weight_GB_per_s_at_median": r["weight_bytes"] / med / 1e3}
        med = {side: row[side]["us_per_call_median"] for side in sides if side in row}
        row["fused_over_unfused"] = med["fused"] / med["unfused"]
        row["rows_over_fused"] = med["rows"] / med["fused"]
        row["rows_over_unfused"] = med["rows"] / med["unfused"]
        # the claim of the row split: faster than fused by more than fused's own min-max spread
        row["rows_beats_fused_by_more_than_fuseds_spread"] = med["fused"] - med["rows"] > row["fused"]["max"] - row["fused"]["min"]
        names = {"fused": "fused", "rows": "rows", "unfused": "unfused (hipBLASLt and its neighbours)"}
        row["faster"] = names[min(names, key=med.get)]
        out[call] = row
    return out


def parity(dev, out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import t5_decode_linear_checks as L
    res = {"tool": "tools/t5_decode_linear_bench.py --parity", "device": torch.cuda.get_device_name(0),
           "rule": "max|kernel - float64| <= 2 * max|unfused - float64| + one bf16 ulp of max|float64|; ratio = left / right",
           "shapes": "tests/t5_decode_linear_checks.py shapes(): M {1,3,16,17,33} x N {16,48,80} x K {32,96,256}, both sides "
                     "of every K break, the M breaks, K 16384", "combinations": {}}
    with torch.no_grad():
        for combo in L.COMBOS:
            norm, (_, with_res, act, gated) = combo
            worst = dict(ratio=0.0)
            for M, N, K in L.shapes(norm):
                x, w, nw, r = L.inputs(M, N, K, gated, seed=1000 * K + 10 * N + M, device=dev)
                kw = dict(norm_w=nw if norm else None, residual=r if with_res else None, act=act, gated=gated)
                ref = L.oracle(x, w, **kw)
                e_u = L.max_err(L.unfused(x, w, **kw), ref)
                got = P.t5_decode_linear(x, w, norm_weight=kw["norm_w"], residual=kw["residual"], act=act, gated=gated)
                e_k = L.max_err(got, ref)
                ratio = e_k / L.bound(e_u, ref)
                if ratio > worst["ratio"]:
                    worst = dict(ratio=ratio, M=M, N=N, K=K, e_kernel=e_k, e_unfused=e_u, bound=L.bound(e_u, ref))
            res["combinations"][L.combo_name(combo)] = worst
            print(L.combo_name(combo), json.dumps(worst))
    res["worst_ratio"] = max(v["ratio"] for v in res["combinations"].values())
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8,32,64,128,256")
    ap.add_argument("--shapes", default="t5_base,d_model_4096")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P.load_library()
    if args.parity:
        return parity(dev, args.out or os.path.join(ROOT, "profiles", "t5_decode_linear_parity.json"))
    result = {"tool": "tools/t5_decode_linear_bench.py", "device": torch.cuda.get_device_name(0), "dtype": "bf16",
              "shapes": SHAPES, "act": ACT, "rows_geometry": sys.modules[P.__name__ + ".t5_decode_linear"].rows_geometry(),
              "routes": "fused = trlx_t5_decode_linear; rows = trlx_t5_decode_linear_rows (split_rows=True); rows_live_F = rows "
                        f"with live= at live fraction F (M {LIVE_AT_M} only); unfused = torch.matmul and its neighbours",
              "timing": f"one captured graph of {CALLS} back-to-back calls per route, rotating over {COPIES} copies of the "
                        f"weights and buffers; routes interleaved and shuffled per repetition; HIP events around one replay / "
                        f"{CALLS}; median of {args.reps} with min-max, microseconds per call"}
    for name in args.shapes.split(","):
        for M in (int(m) for m in args.rows.split(",")):
            result[f"{name}_M{M}"] = run_shape(name, M, dev, args.reps)
            print(f"{name} M {M}: " + json.dumps({k: {s: round(v[s]["us_per_call_median"], 2) for s in sides_of(M) if s in v}
                                                  for k, v in result[f"{name}_M{M}"].items()}))
            torch.cuda.empty_cache()
    out = args.out or os.path.join(ROOT, "profiles", "t5_decode_linear_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
