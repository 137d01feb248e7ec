"""t5_decode_linear_w8 (fp8 weights) against t5_decode_linear (bf16) and hipBLASLt with its neighbour
launches, per call of a decode layer, inside replayed graphs.

Routes: `hipblaslt` (torch.matmul, t5_rmsnorm in front, the bf16 add or t5_ff_act_packed behind),
`bf16` (trlx_t5_decode_linear) and `w8_4` / `w8_8` / `w8_16` (trlx_t5_decode_linear_w8 at each wave
count).  Calls (K -> N) at M 8, 32, 128, 256 for T5-base (D 768, inner 768, F 2048), d_model 2048 (inner
2048, F 5120) and d_model 4096 (inner 4096, F 10240), all gated gelu_new:

  norm_qkv, o_residual, norm_cq, norm_wi_act, wo_residual      the five distinct calls of a layer
  layer_chain     the six projections back to back (the attentions left out: stand-in buffers)
  lm_head         N 32128 at each D, plain
  quantize_block  t5_quantize_linear_weight over the six weights of a block (six launches), M-free

The method is tools/t5_decode_linear_bench.py's: each route is ONE captured graph of 64 back-to-back
calls rotating over 8 copies of the weights and buffers (a layer's weights are not L2-hot when its
turn comes); routes interleaved, their order shuffled per repetition; a sample is one replay between
two HIP events divided by 64; the figure is the median of --reps with min-max in microseconds per call,
and TB/s over the weight bytes the route actually reads (fp8: one byte an element plus the scales).
No speed-up is assumed: every row names its fastest route.

--parity: the accuracy sweep of tests/test_gpu_t5_decode_linear_w8.py (its shapes, the float64 oracle
on dequantize(), t5_decode_linear on dequantize()) and the worst ratio per combination, written to
profiles/t5_decode_linear_w8_parity.json.

    python tools/t5_decode_linear_w8_bench.py [--parity] [--reps 20] [--rows 8,32,128,256]
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
SHAPES = {"t5_base": dict(D=768, inner=768, F=2048), "d_model_2048": dict(D=2048, inner=2048, F=5120),
          "d_model_4096": dict(D=4096, inner=4096, F=10240)}
ACT, VOCAB = "gelu_new", 32128
WAVES = (4, 8, 16)
ROUTES = ("hipblaslt", "bf16") + tuple(f"w8_{w}" for w in WAVES)


def layer_calls(D, inner, F):
    """name -> (K, weight rows, kwargs of the fused call)"""
    return {"norm_qkv": (D, 3 * inner, dict(norm=True)), "o_residual": (inner, D, dict(residual=True)),
            "norm_cq": (D, inner, dict(norm=True)), "norm_wi_act": (D, 2 * F, dict(norm=True, act=ACT, gated=True)),
            "wo_residual": (F, D, dict(residual=True)), "lm_head": (D, VOCAB, {})}


def make_call(K, rows, spec, M, dev, route, g):
    """fn(i) running call copy i % COPIES, and the weight bytes it reads."""
    gated = spec.get("gated", False)
    N = rows // 2 if gated else rows
    ws = [(torch.randn(rows, K, generator=g, device=dev) / K ** 0.5).to(DT) for _ in range(COPIES)]
    xs = [torch.randn(M, K, generator=g, device=dev).to(DT) for _ in range(COPIES)]
    nw = torch.ones(K, dtype=DT, device=dev) if spec.get("norm") else None
    hs = [torch.randn(M, N, generator=g, device=dev).to(DT) for _ in range(COPIES)] if spec.get("residual") else None
    outs = [torch.empty(M, N, dtype=DT, device=dev) for _ in range(COPIES)]
    kw = dict(norm_weight=nw, act=spec.get("act"), gated=gated)
    if route == "hipblaslt":
        def fn(i):
            c = i % COPIES
            y = xs[c] if nw is None else P.t5_rmsnorm(xs[c], nw)
            z = torch.matmul(y, ws[c].t())
            if hs is not None:
                hs[c].add_(z)
            elif gated:
                P.t5_ff_act_packed(z, ACT)
        return fn, rows * K * 2
    if route == "bf16":
        def fn(i):
            c = i % COPIES
            P.t5_decode_linear(xs[c], ws[c], residual=None if hs is None else hs[c], out=outs[c] if hs is None else hs[c], **kw)
        return fn, rows * K * 2
    w8s = [P.t5_quantize_linear_weight(w) for w in ws]
    del ws
    waves = int(route.split("_")[1])

    def fn(i):
        c = i % COPIES
        P.t5_decode_linear_w8(xs[c], w8s[c], residual=None if hs is None else hs[c], out=outs[c] if hs is None else hs[c],
                              waves=waves, **kw)
    return fn, rows * K + rows * 4


def capture(fn):
    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(CALLS):
            fn(i)
    return graph


def measure(graphs, reps, seed):
    keys = list(graphs)
    samples = {k: [] for k in keys}
    rng = random.Random(seed)
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
    return samples


def run_shape(name, M, dev, reps):
    calls = layer_calls(**SHAPES[name])
    graphs, nbytes, alive = {}, {}, []
    with torch.no_grad():
        for route in ROUTES:
            fns = {}
            for call, (K, rows, spec) in calls.items():
                fn, nb = make_call(K, rows, spec, M, dev, route, torch.Generator(device=dev).manual_seed(M))
                fns[call], nbytes[(call, route)] = fn, nb
                graphs[(call, route)] = capture(fn)
            chain = [fns[c] for c in ("norm_qkv", "o_residual", "norm_cq", "o_residual", "norm_wi_act", "wo_residual")]
            nbytes[("layer_chain", route)] = sum(nbytes[(c, route)] for c in
                                                 ("norm_qkv", "o_residual", "norm_cq", "o_residual", "norm_wi_act", "wo_residual"))
            graphs[("layer_chain", route)] = capture(lambda i, chain=chain: [f(i) for f in chain])
            alive.append(fns)
        samples = measure(graphs, reps, M)
    out = {}
    for call in list(calls) + ["layer_chain"]:
        row = {}
        for route in ROUTES:
            s = samples[(call, route)]
            med = statistics.median(s)
            row[route] = {"us_median": med, "min": min(s), "max": max(s), "weight_bytes": nbytes[(call, route)],
                          "weight_TB_per_s": nbytes[(call, route)] / med / 1e6}
        med = {r: row[r]["us_median"] for r in ROUTES}
        row["fastest"] = min(med, key=med.get)
        row["fastest_w8"] = min((r for r in ROUTES if r.startswith("w8")), key=med.get)
        row["w8_loses_to"] = [r for r in ("hipblaslt", "bf16") if med[r] <= med[row["fastest_w8"]]]
        out[call] = row
    return out


def run_quantize(name, dev, reps):
    D, inner, F = (SHAPES[name][k] for k in ("D", "inner", "F"))
    shapes = [(3 * inner, D), (D, inner), (inner, D), (D, inner), (2 * F, D), (D, F)]
    with torch.no_grad():
        ws = [[torch.randn(n, k, device=dev).to(DT) for n, k in shapes] for _ in range(2)]
        outs = [[P.t5_quantize_linear_weight(w) for w in blk] for blk in ws]
        graph = capture(lambda i: [P.t5_quantize_linear_weight(w, out=o) for w, o in zip(ws[i % 2], outs[i % 2])])
        s = measure({"q": graph}, reps, 0)["q"]
    nb = sum(n * k * 3 for n, k in shapes)      # bf16 read (twice, the second from cache), bytes written
    med = statistics.median(s)
    return {"us_median_per_block": med, "min": min(s), "max": max(s), "launches": 6, "bf16_read_plus_fp8_written_bytes": nb,
            "TB_per_s": nb / med / 1e6}


def parity(dev, out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import t5_decode_linear_checks as L
    import test_gpu_t5_decode_linear_w8 as T
    res = {"tool": "tools/t5_decode_linear_w8_bench.py --parity", "device": torch.cuda.get_device_name(0),
           "rule": "max|kernel - float64| <= 2 * max|t5_decode_linear - float64| + one bf16 ulp of max|float64|, all three on "
                   "w8.dequantize(); ratio = left / right",
           "shapes": "tests/test_gpu_t5_decode_linear_w8.py w8_shapes(): waves 4 / 8 / 16 forced, N 16 (48 once), M {1,16,17,33} "
                     "over K {64,192,256,320,256 WV,256 WV+64,512 WV+64}, M {65,129,257} at K 320", "combinations": {}}
    with torch.no_grad():
        for combo in L.COMBOS:
            norm, (_, with_res, act, gated) = combo
            worst = dict(ratio=0.0)
            for wv, M, N, K in T.w8_shapes(norm, gated):
                x, w, nw, r = L.inputs(M, N, K, gated, seed=1000 * K + 10 * N + M, device=dev)
                w8 = P.t5_quantize_linear_weight(w)
                kw = dict(norm_weight=nw if norm else None, residual=r if with_res else None, act=act, gated=gated)
                ref = L.oracle(x, w8.dequantize(), kw["norm_weight"], 1e-6, kw["residual"], act, gated)
                e_b = L.max_err(P.t5_decode_linear(x, w8.dequantize(), **kw), ref)
                e_k = L.max_err(P.t5_decode_linear_w8(x, w8, waves=wv, **kw), ref)
                ratio = e_k / L.bound(e_b, ref)
                if ratio > worst["ratio"]:
                    worst = dict(ratio=ratio, waves=wv, M=M, N=N, K=K, e_kernel=e_k, e_bf16=e_b, bound=L.bound(e_b, ref))
            res["combinations"][L.combo_name(combo)] = worst
            print(L.combo_name(combo), json.dumps(worst))
    res["worst_ratio"] = max(v["ratio"] for v in res["combinations"].values())
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="8,32,128,256")
    ap.add_argument("--shapes", default="t5_base,d_model_2048,d_model_4096")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P.load_library()
    if args.parity:
        return parity(dev, args.out or os.path.join(ROOT, "profiles", "t5_decode_linear_w8_parity.json"))
    geo = P.t5_linear_w8.linear_w8_geometry
    result = {"tool": "tools/t5_decode_linear_w8_bench.py", "device": torch.cuda.get_device_name(0), "shapes": SHAPES, "act": ACT,
              "routes": "hipblaslt = torch.matmul and its neighbour launches; bf16 = trlx_t5_decode_linear; w8_W = "
                        "trlx_t5_decode_linear_w8 at W waves",
              "timing": f"one captured graph of {CALLS} back-to-back calls per route, rotating over {COPIES} copies of the weights "
                        f"and buffers; routes interleaved and shuffled per repetition; HIP events around one replay / {CALLS}; "
                        f"median of {args.reps} with min-max, microseconds per call; TB/s over the weight bytes the route reads"}
    out = args.out or os.path.join(ROOT, "profiles", "t5_decode_linear_w8_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for name in args.shapes.split(","):
        calls = layer_calls(**SHAPES[name])
        result[f"{name}_default_waves"] = {c: geo(rows // 2 if s.get("gated") else rows, K, s.get("gated", False))["waves"]
                                           for c, (K, rows, s) in calls.items()}
        result[f"{name}_quantize_block"] = run_quantize(name, dev, args.reps)
        for M in (int(m) for m in args.rows.split(",")):
            result[f"{name}_M{M}"] = run_shape(name, M, dev, args.reps)
            print(f"{name} M {M}: " + json.dumps({k: {r: round(v[r]["us_median"], 2) for r in ROUTES}
                                                  for k, v in result[f"{name}_M{M}"].items()}), flush=True)
            torch.cuda.empty_cache()
            with open(out, "w") as fh:                            # after every shape: a long run leaves what it has
                json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
