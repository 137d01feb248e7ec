"""T5's layer norm with the residual add before it, four routes, forward alone and forward + backward
(giving dh and dw), at seven bf16 shapes.

  with the add      hf_eager    residual + x, then HF's T5LayerNorm op sequence; autograd keeps the fp32
                                upcast and the normalised tensor
                    torch_best  residual + x, then torch.nn.functional.rms_norm
                    fused       t5_add_rmsnorm (trlx_t5_rmsnorm_fwd / _bwd): one launch forward
  the norm alone    hf_eager_norm / torch_best_norm / fused_norm (t5_rmsnorm) on the same h
Forward + backward differentiates y (and, with the add, h) with fixed dy and dh_in and gives the
gradients of x (or h) and weight.  The routes run interleaved in one process on the same tensors,
their order shuffled per repetition, timed with HIP events after warm-up; medians of --reps (default
20).  A difference inside 5 % is reported as "tie".
Byte model of the fused routes (s = 2 B): forward 4 N D s with the add (read x, residual, write h,
y), 2 N D s alone; backward 4 N D s with the add (read dy, h, dh_in, write dh), 3 N D s alone, plus
the fp32 partials written and read, 2 G D 4 B.  TB/s is that over the median; forward + backward is
timed as one call, its TB/s is over the sum of both models.
Peak memory: the rise of torch.cuda.max_memory_allocated over one forward + backward per route, the
operands and gradients-in already allocated.

One JSON record is printed and written to --out.
GPU-box tool:  python tools/t5_rmsnorm_bench.py [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (N, d_model)
SHAPES = {
    "t5_base_enc_N32768": (32768, 768),
    "t5_base_enc_N131072": (131072, 768),
    "t5_base_dec_N12288": (12288, 768),
    "t5_base_decode_step_N256": (256, 768),
    "t5_large_N32768": (32768, 1024),
    "ul2_like_N16384": (16384, 4096),
    "t5_small_N32768": (32768, 512),
}
EPS = 1e-6


def hf_norm(torch, h, w):
    variance = h.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + EPS)
    if w.dtype in (torch.float16, torch.bfloat16):
        h = h.to(w.dtype)
    return w * h


def bench(torch, P, fb, N, D, dev, reps, warmup, stream, rng):
    import torch.nn.functional as F
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(N + D)
    x = torch.randn(N, D, generator=g, device=dev).to(dtype).requires_grad_()
    r = (3 * torch.randn(N, D, generator=g, device=dev) + 0.5).to(dtype)
    w = (1 + 0.3 * torch.randn(D, generator=g, device=dev)).to(dtype).requires_grad_()
    dy = torch.randn(N, D, generator=g, device=dev).to(dtype)
    dh_in = torch.randn(N, D, generator=g, device=dev).to(dtype)
    hsum = (r + x).detach().requires_grad_()
    keep = {}

    def add_route(norm):
        def fn():
            h = r + x
            return h, norm(h)
        return fn

    def route(fn, wrt, gin):
        def fwd():
            with torch.no_grad():
                keep["y"] = fn()

        def both():
            out = fn()
            keep["g"] = torch.autograd.grad(out, wrt, gin)
        return fwd, both

    add = {"hf_eager": route(add_route(lambda h: hf_norm(torch, h, w)), [x, w], [dh_in, dy]),
           "torch_best": route(add_route(lambda h: F.rms_norm(h, (D,), w, EPS)), [x, w], [dh_in, dy]),
           "fused": route(lambda: P.t5_add_rmsnorm(x, r, w, EPS), [x, w], [dh_in, dy])}
    alone = {"hf_eager_norm": route(lambda: hf_norm(torch, hsum, w), [hsum, w], dy),
             "torch_best_norm": route(lambda: F.rms_norm(hsum, (D,), w, EPS), [hsum, w], dy),
             "fused_norm": route(lambda: P.t5_rmsnorm(hsum, w, EPS), [hsum, w], dy)}
    geo = P.t5_norm.geometry(N, D)
    nd = N * D * 2
    part = 2 * geo["partials"] * D * 4
    model = {"add": {"forward": 4 * nd, "forward_backward": 8 * nd + part},
             "norm": {"forward": 2 * nd, "forward_backward": 5 * nd + part}}
    rec = {"N": N, "D": D, "partials_G": geo["partials"], "rows_per_block": geo["rows_per_block"], "byte_model": model}
    for kind, routes, mine in (("add", add, "fused"), ("norm", alone, "fused_norm")):
        rec[kind] = {}
        for i, what in enumerate(("forward", "forward_backward")):
            fns = {n: rt[i] for n, rt in routes.items()}
            ms = {n: fb.summary(t) for n, t in fb.interleaved(fns, reps, warmup, stream, rng).items()}
            rec[kind][what] = {**ms, "fastest": fb.fastest(ms),
                               f"{mine}_TB_per_s": round(model[kind][what] / (ms[mine]["median_ms"] * 1e-3) / 1e12, 2)}
        grads = {}
        for n, rt in routes.items():                             # results against each other, and peak memory
            rt[1]()
            grads[n] = [t.float() for t in keep.pop("g")]
            keep.clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            rt[1]()
            torch.cuda.synchronize()
            rec[kind][f"{n}_peak_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
            keep.clear()
        rec[kind]["max_abs_grad_diff_vs_fused"] = {
            n: [float((a - b).abs().max()) for a, b in zip(grads[n], grads[mine])] for n in grads if n != mine}
    rec["one_tensor_MB"] = round(nd / 1e6, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape's name")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    import __graft_entry__
    P = __graft_entry__.load_package()
    import t5_attention_bench as fb
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = random.Random(0)
    geo = P.t5_norm.geometry()
    rec = {"tool": "t5_rmsnorm_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "dtype": "bf16",
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "geometry": {k: (list(v) if isinstance(v, tuple) else v) for k, v in geo.items()},
           "byte_model": "fused routes, s = 2 B: forward 4 N D s with the add, 2 N D s alone; backward 4 N D s with the "
                         "add (dh_in read), 3 N D s alone, plus 2 G D 4 B of partials",
           "shapes": {}}
    for name, shape in SHAPES.items():
        if args.only and name != args.only:
            continue
        rec["shapes"][name] = bench(torch, P, fb, *shape, dev, args.reps, args.warmup, stream, rng)
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
