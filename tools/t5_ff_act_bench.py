"""T5's feed-forward activation between the projections, four routes, forward alone and forward +
backward, at six bf16 shapes.

  hf_eager   HF's op sequence: NewGELUActivation's nine elementwise ops / F.silu / relu, then the
             multiply; autograd keeps every intermediate
  torch_best torch's best native form: F.gelu(u, approximate="tanh") * v, F.silu(u) * v, F.relu(u)
  fused      t5_ff_act on separate u and v (trlx_t5_ff_act_fwd / _bwd)
  packed     t5_ff_act_packed on one [N, 2F] tensor holding the same u | v (gated shapes only)
Forward + backward gives gradients for u and v (one [N, 2F] gradient for `packed`) from a fixed dy.
The routes run interleaved in one process on the same tensors, their order shuffled per
repetition, timed with HIP events after warm-up; medians of --reps (default 20).  A difference
inside 5 % is reported as "tie".
Byte model of the fused routes: 3 N F 2 B forward (read u, read v, write y) and 5 N F 2 B backward
(read dy, u, v, write du, dv); 2 and 3 when not gated.  TB/s is that over the median; forward +
backward is timed as one call, its TB/s is over the sum of both models.
Peak memory: the rise of torch.cuda.max_memory_allocated over one forward + backward per route, the
operands and dy already allocated.

One JSON record is printed and written to --out.
GPU-box tool:  python tools/t5_ff_act_bench.py [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (N, d_ff, activation, gated)
SHAPES = {
    "t5v11_base_enc_B64_S512": (32768, 2048, "gelu_new", True),
    "t5v11_base_enc_B256_S512": (131072, 2048, "gelu_new", True),
    "t5v11_base_dec_B256_T48": (12288, 2048, "gelu_new", True),
    "t5v11_base_decode_step_B256": (256, 2048, "gelu_new", True),
    "ul2_like_N16384": (16384, 16384, "silu", True),
    "t5_base_ungated_B64_S512": (32768, 3072, "relu", False),
}


def bench(torch, P, fb, N, F_, act, gated, dev, reps, warmup, stream, rng):
    import math
    import torch.nn.functional as F
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(N + F_)
    u = torch.randn(N, F_, generator=g, device=dev).to(dtype).requires_grad_()
    v = torch.randn(N, F_, generator=g, device=dev).to(dtype).requires_grad_() if gated else None
    uv = torch.cat([u.detach(), v.detach()], dim=1).requires_grad_() if gated else None
    dy = torch.randn(N, F_, generator=g, device=dev).to(dtype)
    leaves = [u, v] if gated else [u]
    keep = {}

    def hf_act(u):
        if act == "gelu_new":
            return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * torch.pow(u, 3.0))))
        return F.silu(u) if act == "silu" else F.relu(u)

    def best_act(u):
        if act == "gelu_new":
            return F.gelu(u, approximate="tanh")
        return F.silu(u) if act == "silu" else F.relu(u)

    def route(fn, wrt):
        def fwd():
            with torch.no_grad():
                keep["y"] = fn()

        def both():
            keep["g"] = torch.autograd.grad(fn(), wrt, dy)
        return fwd, both

    def of(a):
        return lambda: a(u) if v is None else a(u) * v

    routes = {"hf_eager": route(of(hf_act), leaves), "torch_best": route(of(best_act), leaves),
              "fused": route(lambda: P.t5_ff_act(u, v, act), leaves)}
    if gated:
        routes["packed"] = route(lambda: P.t5_ff_act_packed(uv, act), [uv])
    rec = {"N": N, "d_ff": F_, "act": act, "gated": gated}
    nf = N * F_ * 2
    model = {"forward": (3 if gated else 2) * nf, "forward_backward": ((3 + 5) if gated else (2 + 3)) * nf}
    rec["byte_model"] = model
    grads = {}
    for i, what in enumerate(("forward", "forward_backward")):
        fns = {n: r[i] for n, r in routes.items()}
        ms = {n: fb.summary(t) for n, t in fb.interleaved(fns, reps, warmup, stream, rng).items()}
        rec[what] = {**ms, "fastest": fb.fastest(ms)}
        for n in ("fused", "packed"):
            if n in ms:
                rec[what][f"{n}_TB_per_s"] = round(model[what] / (ms[n]["median_ms"] * 1e-3) / 1e12, 2)
    for n, r in routes.items():                                  # results against each other, and peak memory
        r[1]()
        grads[n] = torch.cat([x.float() for x in keep.pop("g")], dim=1)
        keep.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r[1]()
        torch.cuda.synchronize()
        rec[f"{n}_peak_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
        keep.clear()
    rec["one_tensor_MB"] = round(nf / 1e6, 1)
    rec["max_abs_grad_diff_vs_fused"] = {n: float((grads[n] - grads["fused"]).abs().max()) for n in grads if n != "fused"}
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
    rec = {"tool": "t5_ff_act_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "dtype": "bf16",
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "geometry": {"vec_bf16": P.t5_ff.VEC_BF16, "cols_per_block": P.t5_ff.COLS_PER_BLOCK,
                        "rows_per_block": P.t5_ff.ROWS_PER_BLOCK},
           "byte_model": "fused routes: forward 3 N F 2 B, backward 5 N F 2 B (2 and 3 not gated)", "shapes": {}}
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
