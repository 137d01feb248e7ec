"""T5's full-sequence attention, forward + backward, three routes, at tools/t5_attention_bench.py's
nine shapes.

  eager   HF's eager op sequence under autograd: matmul, position_bias = weight-table gathered to
          [1, nH, Tq, S] plus the additive finfo.min mask, fp32 softmax cast back, matmul; autograd
          keeps the [B, nH, Tq, S] tensors
  sdpa    F.scaled_dot_product_attention with the same bias + mask tensor as attn_mask (it requires
          grad through the table) and scale=1.0
  fused   t5_attention_train (trlx_t5_attention_fwd_lse + trlx_t5_attention_bwd, nothing of size
          Tq x S), the table a differentiable leaf too
Each timed call is one forward and one backward from a fixed dO, giving gradients for q, k, v and
(where the shape has a bias) the [nH, Tq + S - 1] table.  The routes run interleaved in one process
on the same tensors, their order shuffled per repetition, timed with HIP events after warm-up;
medians of --reps (default 20).  A difference inside 5 % is reported as "tie".
FLOP model: forward 4·nH·d·sum_b Tq·S_live(b) (causal: the keys j <= i), backward 2.5x that as
mathematics (dP, dV, dK, dQ and the recomputed S); the fused route executes 3.5x (S and dP in both
of its walks).  TFLOP/s is reported over forward x 3.5 = forward + the backward's mathematical
2.5x, the same useful work for every route.
Peak memory: the rise of torch.cuda.max_memory_allocated over one forward + backward per route,
operands and dO already allocated.

--forward-ab PARENT_LIB: the existing forward against an earlier build of the library.  The fused
forward (t5_attention under no_grad) at two encoder shapes in alternating child processes, four
each, TRLX_T5_AMD_LIB naming the library; the new library's median of medians has to lie inside the
earlier library's own min-max spread.  Recorded as "forward_ab".

One JSON record is printed and written to --out.
GPU-box tool:  python tools/t5_attention_bwd_bench.py [--reps N] [--out FILE] [--only NAME] [--forward-ab LIB]"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AB_SHAPES = ("t5base_enc_B64_S512", "t5base_enc_B256_S512_leftpad")


def _load():
    """torch, the package and the forward tool's helpers.  An earlier build of the library named by
    TRLX_T5_AMD_LIB lacks the entries added since: the binding then keeps the ones it has."""
    import ctypes
    import torch
    import __graft_entry__
    P = __graft_entry__.load_package()
    from trlx_t5_amd import _lib
    if os.environ.get("TRLX_T5_AMD_LIB"):
        have = ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
            del _lib.SIGNATURES[name]
    return torch, P


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "n": len(s)}


def fastest(ms):
    order = sorted(ms, key=lambda k: ms[k]["median_ms"])
    if ms[order[0]]["median_ms"] >= 0.95 * ms[order[1]]["median_ms"]:
        return "tie: " + " / ".join(sorted(order[:2]))
    return order[0]


def bench(torch, P, fb, mode, B, nH, d, Tq, S, padded, dev, reps, warmup, stream, rng):
    import torch.nn.functional as F
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(Tq * 1000 + S + B)
    s = d ** -0.25
    q = (torch.randn(B, Tq, nH * d, generator=g, device=dev) * s).to(dtype).requires_grad_()
    k = (torch.randn(B, S, nH * d, generator=g, device=dev) * s).to(dtype).requires_grad_()
    v = torch.randn(B, S, nH * d, generator=g, device=dev).to(dtype).requires_grad_()
    weight = torch.randn(32, nH, generator=g, device=dev)
    dout = torch.randn(B, Tq, nH * d, generator=g, device=dev).to(dtype)
    causal = mode == "decoder"
    table = None if mode == "cross" else P.t5_relative_bias_offsets(weight, Tq, S, mode == "encoder").requires_grad_()
    mask = None
    live = torch.full((B,), S, dtype=torch.long, device=dev)
    if padded:
        live = torch.randint(S // 4, S + 1, (B,), generator=g, device=dev)              # U{128..512} live keys
        mask = (torch.arange(S, device=dev)[None, :] >= (S - live)[:, None]).long()
    rel = torch.arange(S, device=dev)[None, :] - torch.arange(Tq, device=dev)[:, None]
    fixed = torch.zeros(1, 1, Tq, S, dtype=dtype, device=dev)                           # the part without a gradient
    if mask is not None:
        fixed = fixed + torch.zeros(B, 1, 1, S, dtype=dtype, device=dev).masked_fill((mask == 0)[:, None, None, :],
                                                                                     torch.finfo(dtype).min)
    if causal:
        fixed = fixed + torch.zeros(Tq, S, dtype=dtype, device=dev).masked_fill(rel > 0, torch.finfo(dtype).min)[None, None]
    leaves = [q, k, v] + ([] if table is None else [table])
    keep = {}

    def position_bias():
        """HF's position_bias + mask for one stack; with a table it carries the gradient."""
        return fixed if table is None else table[:, rel + (Tq - 1)].to(dtype)[None] + fixed

    def views():
        return (x.view(B, -1, nH, d).transpose(1, 2) for x in (q, k, v))                # HF's [B, nH, T, d] views

    def eager():
        q4, k4, v4 = views()
        scores = torch.matmul(q4, k4.transpose(3, 2)) + position_bias()
        w = torch.softmax(scores.float(), dim=-1).type_as(scores)
        out = torch.matmul(w, v4).transpose(1, 2).reshape(B, Tq, nH * d)
        keep["eager"] = torch.autograd.grad(out, leaves, dout)

    def sdpa():
        q4, k4, v4 = views()
        out = F.scaled_dot_product_attention(q4, k4, v4, attn_mask=position_bias(), scale=1.0) \
            .transpose(1, 2).reshape(B, Tq, nH * d)
        keep["sdpa"] = torch.autograd.grad(out, leaves, dout)

    def fused():
        out = P.t5_attention_train(q, k, v, bias=table, key_mask=mask, causal=causal, n_heads=nH)
        keep["fused"] = torch.autograd.grad(out, leaves, dout)

    fns = {"eager": eager, "sdpa": sdpa, "fused": fused}
    ms = {n: summary(t) for n, t in fb.interleaved(fns, reps, warmup, stream, rng).items()}
    pairs = Tq * (Tq + 1) // 2 * B if causal else int(live.sum()) * Tq
    fwd_flop = 4 * nH * d * pairs
    flop = int(3.5 * fwd_flop)
    rec = {"mode": mode, "B": B, "nH": nH, "d_kv": d, "Tq": Tq, "S": S, "left_padded": padded,
           "live_keys_mean": round(float(live.float().mean()), 1), **ms, "fastest": fastest(ms),
           "forward_flop": fwd_flop, "flop": flop}
    for n in ms:
        rec[f"{n}_TFLOP_per_s"] = round(flop / (ms[n]["median_ms"] * 1e-3) / 1e12, 1)
    names = ["dq", "dk", "dv"] + ([] if table is None else ["dbias"])
    for other in ("eager", "sdpa"):
        rec[f"max_abs_diff_fused_vs_{other}"] = {n: float((a.float() - b.float()).abs().max())
                                                 for n, a, b in zip(names, keep["fused"], keep[other])}
    keep.clear()
    for n, fn in fns.items():                                                            # peak memory, one call each
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        rec[f"{n}_peak_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
        keep.clear()
    rec["one_bf16_score_tensor_MB"] = round(B * nH * Tq * S * 2 / 1e6, 1)
    return rec


def forward_child(reps, warmup):
    """The fused forward alone at AB_SHAPES with whichever library TRLX_T5_AMD_LIB names: one JSON line."""
    torch, P = _load()
    import t5_attention_bench as fb
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = random.Random(0)
    out = {}
    for name in AB_SHAPES:
        out[name] = fb.bench(*fb.SHAPES[name], dev, reps, warmup, stream, rng)["fused"]["median_ms"]
    print("FORWARD_AB " + json.dumps(out), flush=True)


def forward_ab(parent_lib, reps, warmup, runs=4):
    """Alternating child processes, `runs` each; a child that fails ends the A/B (nothing more is started)."""
    parent_lib = os.path.abspath(parent_lib)
    got = {"parent": {n: [] for n in AB_SHAPES}, "new": {n: [] for n in AB_SHAPES}}
    for _ in range(runs):
        for which in ("parent", "new"):
            env = dict(os.environ)
            env.pop("TRLX_T5_AMD_LIB", None)
            if which == "parent":
                env["TRLX_T5_AMD_LIB"] = parent_lib
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-child", "--reps", str(reps),
                                  "--warmup", str(warmup)], env=env, check=True, timeout=300,
                                 stdout=subprocess.PIPE, text=True).stdout
            line = [ln for ln in txt.splitlines() if ln.startswith("FORWARD_AB ")][-1]
            for n, ms in json.loads(line[len("FORWARD_AB "):]).items():
                got[which][n].append(ms)
    rec = {"what": "t5_attention forward (tools/t5_attention_bench.py's fused route) with the earlier library and with "
                   "this one, alternating child processes, medians of %d per run" % reps, "runs_each": runs, "shapes": {}}
    for n in AB_SHAPES:
        p, w = sorted(got["parent"][n]), sorted(got["new"][n])
        med = (w[len(w) // 2 - 1] + w[len(w) // 2]) / 2 if len(w) % 2 == 0 else w[len(w) // 2]
        rec["shapes"][n] = {"parent_median_ms": got["parent"][n], "new_median_ms": got["new"][n],
                            "parent_min_ms": p[0], "parent_max_ms": p[-1], "new_median_of_medians_ms": round(med, 4),
                            "inside_parent_spread": p[0] <= med <= p[-1], "not_slower_than_parent_max": med <= p[-1]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape's name")
    ap.add_argument("--forward-ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--forward-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if args.forward_child:
        return forward_child(args.reps, args.warmup)
    # the A/B's children come first: this process has not opened the GPU yet
    ab = forward_ab(args.forward_ab, args.reps, args.warmup) if args.forward_ab else None
    torch, P = _load()
    import t5_attention_bench as fb
    TR = P.t5_attention_train
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = random.Random(0)
    rec = {"tool": "t5_attention_bwd_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "dtype": "bf16",
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "tiles": {"dq_q": TR.DQ_Q_TILE, "dq_kv": TR.DQ_KV_TILE, "dkv_k": TR.DKV_K_TILE, "dkv_q": TR.DKV_Q_TILE},
           "flop_model": "flop = 3.5 x forward_flop; forward_flop = 4 nH d sum_b Tq S_live(b) (causal: j <= i)",
           "shapes": {}}
    for name, shape in fb.SHAPES.items():
        if args.only and name != args.only:
            continue
        rec["shapes"][name] = bench(torch, P, fb, *shape, dev, args.reps, args.warmup, stream, rng)
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
    if ab is not None:
        rec["forward_ab"] = ab
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
