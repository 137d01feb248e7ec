"""The optimizer step of a bf16 model with torch's state layout (bf16 exp_avg / exp_avg_sq) against
the fp32-state step, at the bf16 shapes of tools/adamw_bench.py: the lm_head weight [50257, 768]
and the PPO value head.  Routes on the same parameters and gradients, interleaved in one process,
timed with HIP events after warm-up (medians of --reps):

  torch_foreach        torch.optim.AdamW (bf16 state)
  torch_fused          torch.optim.AdamW(fused=True) (bf16 state), where this torch build takes it
  fused_fp32_state     FusedAdamW                         22 B per parameter
  fused_param_state    FusedAdamW(state_dtype="param")    14 B per parameter
  fused_fp32_state_clipped / fused_param_state_clipped
                       .step(max_grad_norm=1.0): one more read of the gradients, 24 B / 16 B

The order of the routes is shuffled (seeded) for every repetition: on the launch-bound value head
a step's event time is the host's time in step() unless the queue still holds the previous
route's kernels, so a fixed order would favour whichever route follows the slowest one.

Rates are over those byte models; from bytes alone the bf16 state is bounded at 22/14 = 1.57x
over the fp32 state.  The fastest route per shape is named, whichever it is; a difference inside
5 % is reported as "not faster".

--ab-parent-lib FILE: the fp32-state step must not slow down — tools/grad_clip_bench.py's
unclipped_step_ab (route d at the ILQL-heads shape with the parent commit's library and with
this tree's, child processes in alternation, --ab-rounds each).  One JSON line.
GPU-box tool:  python tools/adamw_bf16_state_bench.py [--reps N] [--ab-parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from adamw_bench import H, V, HYPER, timed, summary, verdict, with_grads, torch_fused_or_reason  # noqa: E402
from grad_clip_bench import ab_unclipped  # noqa: E402

MAX_NORM = 1.0
BYTES = {"fused_fp32_state": 22, "fused_param_state": 14, "fused_fp32_state_clipped": 24,
         "fused_param_state_clipped": 16}


def interleaved(fns, reps, warmup, stream):
    """{name: [ms, ...]} of functions run in alternation, in a new seeded order every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    names, rng = list(fns), random.Random(0)
    evs = {k: [] for k in fns}
    for _ in range(reps):
        rng.shuffle(names)
        for k in names:
            evs[k].append(timed(fns[k], stream))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def bench_shape(name, params, args, stream):
    n = sum(p.numel() for p in params)
    routes = {"torch_foreach": torch.optim.AdamW(params, **HYPER).step}
    tf, why_not = torch_fused_or_reason(params)
    if tf is not None:
        routes["torch_fused"] = tf.step
    fp32, param = P.FusedAdamW(params, **HYPER), P.FusedAdamW(params, state_dtype="param", **HYPER)
    routes["fused_fp32_state"] = fp32.step
    routes["fused_param_state"] = param.step
    routes["fused_fp32_state_clipped"] = lambda: fp32.step(max_grad_norm=MAX_NORM)
    routes["fused_param_state_clipped"] = lambda: param.step(max_grad_norm=MAX_NORM)
    ms = interleaved(routes, args.reps, args.warmup, stream)
    r = {k: summary(v) for k, v in ms.items()}
    for k, b in BYTES.items():
        r[k]["bytes_per_param"] = b
        r[k]["TB_per_s"] = round(n * b / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
    for new, old in (("fused_param_state", "fused_fp32_state"),
                     ("fused_param_state_clipped", "fused_fp32_state_clipped")):
        r[new]["vs_fp32_state"] = verdict(r[new]["median_ms"], r[old]["median_ms"])
        r[new]["speedup_vs_fp32_state"] = round(r[old]["median_ms"] / r[new]["median_ms"], 3)
    for other in ("torch_foreach", "torch_fused"):
        if other in r:
            r["fused_param_state"][f"vs_{other}"] = verdict(r["fused_param_state"]["median_ms"], r[other]["median_ms"])
            r["fused_param_state"][f"speedup_vs_{other}"] = round(
                r[other]["median_ms"] / r["fused_param_state"]["median_ms"], 3)
    unclipped = [k for k in r if not k.endswith("_clipped")]
    rec = {"shape": name, "n_params": n, "n_tensors": len(params), "param_dtype": "bfloat16", "routes": r,
           "fastest_unclipped": min(unclipped, key=lambda k: r[k]["median_ms"]),
           "fastest_clipped": min((k for k in r if k.endswith("_clipped")), key=lambda k: r[k]["median_ms"])}
    if why_not:
        rec["torch_fused_refused"] = why_not
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-parent-lib", default=None)
    ap.add_argument("--ab-rounds", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev)
    shapes = []
    w = with_grads([torch.nn.Parameter((0.02 * torch.randn(V, H, generator=gen, device=dev)).bfloat16())], gen)
    shapes.append(bench_shape("lm_head_bf16", w, args, stream))
    del w
    torch.cuda.empty_cache()
    vh = P.make_value_head(H, 1).to(dev)
    shapes.append(bench_shape("ppo_value_head", with_grads(list(vh.parameters()), gen), args, stream))
    del vh
    torch.cuda.empty_cache()
    rec = {"tool": "adamw_bf16_state_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hyper": {k: list(v) if isinstance(v, tuple) else v for k, v in HYPER.items()}, "max_norm": MAX_NORM,
           "reps": args.reps, "shapes": shapes}
    if args.ab_parent_lib:
        rec["unclipped_step_ab"] = ab_unclipped(args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
