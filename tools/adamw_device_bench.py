"""FusedAdamW's device-resident mode against the default mode, at the value-head shape and the
ILQL-heads shape of tools/adamw_bench.py, unclipped and clipped (max_grad_norm 1.0), three
routes interleaved in one process, timed with HIP events after warm-up (medians of --reps).
The three optimizers step the SAME parameters, gradients and moments (the capturable ones are
handed the first one's exp_avg / exp_avg_sq): at the 4.4 GB ILQL shape, copies of the tensors
at other addresses differ by several per cent in time on their own, more than the routes do.

  a  FusedAdamW.step()                             the default mode: scalars formed on the host
  b  FusedAdamW(capturable=True).step()            eager: + one trlx_adamw_advance launch per group
  c  one captured update of (b), graph.replay()    torch.cuda.graph, one stream, a linear chain

No speed-up is required of (b): it costs one more tiny launch than (a).  Each shape reports the
three medians, b/a and c/a, and the fastest.  If the capture fails, (c) is left out and the
reason recorded.

--ab-parent-lib FILE: route (a), unclipped, at the ILQL-heads shape with that build of the
library (the parent commit's) and with this tree's, in child processes run in alternation
(--ab-rounds each): the median of the new library's runs must lie inside the min-max spread of
the parent's own runs.  A difference inside 5 % is reported as "not faster".  One JSON line.
GPU-box tool:  python tools/adamw_device_bench.py [--reps N] [--ab-parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

NEW_ENTRIES = ("trlx_adamw_advance", "trlx_adamw_sched_scalars_host", "trlx_adamw_step_dev",
               "trlx_adamw_step_clipped_dev")
if os.environ.get("ADAMW_DEVICE_BENCH_OLD_LIB"):  # a child on the parent's library: it has no schedule entries
    import importlib.util
    _spec = importlib.util.spec_from_file_location("trlx_t5_amd._lib", os.path.join(__graft_entry__.PKG_DIR, "_lib.py"))
    _mod = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_mod)
    for _name in NEW_ENTRIES:
        _mod.SIGNATURES.pop(_name)
    sys.modules["trlx_t5_amd._lib"] = _mod

P = __graft_entry__.load_package()
from adamw_bench import H, V, HYPER, interleaved, summary, verdict, with_grads  # noqa: E402


def share_moments(opt, donor, params):
    for p in params:
        opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = donor.state[p]["exp_avg"], donor.state[p]["exp_avg_sq"]


def bench_shape(name, params, args, stream, max_grad_norm):
    n = sum(p.numel() for p in params)
    host = P.FusedAdamW(params, max_grad_norm=max_grad_norm, **HYPER)
    eager = P.FusedAdamW(params, max_grad_norm=max_grad_norm, capturable=True, **HYPER)
    captured = P.FusedAdamW(params, max_grad_norm=max_grad_norm, capturable=True, **HYPER)
    for opt in (host, eager):
        opt.step()
    share_moments(eager, host, params)
    routes = {"a_host_scalars": host.step, "b_capturable_eager": eager.step}
    rec = {"shape": name, "clipped": max_grad_norm is not None, "n_params": n, "n_tensors": len(params),
           "param_dtype": str(params[0].dtype).split(".")[-1]}
    captured.step()  # warm-up: every buffer exists before the capture
    share_moments(captured, host, params)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured.step()
        graph.replay()
        torch.cuda.synchronize()
        routes["c_graph_replay"] = graph.replay
    except RuntimeError as e:
        rec["c_graph_replay_left_out"] = f"{type(e).__name__}: {str(e)[:200]}"
    ms = interleaved(routes, args.reps, args.warmup, stream)
    r = rec["routes"] = {k: summary(v) for k, v in ms.items()}
    a = r["a_host_scalars"]["median_ms"]
    for k in ("b_capturable_eager", "c_graph_replay"):
        if k in r:
            r[k]["ratio_to_a"] = round(r[k]["median_ms"] / a, 3)
            r[k]["vs_a"] = verdict(r[k]["median_ms"], a)
    rec["fastest"] = min(r, key=lambda k: r[k]["median_ms"])
    return rec


def ilql_trainable(dev, gen):
    heads = P.ILQLHeads(P.ILQLConfig(), H, V).to(dev)
    return with_grads([p for p in heads.parameters() if p.requires_grad], gen)


def unclipped_only(args, dev, gen, stream):
    """Route (a), unclipped, alone at the ILQL-heads shape (the A/B child)."""
    ours = P.FusedAdamW(ilql_trainable(dev, gen), **HYPER)
    ms = interleaved({"a": ours.step}, args.reps, args.warmup, stream)
    print(json.dumps(summary(ms["a"])), flush=True)


def ab_unclipped(args):
    """Children in alternation, the order swapped every round (parent, new, new, parent, ...) so
    that a drift over the run falls on both alike."""
    runs = {"parent": [], "new": []}
    for k in range(args.ab_rounds):
        for which in (("parent", "new") if k % 2 == 0 else ("new", "parent")):
            env = dict(os.environ)
            if which == "parent":
                env["TRLX_T5_AMD_LIB"] = os.path.abspath(args.ab_parent_lib)
                env["ADAMW_DEVICE_BENCH_OLD_LIB"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--unclipped-only", "--reps", str(args.reps),
                                  "--warmup", str(args.warmup)], env=env, check=True, capture_output=True, text=True,
                                 timeout=300)
            runs[which].append(json.loads(out.stdout.strip().splitlines()[-1])["median_ms"])
    lo, hi = min(runs["parent"]), max(runs["parent"])
    new = round(statistics.median(runs["new"]), 4)  # the mean of the two middle runs of an even number
    return {"shape": "ilql_heads_c5", "route": "a_host_scalars, unclipped", "parent_medians_ms": runs["parent"],
            "new_medians_ms": runs["new"], "parent_min_ms": lo, "parent_max_ms": hi, "new_median_ms": new,
            "new_inside_parent_spread": lo <= new <= hi, "new_not_slower_than_parent_max": new <= hi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-parent-lib", default=None)
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--unclipped-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev)
    if args.unclipped_only:
        return unclipped_only(args, dev, gen, stream)
    shapes = []
    for clip in (None, 1.0):
        vh = P.make_value_head(H, 1).to(dev)
        shapes.append(bench_shape("ppo_value_head", with_grads(list(vh.parameters()), gen), args, stream, clip))
    for clip in (None, 1.0):
        shapes.append(bench_shape("ilql_heads_c5", ilql_trainable(dev, gen), args, stream, clip))
        torch.cuda.empty_cache()
    rec = {"tool": "adamw_device_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hyper": {k: list(v) if isinstance(v, tuple) else v for k, v in HYPER.items()}, "reps": args.reps,
           "shapes": shapes}
    del shapes
    torch.cuda.empty_cache()
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
