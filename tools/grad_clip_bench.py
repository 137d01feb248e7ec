"""The clipped optimizer step at the shapes of tools/adamw_bench.py, four routes on the same
parameters and gradients, interleaved in one process, timed with HIP events after warm-up
(medians of --reps):

  a  torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True) (foreach where this torch
     build refuses fused=True for the tensors)
  b  torch.nn.utils.clip_grad_norm_ + FusedAdamW.step()       the best route without the fold
  c  FusedAdamW.step(max_grad_norm=1.0)                        the fold
  d  FusedAdamW.step()                                         no clip

Byte model of c: the unclipped step (tools/adamw_bench.py: 28 B per fp32 parameter, 22 B per bf16
parameter, 28 B with a master) plus one more read of the gradients.  k_grad_sumsq alone
(trlx_grad_norm, record only) is timed too and its rate over the gradients' bytes reported: it is
a read-only stream with an fp64 multiply-add per element.

--ab-parent-lib FILE: route d at the ILQL-heads shape with that build of the library (the parent
commit's) and with this tree's, in child processes run in alternation (--ab-rounds each): the
new library's median must lie inside the min-max spread of the parent's own runs.
A difference inside 5 % is reported as "not faster".  One JSON line.
GPU-box tool:  python tools/grad_clip_bench.py [--reps N] [--ab-parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

NEW_ENTRIES = ("trlx_grad_norm_workspace_bytes", "trlx_grad_norm", "trlx_adamw_step_clipped", "trlx_adamw_step_ex")
if os.environ.get("GRAD_CLIP_BENCH_OLD_LIB"):  # a child on the parent's library: it may lack the newer entries
    import importlib.util
    _spec = importlib.util.spec_from_file_location("trlx_t5_amd._lib", os.path.join(__graft_entry__.PKG_DIR, "_lib.py"))
    _mod = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_mod)
    for _name in NEW_ENTRIES:
        _mod.SIGNATURES.pop(_name)
    sys.modules["trlx_t5_amd._lib"] = _mod

P = __graft_entry__.load_package()
from trlx_t5_amd import optim as O  # noqa: E402
from adamw_bench import H, V, HYPER, interleaved, summary, verdict, with_grads, torch_fused_or_reason  # noqa: E402

MAX_NORM = 1.0


def bench_shape(name, params, args, stream, master=False):
    n = sum(p.numel() for p in params)
    es = params[0].element_size()
    torch_opt, why_not = torch_fused_or_reason(params)
    if torch_opt is None:
        torch_opt = torch.optim.AdamW(params, **HYPER)
    ours = P.FusedAdamW(params, master_weights=master, **HYPER)
    grads = [p.grad for p in params]
    record = torch.zeros(O.RECORD_FLOATS, dtype=torch.float32, device=params[0].device)
    workspace = torch.empty(O._workspace_bytes(grads) // 8, dtype=torch.float64, device=params[0].device)

    def a():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        torch_opt.step()

    def b():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        ours.step()

    routes = {"a_torch_clip_torch_adamw": a, "b_torch_clip_fused_adamw": b,
              "c_fused_clipped_step": lambda: ours.step(max_grad_norm=MAX_NORM), "d_fused_step": ours.step,
              "sumsq_and_finish_only": lambda: O._grad_norm(grads, MAX_NORM, record, workspace, 0)}
    ms = interleaved(routes, args.reps, args.warmup, stream)
    r = {k: summary(v) for k, v in ms.items()}
    step_bytes = n * (28 if es == 4 or master else 22)
    g_bytes = sum(g.numel() * g.element_size() for g in grads)
    rec = {"shape": name, "n_params": n, "n_tensors": len(params), "param_dtype": str(params[0].dtype).split(".")[-1],
           "master": master, "torch_adamw": "fused" if why_not is None else "foreach", "routes": r,
           "bytes_per_param": {"d_fused_step": step_bytes / n, "c_fused_clipped_step": (step_bytes + g_bytes) / n,
                               "torch_clip_on_top": 3 * g_bytes / n}}
    for k, nbytes in (("c_fused_clipped_step", step_bytes + g_bytes), ("d_fused_step", step_bytes),
                      ("sumsq_and_finish_only", g_bytes)):
        r[k]["TB_per_s"] = round(nbytes / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
    c = r["c_fused_clipped_step"]["median_ms"]
    for other in ("a_torch_clip_torch_adamw", "b_torch_clip_fused_adamw"):
        r["c_fused_clipped_step"][f"vs_{other[0]}"] = verdict(c, r[other]["median_ms"])
        r["c_fused_clipped_step"][f"speedup_vs_{other[0]}"] = round(r[other]["median_ms"] / c, 3)
    rec["fastest_of_a_b_c"] = min(("a_torch_clip_torch_adamw", "b_torch_clip_fused_adamw", "c_fused_clipped_step"),
                                  key=lambda k: r[k]["median_ms"])
    r["c_fused_clipped_step"]["cost_of_the_clip_ms"] = round(c - r["d_fused_step"]["median_ms"], 4)
    if why_not:
        rec["torch_fused_refused"] = why_not
    return rec


def ilql_trainable(dev, gen):
    heads = P.ILQLHeads(P.ILQLConfig(), H, V).to(dev)
    return with_grads([p for p in heads.parameters() if p.requires_grad], gen)


def unclipped_only(args, dev, gen, stream):
    """Route d alone at the ILQL-heads shape (the A/B child)."""
    params = ilql_trainable(dev, gen)
    ours = P.FusedAdamW(params, **HYPER)
    ms = interleaved({"d_fused_step": ours.step}, args.reps, args.warmup, stream)
    print(json.dumps(summary(ms["d_fused_step"])), flush=True)


def ab_unclipped(args):
    """Children in alternation: parent's library, this tree's, parent's, ..."""
    runs = {"parent": [], "new": []}
    for _ in range(args.ab_rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            if which == "parent":
                env["TRLX_T5_AMD_LIB"] = os.path.abspath(args.ab_parent_lib)
                env["GRAD_CLIP_BENCH_OLD_LIB"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--unclipped-only", "--reps", str(args.reps),
                                  "--warmup", str(args.warmup)], env=env, check=True, capture_output=True, text=True,
                                 timeout=300)
            runs[which].append(json.loads(out.stdout.strip().splitlines()[-1])["median_ms"])
    lo, hi = min(runs["parent"]), max(runs["parent"])
    new = sorted(runs["new"])[len(runs["new"]) // 2]
    return {"shape": "ilql_heads_c5", "route": "d_fused_step", "parent_medians_ms": runs["parent"],
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
    trainable = ilql_trainable(dev, gen)
    shapes.append(bench_shape("ilql_heads_c5", trainable, args, stream))
    del trainable
    torch.cuda.empty_cache()
    for master in (False, True):
        w = with_grads([torch.nn.Parameter((0.02 * torch.randn(V, H, generator=gen, device=dev)).bfloat16())], gen)
        shapes.append(bench_shape("lm_head_bf16", w, args, stream, master=master))
        del w
        torch.cuda.empty_cache()
    for master in (False, True):
        vh = P.make_value_head(H, 1).to(dev)
        shapes.append(bench_shape("ppo_value_head", with_grads(list(vh.parameters()), gen), args, stream, master=master))
    rec = {"tool": "grad_clip_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hyper": {k: list(v) if isinstance(v, tuple) else v for k, v in HYPER.items()}, "max_norm": MAX_NORM,
           "reps": args.reps, "shapes": shapes}
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
