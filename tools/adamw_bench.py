"""The optimizer step at the shapes the library trains: torch.optim.AdamW (default = foreach),
torch.optim.AdamW(fused=True) where this torch build accepts it on the device, and FusedAdamW,
on the same parameters and gradients, interleaved in one process, timed with HIP events after
warm-up (medians of --reps); on a sync step FusedAdamW.step() + polyak_update against the
folded FusedAdamW.step(polyak=...).

  ilql_heads_c5      the trainable ILQL heads at C5 (H 768, V 50257, two Q heads + V head), fp32
  lm_head_bf16       the lm_head weight [50257, 768] in bf16, without and with an fp32 master
  ppo_value_head     make_value_head(768) in bf16 (without and with master)

Rates are over the byte model of one update: 28 B per fp32 parameter (read p, g, m, v; write
p, m, v), 36 B folded (+ read and write the target), 40 B unfolded (+ the sync's re-read of p);
bf16 parameters: 2 B for each of p, g (and target) accesses, 4 B for m, v and master.  torch's
routes keep bf16 states for bf16 parameters, so their byte count differs; only times are
compared there.  A difference inside 5 % is reported as "not faster".  One JSON line.
GPU-box tool:  python tools/adamw_bench.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from trlx_t5_amd.timing import make_event  # noqa: E402

H, V = 768, 50257
HYPER = dict(lr=1e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-6)


def timed(fn, stream):
    e0, e1 = make_event(), make_event()
    e0.record(stream)
    fn()
    e1.record(stream)
    return e0, e1


def interleaved(fns, reps, warmup, stream):
    """{name: [ms, ...]} of functions run in alternation (same clocks, same cache state)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            evs[k].append(timed(fn, stream))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "n": len(s)}


def verdict(new, old):
    return "faster" if new < 0.95 * old else "slower" if old < 0.95 * new else "not faster"


def torch_fused_or_reason(params):
    try:
        opt = torch.optim.AdamW(params, fused=True, **HYPER)
        opt.step()
        torch.cuda.synchronize()
        return opt, None
    except Exception as e:  # this torch build does not take fused=True for these tensors
        return None, f"{type(e).__name__}: {str(e)[:200]}"


def bench_shape(name, params, args, stream, master=False, sync=None):
    """params: leaf tensors with .grad set.  sync: (targets, sources, alpha) for the sync step."""
    n = sum(p.numel() for p in params)
    es = params[0].element_size()
    routes, opts = {}, {}
    opts["torch_foreach"] = torch.optim.AdamW(params, **HYPER)
    tf, why_not = torch_fused_or_reason(params)
    if tf is not None:
        opts["torch_fused"] = tf
    opts["fused_adamw"] = P.FusedAdamW(params, master_weights=master, **HYPER)
    for k, o in opts.items():
        routes[k] = o.step
    if sync is not None:
        targets, sources, alpha = sync
        ours = opts["fused_adamw"]

        def unfolded():
            ours.step()
            P.polyak_update(targets, sources, alpha)

        routes["fused_adamw_then_polyak"] = unfolded
        routes["fused_adamw_folded"] = lambda: ours.step(polyak=sync)
    ms = interleaved(routes, args.reps, args.warmup, stream)
    rec = {"shape": name, "n_params": n, "n_tensors": len(params), "param_dtype": str(params[0].dtype).split(".")[-1],
           "master": master, "routes": {k: summary(v) for k, v in ms.items()}}
    if why_not:
        rec["torch_fused_refused"] = why_not
    r = rec["routes"]
    # fp32: 4 reads + 3 writes of 4 B.  bf16: p, g read and p written at 2 B, m and v read and written at
    # 4 B (22 B); with a master p is only written and the master is read and written (28 B).
    step_bytes = n * (28 if es == 4 or master else 22)
    rec["bytes_per_param"] = {"fused_adamw": step_bytes / n}
    r["fused_adamw"]["TB_per_s"] = round(step_bytes / (r["fused_adamw"]["median_ms"] * 1e-3) / 1e12, 3)
    for other in ("torch_foreach", "torch_fused"):
        if other in r:
            r["fused_adamw"][f"vs_{other}"] = verdict(r["fused_adamw"]["median_ms"], r[other]["median_ms"])
            r["fused_adamw"][f"speedup_vs_{other}"] = round(r[other]["median_ms"] / r["fused_adamw"]["median_ms"], 3)
    if sync is not None:
        ns = sum(s.numel() for s in sync[1])
        folded, unfolded_b = step_bytes + 2 * es * ns, step_bytes + 3 * es * ns
        rec["bytes_per_param"].update(folded=folded / n, then_polyak=unfolded_b / n)
        r["fused_adamw_folded"]["TB_per_s"] = round(folded / (r["fused_adamw_folded"]["median_ms"] * 1e-3) / 1e12, 3)
        r["fused_adamw_then_polyak"]["TB_per_s"] = round(
            unfolded_b / (r["fused_adamw_then_polyak"]["median_ms"] * 1e-3) / 1e12, 3)
        r["fused_adamw_folded"]["vs_then_polyak"] = verdict(r["fused_adamw_folded"]["median_ms"],
                                                            r["fused_adamw_then_polyak"]["median_ms"])
        r["fused_adamw_folded"]["speedup_vs_then_polyak"] = round(
            r["fused_adamw_then_polyak"]["median_ms"] / r["fused_adamw_folded"]["median_ms"], 3)
    return rec


def with_grads(params, gen):
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen, device=p.device) * 1e-2).to(p.dtype)
    return params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev)
    shapes = []

    cfg = P.ILQLConfig()
    heads = P.ILQLHeads(cfg, H, V).to(dev)
    trainable = with_grads([p for p in heads.parameters() if p.requires_grad], gen)
    sync = ([p.data for h in heads.target_q_heads for p in h.parameters()],
            [p.data for h in heads.q_heads for p in h.parameters()], cfg.alpha)
    shapes.append(bench_shape("ilql_heads_c5", trainable, args, stream, sync=sync))
    del heads, trainable, sync
    torch.cuda.empty_cache()

    for master in (False, True):
        w = with_grads([torch.nn.Parameter((0.02 * torch.randn(V, H, generator=gen, device=dev)).bfloat16())], gen)
        shapes.append(bench_shape("lm_head_bf16", w, args, stream, master=master))
        del w
        torch.cuda.empty_cache()
    for master in (False, True):
        vh = P.make_value_head(H, 1).to(dev)
        shapes.append(bench_shape("ppo_value_head", with_grads(list(vh.parameters()), gen), args, stream,
                                  master=master))

    rec = {"tool": "adamw_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hyper": {k: list(v) if isinstance(v, tuple) else v for k, v in HYPER.items()},
           "reps": args.reps, "shapes": shapes}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
