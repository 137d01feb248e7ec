"""ILQL heads at the C5 shape (B 128, A 63, H 768, V 50257, fp32 heads): the target-Q part of
the step on the parent route (torch builds both full [B, A, V] target heads, then the loss)
against the new route (first Linear + ReLU in torch, trlx_ilql_tq_at_actions, then the loss on
the gathered values), and ILQLHeads.sync_target_q_heads() against the reference's per-tensor
expression.  Both pairs are timed interleaved in one process with HIP events after warm-up;
one JSON line is printed (medians and minima in ms).  A difference inside 5 % (the README's
box-to-box spread) is reported as "not faster".
GPU-box tool:  python tools/ilql_heads_bench.py [--reps N] [--out FILE]"""
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

B, L, H, V = 128, 64, 768, 50257
A = L - 1
HBM_PEAK = 8.0e12  # bytes / s (spec)


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
    return "faster" if new < 0.95 * old else "not faster"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = P.ILQLConfig()
    heads = P.ILQLHeads(cfg, H, V).to(dev)
    with torch.no_grad():
        for p in heads.target_q_heads.parameters():
            p.add_(0.01 * torch.randn_like(p))
    g = torch.Generator(device=dev).manual_seed(1)
    hs = torch.randn(B, L, H, generator=g, device=dev)
    ids = torch.randint(0, V, (B, L), generator=g, device=dev)
    six, aix = torch.arange(L, device=dev).repeat(B, 1), torch.arange(A, device=dev).repeat(B, 1)
    dones = torch.ones(B, L, dtype=torch.long, device=dev)
    dones[:, -1] = 0
    batch = P.ILQLBatch(ids, torch.ones(B, L, dtype=torch.long, device=dev),
                        torch.randn(B, A, generator=g, device=dev), six, aix, dones)
    logits = torch.randn(B, L, V, generator=g, device=dev)
    with torch.no_grad():
        a_hs = hs[torch.arange(B, device=dev)[:, None], aix]
        qs = [h(a_hs) for h in heads.q_heads]
        vs = heads.v_head(hs).reshape(B, L).contiguous()
    hp = P.ILQLHotPath(cfg, B, L, V, torch.float32, dev)
    stream = torch.cuda.current_stream(dev)
    w2 = [h[2].weight for h in heads.target_q_heads]
    b2 = [h[2].bias for h in heads.target_q_heads]
    keep = {}

    def first_layers():
        with torch.no_grad():
            return [h[1](h[0](a_hs)) for h in heads.target_q_heads]

    def parent_route():  # full [B, A, V] target heads, then the loss gathers them at a*
        with torch.no_grad():
            tq = [h(a_hs) for h in heads.target_q_heads]
        keep["parent"] = hp.step(logits, qs, tq, vs, batch)[0].clone()

    def new_route():  # the target heads at a* only, then the loss on the gathered values
        tq = P.ilql_target_q_at_actions(first_layers(), w2, b2, ids, aix)
        keep["new"] = hp.step(logits, qs, tq, vs, batch)[0].clone()

    zs = first_layers()

    def loss_only():
        hp.step(logits, qs, keep["tq_at"], vs, batch)

    def dot_only():
        keep["tq_at"] = P.ilql_target_q_at_actions(zs, w2, b2, ids, aix)

    dot_only()
    route = interleaved({"parent": parent_route, "new": new_route, "loss_only": loss_only, "dot_kernel": dot_only},
                        args.reps, args.warmup, stream)
    same = bool(torch.allclose(keep["parent"], keep["new"], rtol=1e-5, atol=1e-6))

    alpha = cfg.alpha

    def sync_fused():
        heads.sync_target_q_heads()

    def sync_per_tensor():  # ilql_models.py:161-168
        with torch.no_grad():
            for th, qh in zip(heads.target_q_heads, heads.q_heads):
                for tp, cp in zip(th.parameters(), qh.parameters()):
                    tp.data.copy_((alpha * cp.data) + (1.0 - alpha) * tp.data)

    sync = interleaved({"fused": sync_fused, "per_tensor": sync_per_tensor}, args.reps, args.warmup, stream)

    N, K, es = B * A, 2 * H, 4
    dot_bytes = 2 * (2 * N * K * es + N * (es + 4)) + 8 * (B * L + N)  # z + W2 rows + bias + out per head, ids
    n_params = sum(p.numel() for h in heads.target_q_heads for p in h.parameters())
    rec = {
        "tool": "ilql_heads_bench", "shape": {"B": B, "A": A, "L": L, "H": H, "V": V, "dtype": "float32", "nq": 2},
        "device": torch.cuda.get_device_name(0),
        "target_q_step": {k: summary(v) for k, v in route.items()},
        "sync_target_q_heads": {k: summary(v) for k, v in sync.items()},
        "losses_agree": same,
    }
    r, s = rec["target_q_step"], rec["sync_target_q_heads"]
    r["new_vs_parent"] = verdict(r["new"]["median_ms"], r["parent"]["median_ms"])
    r["speedup"] = round(r["parent"]["median_ms"] / r["new"]["median_ms"], 3)
    s["fused_vs_per_tensor"] = verdict(s["fused"]["median_ms"], s["per_tensor"]["median_ms"])
    s["speedup"] = round(s["per_tensor"]["median_ms"] / s["fused"]["median_ms"], 3)
    dot_s = r["dot_kernel"]["median_ms"] * 1e-3
    rec["dot_kernel"] = {"bytes": dot_bytes, "TB_per_s": round(dot_bytes / dot_s / 1e12, 3),
                         "share_of_8TB_per_s": round(dot_bytes / dot_s / HBM_PEAK, 4)}
    sync_bytes = 3 * n_params * es  # read source, read + write target
    rec["sync_kernel"] = {"bytes": sync_bytes,
                          "TB_per_s": round(sync_bytes / (s["fused"]["median_ms"] * 1e-3) / 1e12, 3)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
