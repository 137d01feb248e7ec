"""The bf16 value head, fused route against the torch route, at the decode and training shapes.

  torch   the reference's three modules (Linear, ReLU, Linear, all bf16) and their autograd
  fused   ValueHead.values (trlx_value_head_fwd) and its backward (trlx_value_head_bwd + the two
          torch.matmul GEMMs)

Both routes run interleaved in one process on the same parameters and inputs, timed with HIP
events after warm-up; medians of --reps (default 20).  A difference inside 5 % is reported as
"tie".  One JSON record is printed and written to --out.
GPU-box tool:  python tools/value_head_bench.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from trlx_t5_amd.timing import make_event  # noqa: E402

# (name, N, H, with backward)
SHAPES = [("decode_B128_H768", 128, 768, False), ("C2_N6144_H768", 6144, 768, True),
          ("C3shard_N12288_H768", 12288, 768, True), ("N6144_H1024", 6144, 1024, True)]


def interleaved(fns, reps, warmup, stream):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = make_event(), make_event()
            e0.record(stream)
            fn()
            e1.record(stream)
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "n": len(s)}


def faster(fused, torch_ms):
    if fused < 0.95 * torch_ms:
        return "fused"
    return "torch" if torch_ms < 0.95 * fused else "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rec = {"tool": "value_head_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "shapes": {}}
    for name, N, H, with_bwd in SHAPES:
        torch.manual_seed(0)
        head = P.ValueHead(H).to(dev)
        ref = nn.Sequential(nn.Linear(H, 2 * H).bfloat16(), nn.ReLU().bfloat16(), nn.Linear(2 * H, 1).bfloat16()).to(dev)
        ref.load_state_dict(head.state_dict(), strict=True)
        g = torch.Generator(device=dev).manual_seed(1)
        h = torch.randn(N, H, generator=g, device=dev).to(torch.bfloat16)
        dv = torch.randn(N, generator=g, device=dev).to(torch.bfloat16)
        hg = h.clone().requires_grad_(True)
        keep = {}

        def fwd_torch():
            with torch.no_grad():
                keep["t"] = ref(h).squeeze(-1)

        def fwd_fused():
            with torch.no_grad():
                keep["f"] = head.values(h, torch.bfloat16)

        def step_torch():
            hg.grad = None
            ref.zero_grad(set_to_none=True)
            ref(hg).squeeze(-1).backward(dv)

        def step_fused():
            hg.grad = None
            head.zero_grad(set_to_none=True)
            head.values(hg, torch.bfloat16).backward(dv)

        fns = {"fwd_torch": fwd_torch, "fwd_fused": fwd_fused}
        if with_bwd:
            fns.update(fwd_bwd_torch=step_torch, fwd_bwd_fused=step_fused)
        ms = {k: summary(v) for k, v in interleaved(fns, args.reps, args.warmup, stream).items()}
        diff = float((keep["t"].float() - keep["f"].float()).abs().max())
        S = P.value_head_splits(N, H)
        # the forward kernel's own traffic and work: h once per column slice, W1 / b1 / w2 once per
        # token block, the partials out and back, the values
        ntb = -(-N // 64)
        fwd_bytes = S * N * H * 2 + ntb * (2 * H * H * 2 + 2 * 2 * H * 2) + (2 * S * N * 4 if S > 1 else 0) + N * 2
        fwd_flops = 2 * N * 2 * H * H + 2 * N * 2 * H
        r = {"N": N, "H": H, "splits": S, **ms, "max_abs_diff_between_routes": diff,
             "fwd_faster": faster(ms["fwd_fused"]["median_ms"], ms["fwd_torch"]["median_ms"]),
             "fwd_kernel": {"bytes_requested": fwd_bytes, "unique_bytes": N * H * 2 + 2 * H * H * 2 + N * 2,
                            "flops": fwd_flops,
                            "TFLOP_per_s": round(fwd_flops / (ms["fwd_fused"]["median_ms"] * 1e-3) / 1e12, 2)},
             "torch_activation_bytes_each_way": N * 2 * H * 2}
        if with_bwd:
            r["fwd_bwd_faster"] = faster(ms["fwd_bwd_fused"]["median_ms"], ms["fwd_bwd_torch"]["median_ms"])
        rec["shapes"][name] = r
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
