"""T5's full-sequence attention, three routes, at the rollout's shapes.

  eager   HF's eager op sequence: matmul, the materialised [1, nH, Tq, S] bias plus the additive
          finfo.min mask (both precomputed, as HF reuses position_bias across layers), fp32 softmax
          cast back, matmul, transpose to [B, Tq, nH*d]
  sdpa    F.scaled_dot_product_attention with bias plus additive mask as attn_mask and scale=1.0
  fused   t5_attention (trlx_t5_attention, one launch, no [Tq, S] tensor)

The routes run interleaved in one process on the same tensors, their order shuffled per
repetition, timed with HIP events after warm-up; medians of --reps (default 20).  A difference
inside 5 % is reported as "tie".  FLOPs: 4·nH·d·sum_b Tq·S_live(b) (causal: the keys j <= i).
Byte model of the fused call: q and out once, K and V once per query block of Q_TILE rows (live
keys only), the mask row once per workgroup, the bias window per tile.  One JSON record is printed
and written to --out.
GPU-box tool:  python tools/t5_attention_bench.py [--reps N] [--out FILE] [--only NAME]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from trlx_t5_amd.timing import make_event  # noqa: E402

QT, KT = P.t5_attention.Q_TILE, P.t5_attention.KV_TILE
# name -> (mode, B, nH, d_kv, Tq, S, left-padded)
SHAPES = {
    "t5base_enc_B64_S512": ("encoder", 64, 12, 64, 512, 512, False),
    "t5base_enc_B64_S512_leftpad": ("encoder", 64, 12, 64, 512, 512, True),
    "t5base_enc_B256_S512": ("encoder", 256, 12, 64, 512, 512, False),
    "t5base_enc_B256_S512_leftpad": ("encoder", 256, 12, 64, 512, 512, True),
    "t5base_dec_causal_B256_T48": ("decoder", 256, 12, 64, 48, 48, False),
    "t5base_cross_B256_48x512": ("cross", 256, 12, 64, 48, 512, False),
    "t5base_cross_B256_48x512_leftpad": ("cross", 256, 12, 64, 48, 512, True),
    "nH32_d128_enc_B32_S512": ("encoder", 32, 32, 128, 512, 512, False),
    "nH32_d128_enc_B32_S512_leftpad": ("encoder", 32, 32, 128, 512, 512, True),
}


def interleaved(fns, reps, warmup, stream, rng):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(reps):
        order = list(fns)
        rng.shuffle(order)
        for k in order:
            e0, e1 = make_event(), make_event()
            e0.record(stream)
            fns[k]()
            e1.record(stream)
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in evs.items()}


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "n": len(s)}


def fastest(ms):
    order = sorted(ms, key=lambda k: ms[k]["median_ms"])
    if ms[order[0]]["median_ms"] >= 0.95 * ms[order[1]]["median_ms"]:
        return "tie: " + " / ".join(sorted(order[:2]))
    return order[0]


def bench(mode, B, nH, d, Tq, S, padded, dev, reps, warmup, stream, rng):
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(Tq * 1000 + S + B)
    s = d ** -0.25
    q = (torch.randn(B, Tq, nH * d, generator=g, device=dev) * s).to(dtype)      # the projections' outputs
    k = (torch.randn(B, S, nH * d, generator=g, device=dev) * s).to(dtype)
    v = torch.randn(B, S, nH * d, generator=g, device=dev).to(dtype)
    weight = torch.randn(32, nH, generator=g, device=dev)
    causal = mode == "decoder"
    table = None if mode == "cross" else P.t5_relative_bias_offsets(weight, Tq, S, mode == "encoder")
    mask = None
    live = torch.full((B,), S, dtype=torch.long, device=dev)
    if padded:
        live = torch.randint(S // 4, S + 1, (B,), generator=g, device=dev)              # U{128..512} live keys
        mask = (torch.arange(S, device=dev)[None, :] >= (S - live)[:, None]).long()
    rel = torch.arange(S, device=dev)[None, :] - torch.arange(Tq, device=dev)[:, None]
    add = torch.zeros(1, 1, Tq, S, dtype=dtype, device=dev)
    if table is not None:
        add = add + table[:, rel + (Tq - 1)].to(dtype)[None]
    if mask is not None:
        add = add + torch.zeros(B, 1, 1, S, dtype=dtype, device=dev).masked_fill((mask == 0)[:, None, None, :],
                                                                                 torch.finfo(dtype).min)
    if causal:
        add = add + torch.zeros(Tq, S, dtype=dtype, device=dev).masked_fill(rel > 0, torch.finfo(dtype).min)[None, None]
    add = add.contiguous()
    q4, k4, v4 = (x.view(B, -1, nH, d).transpose(1, 2) for x in (q, k, v))             # HF's [B, nH, T, d] views
    keep = {}

    def eager():
        scores = torch.matmul(q4, k4.transpose(3, 2))
        scores = scores + add
        w = torch.softmax(scores.float(), dim=-1).type_as(scores)
        keep["eager"] = torch.matmul(w, v4).transpose(1, 2).reshape(B, Tq, nH * d)

    def sdpa():
        keep["sdpa"] = F.scaled_dot_product_attention(q4, k4, v4, attn_mask=add, scale=1.0) \
            .transpose(1, 2).reshape(B, Tq, nH * d)

    def fused():
        keep["fused"] = P.t5_attention(q, k, v, bias=table, key_mask=mask, causal=causal, n_heads=nH)

    with torch.no_grad():
        ms = {n: summary(t) for n, t in interleaved({"eager": eager, "sdpa": sdpa, "fused": fused}, reps, warmup,
                                                    stream, rng).items()}
    pairs = Tq * (Tq + 1) // 2 * B if causal else int(live.sum()) * Tq
    flop = 4 * nH * d * pairs
    nqb = (Tq + QT - 1) // QT
    kv_live = int(live.sum()) if not causal else sum(min(S, (b + 1) * QT) for b in range(nqb)) * B // nqb
    model = 2 * B * Tq * nH * d * 2 + 2 * kv_live * nqb * nH * d * 2 \
        + (B * S * 8 * nH * nqb if mask is not None else 0) \
        + (0 if table is None else B * nH * nqb * ((S + KT - 1) // KT) * (QT + KT) * 4)
    rec = {"mode": mode, "B": B, "nH": nH, "d_kv": d, "Tq": Tq, "S": S, "left_padded": padded,
           "live_keys_mean": round(float(live.float().mean()), 1), "workgroups": B * nH * nqb, **ms,
           "fastest": fastest(ms), "flop": flop, "fused_bytes_model": model}
    for n in ms:
        rec[f"{n}_TFLOP_per_s"] = round(flop / (ms[n]["median_ms"] * 1e-3) / 1e12, 1)
    rec["fused_GB_per_s_over_model"] = round(model / (ms["fused"]["median_ms"] * 1e-3) / 1e9, 1)
    f = keep["fused"].float()
    rec["max_abs_diff_fused_vs_eager"] = float((f - keep["eager"].float()).abs().max())
    rec["max_abs_diff_fused_vs_sdpa"] = float((f - keep["sdpa"].float()).abs().max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape's name")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = random.Random(0)
    print(f"t5_attention tiles: Q_TILE {QT}, KV_TILE {KT}", file=sys.stderr, flush=True)
    rec = {"tool": "t5_attention_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "dtype": "bf16",
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "Q_TILE": QT, "KV_TILE": KT,
           "shapes": {}}
    for name, shape in SHAPES.items():
        if args.only and name != args.only:
            continue
        rec["shapes"][name] = bench(*shape, dev, args.reps, args.warmup, stream, rng)
        torch.cuda.empty_cache()
        print(name, "done", file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
