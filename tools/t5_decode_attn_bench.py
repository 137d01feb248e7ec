"""One T5 decode-step attention, three routes, at the rollout's shapes.

  eager   HF's eager op sequence on a preallocated cache: index copy of k_new / v_new, matmul,
          compute_bias (arange, bucket formula, embedding lookup, permute) or the additive mask,
          fp32 softmax cast back, matmul
  sdpa    the index copy, then F.scaled_dot_product_attention with the (precomputed) bias row or
          the additive mask as attn_mask and scale=1.0
  fused   t5_decode_self_attention / t5_decode_cross_attention (trlx_t5_decode_attn, one launch)

The routes run interleaved in one process on the same tensors, timed with HIP events after
warm-up; medians of --reps (default 20).  A difference inside 5 % is reported as "tie".  Byte
model of the fused call: 2·B·nH·kv_len·d_kv·sizeof(T) read (kv_len the live keys), plus q, the
appended k_new / v_new (read and written) and the output.  One JSON record is printed and written
to --out.
GPU-box tool:  python tools/t5_decode_attn_bench.py [--reps N] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from trlx_t5_amd.timing import make_event  # noqa: E402

# (name, B, nH, d_kv): T5-base decode at the C3 shard, its low-occupancy case, a wide-head model
MODELS = [("t5base_B256", 256, 12, 64), ("t5base_B8", 8, 12, 64), ("nH32_d128_B128", 128, 32, 128)]
SELF_T = (0, 24, 47)
MAX_LEN = 48
CROSS_S = 512
NUM_BUCKETS, MAX_DISTANCE = 32, 128


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


def fastest(ms):
    order = sorted(ms, key=lambda k: ms[k]["median_ms"])
    if ms[order[0]]["median_ms"] >= 0.95 * ms[order[1]]["median_ms"]:
        return "tie: " + " / ".join(sorted(order[:2]))
    return order[0]


def hf_bias(weight, t):
    """compute_bias of HF's decoder for the query at t over keys 0..t: [1, nH, 1, t + 1]."""
    context = torch.arange(1, dtype=torch.long, device=weight.device)[:, None] + t
    memory = torch.arange(t + 1, dtype=torch.long, device=weight.device)[None, :]
    rel = -torch.min(memory - context, torch.zeros(1, t + 1, dtype=torch.long, device=weight.device))
    max_exact = NUM_BUCKETS // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(MAX_DISTANCE / max_exact)
                         * (NUM_BUCKETS - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, NUM_BUCKETS - 1))
    buckets = torch.where(rel < max_exact, rel, large)
    return F.embedding(buckets, weight).permute([2, 0, 1]).unsqueeze(0)


def bench_self(B, nH, d, t, dtype, dev, reps, warmup, stream):
    g = torch.Generator(device=dev).manual_seed(t)
    s = d ** -0.25
    q, kn, vn = ((torch.randn(B, 1, nH * d, generator=g, device=dev) * f).to(dtype) for f in (s, s, 1.0))
    cache = P.T5DecodeKVCache(B, nH, d, MAX_LEN, dtype, dev)
    cache.k.copy_((torch.randn(cache.k.shape, generator=g, device=dev) * s).to(dtype))
    cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev).to(dtype))
    weight = torch.randn(NUM_BUCKETS, nH, generator=g, device=dev).to(dtype)
    table = P.t5_relative_bias_table(weight, MAX_LEN)
    bias_row = hf_bias(weight, t).contiguous()
    keep = {}
    q4, k4, v4 = (x.view(B, 1, nH, d).transpose(1, 2) for x in (q, kn, vn))    # HF's [B, nH, 1, d] views

    def append():
        cache.k[:, :, t:t + 1] = k4
        cache.v[:, :, t:t + 1] = v4
        return cache.k[:, :, :t + 1], cache.v[:, :, :t + 1]

    def eager():
        K, V = append()
        scores = torch.matmul(q4, K.transpose(2, 3)) + hf_bias(weight, t)
        w = torch.softmax(scores.float(), dim=-1).type_as(scores)
        keep["eager"] = torch.matmul(w, V).transpose(1, 2).reshape(B, nH * d)

    def sdpa():
        K, V = append()
        keep["sdpa"] = F.scaled_dot_product_attention(q4, K, V, attn_mask=bias_row, scale=1.0) \
            .transpose(1, 2).reshape(B, nH * d)

    def fused():
        keep["fused"] = P.t5_decode_self_attention(q, kn, vn, cache, t, table)

    with torch.no_grad():
        ms = {k: summary(v) for k, v in interleaved({"eager": eager, "sdpa": sdpa, "fused": fused}, reps, warmup,
                                                    stream).items()}
    es = q.element_size()
    model = 2 * B * nH * t * d * es + 3 * B * nH * d * es + 2 * B * nH * d * es + B * nH * d * es + nH * (t + 1) * 4
    return ms, model, keep


def bench_cross(B, nH, d, S, padded, dtype, dev, reps, warmup, stream):
    g = torch.Generator(device=dev).manual_seed(S)
    s = d ** -0.25
    q = (torch.randn(B, 1, nH * d, generator=g, device=dev) * s).to(dtype)
    K = (torch.randn(B, nH, S, d, generator=g, device=dev) * s).to(dtype)
    V = torch.randn(B, nH, S, d, generator=g, device=dev).to(dtype)
    mask, add = None, None
    live = B * S
    if padded:
        lengths = torch.randint(S // 4, S + 1, (B,), generator=g, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] < lengths[:, None]).long()
        add = torch.zeros(B, 1, 1, S, dtype=dtype, device=dev).masked_fill((mask == 0)[:, None, None, :],
                                                                          torch.finfo(dtype).min)
        live = int(mask.sum())
    keep = {}
    q4 = q.view(B, 1, nH, d).transpose(1, 2)

    def eager():
        scores = torch.matmul(q4, K.transpose(2, 3))
        if add is not None:
            scores = scores + add
        w = torch.softmax(scores.float(), dim=-1).type_as(scores)
        keep["eager"] = torch.matmul(w, V).transpose(1, 2).reshape(B, nH * d)

    def sdpa():
        keep["sdpa"] = F.scaled_dot_product_attention(q4, K, V, attn_mask=add, scale=1.0) \
            .transpose(1, 2).reshape(B, nH * d)

    def fused():
        keep["fused"] = P.t5_decode_cross_attention(q, K, V, mask)

    with torch.no_grad():
        ms = {k: summary(v) for k, v in interleaved({"eager": eager, "sdpa": sdpa, "fused": fused}, reps, warmup,
                                                    stream).items()}
    es = q.element_size()
    model = 2 * live * nH * d * es + 2 * B * nH * d * es + (B * S * 8 if padded else 0)
    return ms, model, keep


def record(ms, model, keep, **tags):
    f = keep["fused"].float()
    return {**tags, **ms, "fastest": fastest(ms), "fused_bytes_model": model,
            "fused_GB_per_s_over_model": round(model / (ms["fused"]["median_ms"] * 1e-3) / 1e9, 1),
            "max_abs_diff_fused_vs_eager": float((f - keep["eager"].float()).abs().max()),
            "max_abs_diff_fused_vs_sdpa": float((f - keep["sdpa"].float()).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    dtype = torch.bfloat16
    rec = {"tool": "t5_decode_attn_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "dtype": "bf16", "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": {}}
    for name, B, nH, d in MODELS:
        for t in SELF_T:
            ms, model, keep = bench_self(B, nH, d, t, dtype, dev, args.reps, args.warmup, stream)
            rec["shapes"][f"{name}_self_t{t}"] = record(ms, model, keep, B=B, nH=nH, d_kv=d, t=t, workgroups=B * nH)
        for padded in (False, True):
            ms, model, keep = bench_cross(B, nH, d, CROSS_S, padded, dtype, dev, args.reps, args.warmup, stream)
            rec["shapes"][f"{name}_cross_S{CROSS_S}" + ("_padded" if padded else "")] = record(
                ms, model, keep, B=B, nH=nH, d_kv=d, S=CROSS_S, padded=padded, workgroups=B * nH)
        print(name, "done", file=sys.stderr, flush=True)
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
