"""The decode cross-attention over bf16 and over fp8 encoder keys / values, and the quantiser, at the
cross shapes of tools/t5_decode_attn_bench.py (T5-base B 256 and B 8, nH 32 d_kv 128 B 128; S 512,
plain and padded).

  bf16       t5_decode_cross_attention (trlx_t5_decode_attn)
  kv8        t5_decode_cross_attention_kv8 (trlx_t5_decode_attn_kv8) on the quantised tensors
  quantise   t5_quantize_cross_kv (trlx_t5_cross_kv_quantize): once per rollout and layer

The three run interleaved in one process on the same tensors, their order shuffled per repetition,
each call between two HIP events after warm-up; medians of --reps (default 20) with min and max.
Byte models (live = the unmasked keys): bf16 2·live·nH·d·2 + q + out (+ the mask); kv8 2·live·nH·d·1
+ the two scales + q + out (+ the mask); quantise 2·live·nH·d·2 read + 2·B·S·nH·d written + scales
(+ the mask, twice: two passes; the second pass over K and V is counted as a cache hit, not as bytes).
No ratio is assumed: the bytes bound the gain of kv8 at 2x, and a launch-bound shape shows none.

--parity-out FILE: accuracy, measured and not toleranced.  Per test case (tests/t5_decode_attn_checks
cross_case) the largest |error| of the kv8 route and of the bf16 kernel against the float64 oracle on
the ORIGINAL bf16 keys and values, and of the kv8 route against the oracle on its dequantised values.

    python tools/t5_cross_kv8_bench.py [--reps N] [--out FILE] [--parity-out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()

MODELS = [("t5base_B256", 256, 12, 64), ("t5base_B8", 8, 12, 64), ("nH32_d128_B128", 128, 32, 128)]
S = 512


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def bench_shape(B, nH, d, padded, dev, reps, warmup, rng):
    g = torch.Generator(device=dev).manual_seed(S + B)
    s = d ** -0.25
    q = (torch.randn(B, 1, nH * d, generator=g, device=dev) * s).to(torch.bfloat16)
    K = (torch.randn(B, nH, S, d, generator=g, device=dev) * s).to(torch.bfloat16)
    V = torch.randn(B, nH, S, d, generator=g, device=dev).to(torch.bfloat16)
    mask, live = None, B * S
    if padded:
        lengths = torch.randint(S // 4, S + 1, (B,), generator=g, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] < lengths[:, None]).long()
        live = int(mask.sum())
    kv8 = P.t5_quantize_cross_kv(K, V, mask)
    keep = {}
    fns = {"bf16": lambda: keep.__setitem__("bf16", P.t5_decode_cross_attention(q, K, V, mask)),
           "kv8": lambda: keep.__setitem__("kv8", P.t5_decode_cross_attention_kv8(q, kv8, mask)),
           "quantise": lambda: P.t5_quantize_cross_kv(K, V, mask, out=kv8)}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        evs = {k: [] for k in fns}
        order = list(fns)
        for _ in range(reps):
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[k]()
                e1.record()
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1000.0 for a, b in v] for k, v in evs.items()}
    small = 2 * B * nH * d * 2 + (B * S * 8 if padded else 0)             # q, out, the mask
    model = {"bf16": 2 * live * nH * d * 2 + small,
             "kv8": 2 * live * nH * d + 2 * B * nH * 4 + small,
             "quantise": 2 * live * nH * d * 2 + 2 * B * S * nH * d + 2 * B * nH * 4 + (2 * B * S * 8 if padded else 0)}
    rec = {"B": B, "nH": nH, "d_kv": d, "S": S, "padded": padded, "live_keys": live, "workgroups": B * nH}
    for k in fns:
        rec[k] = {**stats(us[k]), "bytes_model": model[k],
                  "TB_per_s_over_model": round(model[k] / (statistics.median(us[k]) * 1e-6) / 1e12, 3)}
    rec["bf16_over_kv8"] = round(rec["bf16"]["median_us"] / rec["kv8"]["median_us"], 3)
    rec["kv8_faster"] = rec["kv8"]["median_us"] < rec["bf16"]["median_us"]
    rec["max_abs_diff_kv8_vs_bf16"] = float((keep["kv8"].float() - keep["bf16"].float()).abs().max())
    return rec


def parity(dev):
    import t5_decode_attn_checks as A

    cases = {}
    worst = {"kv8": 0.0, "bf16": 0.0}
    for d in (64, 128):
        for Sx in A.CROSS_S:
            for kind in A.MASKS:
                c = A.cross_case(torch.bfloat16, d, Sx, kind)
                q, K, V, m = (None if x is None else x.to(dev) for x in (c["q"], c["K"], c["V"], c["mask"]))
                kv8 = P.t5_quantize_cross_kv(K, V, m)
                ref = A.oracle_cross(c["q"], c["K"], c["V"], c["mask"])
                Kd, Vd = kv8.dequantize()
                ref_deq = A.oracle_cross(c["q"], Kd.cpu(), Vd.cpu(), c["mask"])
                out8 = P.t5_decode_cross_attention_kv8(q, kv8, m)
                out16 = P.t5_decode_cross_attention(q, K, V, m)
                e = {"kv8_vs_oracle_on_original": A.max_err(out8, ref), "bf16_kernel_vs_oracle_on_original": A.max_err(out16, ref),
                     "kv8_vs_oracle_on_dequantised": A.max_err(out8, ref_deq), "max_abs_oracle": float(ref.abs().max())}
                cases[f"d{d}_S{Sx}_{kind}"] = e
                worst["kv8"] = max(worst["kv8"], e["kv8_vs_oracle_on_original"])
                worst["bf16"] = max(worst["bf16"], e["bf16_kernel_vs_oracle_on_original"])
    return {"tool": "tools/t5_cross_kv8_bench.py --parity-out", "device": torch.cuda.get_device_name(0),
            "what": "max |out - float64 oracle| per case (B 3, nH 5, bf16 inputs of tests/t5_decode_attn_checks.cross_case); "
                    "measured, not a tolerance", "worst_kv8_vs_oracle_on_original": worst["kv8"],
            "worst_bf16_kernel_vs_oracle_on_original": worst["bf16"], "cases": cases}


def dump(obj, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(obj, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_cross_kv8_bench.json"))
    ap.add_argument("--parity-out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = random.Random(8)
    rec = {"tool": "tools/t5_cross_kv8_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "HIP events around single calls, bf16 / kv8 / quantise interleaved, order shuffled per repetition",
           "shapes": {}}
    for name, B, nH, d in MODELS:
        for padded in (False, True):
            key = f"{name}_cross_S{S}" + ("_padded" if padded else "")
            rec["shapes"][key] = bench_shape(B, nH, d, padded, dev, args.reps, args.warmup, rng)
            print(key, json.dumps(rec["shapes"][key]), flush=True)
    dump(rec, args.out)
    if args.parity_out:
        par = parity(dev)
        print("parity", json.dumps({k: v for k, v in par.items() if k != "cases"}), flush=True)
        dump(par, args.parity_out)


if __name__ == "__main__":
    main()
