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

--set d256: the UL2 head (nH 16, d_kv 256, S 512) at B 128 and B 8, plain and padded: bf16, the kv8
call (k_t5_decode_attn_kv8_d256) at splits 1 / 2 / 4 / 8 and the quantiser, all interleaved.  A route
is called faster than another only where its whole min-max spread lies below the other's median
(slower: above it), else "tie"; the shapes where fp8 or a split loses are listed.  The parity file is
then the d_kv 256 one: the test cases of tests/test_gpu_t5_cross_kv8_d256.py at splits 1 / 2 / 3 with
the worst error / bound of the test's rule, and the quantisation's cost against the original keys.

--parent-lib PATH: the entries that existed before (trlx_t5_decode_attn_kv8 and
trlx_t5_cross_kv_quantize at nH 32, d_kv 128, B 128, S 512 padded) with that build of the library and
with this tree's, in alternating child processes, four each; this tree's median has to lie inside
the parent's own spread.

    python tools/t5_cross_kv8_bench.py [--set base|d256] [--reps N] [--out FILE] [--parity-out FILE]
                                       [--parent-lib other/libtrlx_t5_amd.so]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()

MODELS = [("t5base_B256", 256, 12, 64), ("t5base_B8", 8, 12, 64), ("nH32_d128_B128", 128, 32, 128)]
MODELS_D256 = [("ul2_B128", 128, 16, 256), ("ul2_B8", 8, 16, 256)]
D256_SPLITS = (1, 2, 4, 8)
S = 512


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def verdict(a, b):
    """a against b: faster / slower only where a's whole spread lies on one side of b's median."""
    if a["max_us"] < b["median_us"]:
        return "faster"
    return "slower" if a["min_us"] > b["median_us"] else "tie"


def bench_shape(B, nH, d, padded, dev, reps, warmup, rng, splits=()):
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
    if splits:   # the d_kv 256 call: one route per number of key ranges
        del fns["kv8"]
        for x in splits:
            fns[f"kv8_s{x}"] = lambda x=x: keep.__setitem__(f"kv8_s{x}", P.t5_decode_cross_attention_kv8(q, kv8, mask, splits=x))
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
             # a split adds its fp32 states, written once and read once
             **{f"kv8_s{x}": 2 * live * nH * d + 2 * B * nH * 4 + small + (2 * x * B * nH * 258 * 4 if x > 1 else 0) for x in splits},
             "quantise": 2 * live * nH * d * 2 + 2 * B * S * nH * d + 2 * B * nH * 4 + (2 * B * S * 8 if padded else 0)}
    rec = {"B": B, "nH": nH, "d_kv": d, "S": S, "padded": padded, "live_keys": live, "workgroups": B * nH}
    for k in fns:
        rec[k] = {**stats(us[k]), "bytes_model": model[k],
                  "TB_per_s_over_model": round(model[k] / (statistics.median(us[k]) * 1e-6) / 1e12, 3)}
    if splits:
        for x in splits:
            r = rec[f"kv8_s{x}"]
            r["bf16_over_this"] = round(rec["bf16"]["median_us"] / r["median_us"], 3)
            r["against_bf16"] = verdict(r, rec["bf16"])
            r["against_kv8_s1"] = verdict(r, rec["kv8_s1"]) if x > 1 else None
            r["max_abs_diff_vs_bf16"] = float((keep[f"kv8_s{x}"].float() - keep["bf16"].float()).abs().max())
        return rec
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


def parity_d256(dev):
    """The cases of tests/test_gpu_t5_cross_kv8_d256.py (its S, the four masks, splits 1 / 2 / 3)."""
    import t5_decode_attn_checks as A

    geo = {x: P.t5_decode_cross_attention_kv8_d256_geometry(A.CROSS_S[-1], x) for x in (1, 2, 3)}
    breaks = {geo[1][k] for k in ("rows_per_wave_load", "lane_groups", "keys_per_trip")} | {geo[x]["keys_per_range"] for x in (2, 3)}
    cases, worst = {}, {"ratio": 0.0, "kv8": 0.0, "bf16": 0.0}
    for Sx in sorted(set(A.CROSS_S) | {e + o for e in breaks for o in (-1, 0, 1)}):
        for kind in A.MASKS:
            c = A.cross_case(torch.bfloat16, 256, Sx, kind)
            q, K, V, m = (None if x is None else x.to(dev) for x in (c["q"], c["K"], c["V"], c["mask"]))
            kv8 = P.t5_quantize_cross_kv(K, V, m)
            Kd, Vd = kv8.dequantize()
            ref = A.oracle_cross(c["q"], c["K"], c["V"], c["mask"])
            ref_deq = A.oracle_cross(c["q"], Kd.cpu(), Vd.cpu(), c["mask"])
            limit = A.bound(torch.bfloat16, A.max_err(A.eager_cross(q, Kd, Vd, m), ref_deq), ref_deq)
            e = {"bound_of_the_rule": limit, "bf16_kernel_vs_oracle_on_original": A.max_err(P.t5_decode_cross_attention(q, K, V, m), ref),
                 "max_abs_oracle": float(ref.abs().max())}
            for x in (1, 2, 3):
                out8 = P.t5_decode_cross_attention_kv8(q, kv8, m, splits=x)
                e[f"splits{x}_vs_oracle_on_dequantised"] = A.max_err(out8, ref_deq)
                e[f"splits{x}_vs_oracle_on_original"] = A.max_err(out8, ref)
                worst["ratio"] = max(worst["ratio"], e[f"splits{x}_vs_oracle_on_dequantised"] / limit)
                worst["kv8"] = max(worst["kv8"], e[f"splits{x}_vs_oracle_on_original"])
            worst["bf16"] = max(worst["bf16"], e["bf16_kernel_vs_oracle_on_original"])
            cases[f"S{Sx}_{kind}"] = e
    return {"tool": "tools/t5_cross_kv8_bench.py --set d256 --parity-out", "device": torch.cuda.get_device_name(0),
            "what": "max |out - float64 oracle| per case (B 3, nH 5, d_kv 256, bf16 inputs of tests/t5_decode_attn_checks.cross_case)",
            "worst_e_kernel_over_bound_on_dequantised": worst["ratio"],
            "worst_kv8_vs_oracle_on_original": worst["kv8"], "worst_bf16_kernel_vs_oracle_on_original": worst["bf16"],
            "note": "the rows against the original keys are the quantisation's cost: measured, not a tolerance", "cases": cases}


def ab_child():
    """Per-call us of the two entries that existed before, on whatever library TRLX_T5_AMD_LIB names."""
    lib = ctypes.CDLL(P._lib.LIB_PATH)
    for n in [n for n in P._lib.SIGNATURES if not hasattr(lib, n)]:   # an older build lacks the newer entries
        del P._lib.SIGNATURES[n]
    dev = torch.device("cuda:0")
    B, nH, d = 128, 32, 128
    g = torch.Generator(device=dev).manual_seed(3)
    q = (torch.randn(B, nH * d, generator=g, device=dev) * d ** -0.25).to(torch.bfloat16)
    K = (torch.randn(B, nH, S, d, generator=g, device=dev) * d ** -0.25).to(torch.bfloat16)
    V = torch.randn(B, nH, S, d, generator=g, device=dev).to(torch.bfloat16)
    mask = torch.ones(B, S, dtype=torch.int64, device=dev)
    mask[:, S - 37:] = 0
    kv8 = P.t5_quantize_cross_kv(K, V, mask)
    res = {}
    for name, fn in (("t5_decode_attn_kv8_nH32_d128_B128", lambda: P.t5_decode_cross_attention_kv8(q, kv8, mask)),
                     ("t5_cross_kv_quantize_nH32_d128_B128", lambda: P.t5_quantize_cross_kv(K, V, mask, out=kv8))):
        for _ in range(10):
            fn()
        per = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1000.0 / 10)
        res[name] = statistics.median(per)
    print("AB_CHILD " + json.dumps(res))


def existing_entries_ab(parent_lib, runs=4):
    sides = {"parent": os.path.abspath(parent_lib), "this_tree": P._lib.LIB_PATH}
    got = {s: {} for s in sides}
    for _ in range(runs):
        for side, lib in sides.items():   # alternating child processes
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child"], env=dict(os.environ, TRLX_T5_AMD_LIB=lib),
                               capture_output=True, text=True, timeout=300, check=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_CHILD ")][-1]
            for k, v in json.loads(line[len("AB_CHILD "):]).items():
                got[side].setdefault(k, []).append(v)
    out = {"unit": "us per call (HIP events around 10 calls, median of 30), one figure per child process",
           "criterion": "this tree's median inside the parent's own min-max spread"}
    for k in got["parent"]:
        p, c = got["parent"][k], got["this_tree"][k]
        med = statistics.median(c)
        out[k] = {"parent": p, "this_tree": c, "this_tree_median": med,
                  "verdict": "inside" if min(p) <= med <= max(p) else ("faster" if med < min(p) else "REGRESSION")}
    return out


def dump(obj, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(obj, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--set", choices=("base", "d256"), default="base")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity-out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-child", action="store_true")
    args = ap.parse_args()
    if args.ab_child:
        return ab_child()
    d256 = args.set == "d256"
    out = args.out or os.path.join(ROOT, "profiles", "t5_cross_kv8_d256_bench.json" if d256 else "t5_cross_kv8_bench.json")
    rec = {"tool": "tools/t5_cross_kv8_bench.py" + (" --set d256" if d256 else ""), "reps": args.reps,
           "timing": "HIP events around single calls, bf16 / kv8 / quantise interleaved, order shuffled per repetition",
           "shapes": {}}
    if args.parent_lib:   # first: no GPU context in this process while the children run
        rec["existing_entries_ab"] = existing_entries_ab(args.parent_lib)
        print(json.dumps(rec["existing_entries_ab"]), flush=True)
    dev = torch.device("cuda:0")
    rec["device"] = torch.cuda.get_device_name(0)
    rng = random.Random(8)
    for name, B, nH, d in (MODELS_D256 if d256 else MODELS):
        for padded in (False, True):
            key = f"{name}_cross_S{S}" + ("_padded" if padded else "")
            rec["shapes"][key] = bench_shape(B, nH, d, padded, dev, args.reps, args.warmup, rng, D256_SPLITS if d256 else ())
            print(key, json.dumps(rec["shapes"][key]), flush=True)
    if d256:
        rec["fp8_or_a_split_does_not_win"] = [
            f"{key}: kv8_s{x} {sh[f'kv8_s{x}']['median_us']} us is {sh[f'kv8_s{x}'][w]} against {o} {sh[o]['median_us']} us"
            for key, sh in rec["shapes"].items() for x in D256_SPLITS
            for w, o in (("against_bf16", "bf16"), ("against_kv8_s1", "kv8_s1")) if sh[f"kv8_s{x}"][w] in ("slower", "tie")]
    dump(rec, out)
    if args.parity_out:
        par = parity_d256(dev) if d256 else parity(dev)
        print("parity", json.dumps({k: v for k, v in par.items() if k != "cases"}), flush=True)
        dump(par, args.parity_out)


if __name__ == "__main__":
    main()
