"""The grouped decode cross-attention on MFMA (t5_decode_cross_attention_grouped_mma) against the two
routes that exist: built like tools/t5_cross_group_bench.py.

  a_expanded     t5_decode_cross_attention on K / V repeat_interleave'd to [P*G, nH, S, d], contiguous
  b_grouped      t5_decode_cross_attention_grouped on the shared [P, nH, S, d], at its default tile
  d_grouped_mma  t5_decode_cross_attention_grouped_mma on the same shared tensors

All routes run interleaved in one process on the same values, their order shuffled per repetition,
each call between two HIP events after warm-up; medians of --reps (default 20) with min and max.
Before anything is timed every route's result is held to the rule of the GPU test: max|route -
float64| <= 2 * e_torch + one bf16 ulp of max|float64|, e_torch from torch's eager bf16 route on the
expanded operands.  Byte models (live = the unmasked keys per prompt, summed; e = 2): a 2 * G * live *
nH * d * e, b 2 * live * nH * d * e per prompt (what it needs; the kernel re-reads per tile of 4),
d 2 * ceil(G / 16) * live * nH * d * e, each + q + out.  A difference between two routes counts only
when the medians differ by more than the slower route's own max - min: `verdicts` applies that rule
and `mma_does_not_win` lists every shape where d does not beat the better of a and b by it.

--parity: no timing; the cases of tests/test_gpu_t5_cross_group_mma.py's accuracy test, the largest
e_kernel / bound per d_kv written to --out (profiles/t5_cross_group_mma_parity.json).

    python tools/t5_cross_group_mma_bench.py [--reps N] [--out FILE] [--parity]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
BF = torch.bfloat16
S = 512
# name, P, G, nH, d, padded variants
SHAPES = [(f"t5base_P{256 // g}_G{g}", 256 // g, g, 12, 64, (False, True)) for g in (4, 8, 16, 32, 64)] + \
         [(f"nH32_d128_P{128 // g}_G{g}", 128 // g, g, 32, 128, (False,)) for g in (8, 16)] + \
         [("t5base_P2_G4", 2, 4, 12, 64, (False,))]
ROUTES = ("a_expanded", "b_grouped", "d_grouped_mma")


def bf16_ulp(x):
    return 0.0 if x <= 0 else 2.0 ** (torch.tensor(x).log2().floor().item() - 7)


def oracle(q, K, V, mask, G):
    """float64 softmax(q·K^T)·V per prompt on the device, masked keys excluded; [P*G, nH*d]."""
    Pn, nH, Sn, d = K.shape
    s = torch.einsum("pgnd,pnsd->pgns", q.view(Pn, G, nH, d).double(), K.double())
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    return torch.einsum("pgns,pnsd->pgnd", torch.softmax(s, -1), V.double()).reshape(Pn * G, nH * d)


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "n": len(us)}


def verdict(x, y):
    """x against y by the spread rule: 'faster', 'slower' or 'no difference'."""
    slow = x if x["median_us"] >= y["median_us"] else y
    if abs(x["median_us"] - y["median_us"]) <= slow["max_us"] - slow["min_us"]:
        return "no difference"
    return "faster" if x["median_us"] < y["median_us"] else "slower"


def bench_shape(Pn, G, nH, d, padded, dev, reps, warmup, rng):
    g = torch.Generator(device=dev).manual_seed(S + Pn + G)
    s, B, inner, e = d ** -0.25, Pn * G, nH * d, 2
    q = (torch.randn(B, inner, generator=g, device=dev) * s).to(BF)
    K = (torch.randn(Pn, nH, S, d, generator=g, device=dev) * s).to(BF)
    V = torch.randn(Pn, nH, S, d, generator=g, device=dev).to(BF)
    Kx, Vx = K.repeat_interleave(G, 0).contiguous(), V.repeat_interleave(G, 0).contiguous()
    mask, maskx, live = None, None, Pn * S
    if padded:
        lengths = torch.randint(S // 4, S + 1, (Pn,), generator=g, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] < lengths[:, None]).long()
        maskx = mask.repeat_interleave(G, 0).contiguous()
        live = int(mask.sum())
    keep = {}
    fns = {"a_expanded": lambda: keep.__setitem__("a_expanded", P.t5_decode_cross_attention(q, Kx, Vx, maskx)),
           "b_grouped": lambda: keep.__setitem__("b_grouped", P.t5_decode_cross_attention_grouped(q, K, V, mask)),
           "d_grouped_mma": lambda: keep.__setitem__("d_grouped_mma", P.t5_decode_cross_attention_grouped_mma(q, K, V, mask))}
    with torch.no_grad():
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        want = oracle(q, K, V, mask, G)
        e_t = float((P.t5_decode._torch_cross_attention(q, Kx, Vx, maskx).double() - want).abs().max())
        lim = 2.0 * e_t + bf16_ulp(float(want.abs().max()))
        errs = {r: float((keep[r].double() - want).abs().max()) for r in ROUTES}
        for r in ROUTES:
            assert errs[r] <= lim, f"{r}: error {errs[r]} above the bound {lim}"
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
    small = 2 * B * inner * e
    tiles = -(-G // 16)
    model = {"a_expanded": 2 * G * live * inner * e + small + (B * S * 8 if padded else 0),
             "b_grouped": 2 * live * inner * e + small + (Pn * S * 8 if padded else 0),
             "d_grouped_mma": 2 * tiles * live * inner * e + small + (Pn * tiles * S * 8 if padded else 0)}
    groups = {"a_expanded": B * nH, "b_grouped": Pn * nH * -(-G // min(4, G)), "d_grouped_mma": Pn * nH * tiles}
    rec = {"P": Pn, "G": G, "B": B, "nH": nH, "d_kv": d, "S": S, "padded": padded, "live_keys_per_prompt_summed": live,
           "e_torch": e_t, "bound": lim, "e_route": errs}
    for k in fns:
        med = statistics.median(us[k])
        rec[k] = {**stats(us[k]), "bytes_model": model[k], "TB_per_s_over_model": round(model[k] / (med * 1e-6) / 1e12, 3),
                  "workgroups": groups[k]}
    best = min(("a_expanded", "b_grouped"), key=lambda r: rec[r]["median_us"])
    rec["verdicts"] = {"d_vs_a": verdict(rec["d_grouped_mma"], rec["a_expanded"]),
                       "d_vs_b": verdict(rec["d_grouped_mma"], rec["b_grouped"]),
                       "best_existing": best, "d_vs_best_existing": verdict(rec["d_grouped_mma"], rec[best])}
    return rec


def parity(dev):
    """The accuracy test's cases, figures only: the worst e_kernel / bound per d_kv."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import t5_cross_split_checks as C
    import t5_decode_attn_checks as A
    GS, worst = (1, 7, 16, 17, 33), {}
    for d in A.D_KVS:
        w = P.t5_decode.t5_decode_cross_attention_grouped_mma_waves(d)
        for Sn in sorted({1, 31, 32, 33, 32 * w - 1, 32 * w, 32 * w + 1, 200}):
            for Gn in GS:
                for kind in A.MASKS:
                    want, e_t = C.reference(BF, d, Sn, kind, Gn, str(dev))
                    c = C.group_case(BF, d, Sn, kind, Gn)
                    got = P.t5_decode_cross_attention_grouped_mma(
                        c["q"].to(dev), C.poison(c["K"], c["mask"]).to(dev), C.poison(c["V"], c["mask"]).to(dev),
                        None if c["mask"] is None else c["mask"].to(dev))
                    e_k, lim = A.max_err(got, want), 2.0 * e_t + A.bf16_ulp(float(want.abs().max()))
                    ratio = 0.0 if e_k == 0.0 else e_k / lim
                    if ratio >= worst.get(f"d{d}", {}).get("e_kernel_over_bound", -1.0):
                        worst[f"d{d}"] = dict(d_kv=d, waves=w, S=Sn, G=Gn, mask=kind, e_torch=e_t, e_kernel=e_k, bound=lim,
                                              e_kernel_over_bound=ratio)
    return {"tool": "tools/t5_cross_group_mma_bench.py --parity",
            "rule": "e_kernel <= 2 * e_torch + one bf16 ulp of max|oracle|; e = max abs error against the float64 oracle, "
                    "e_torch = torch's eager bf16 route on the device",
            "cases": "bf16 x d_kv 64, 128 x G 1, 7, 16, 17, 33 x S 1, 31, 32, 33, 32 W - 1, 32 W, 32 W + 1, 200 x masks none, "
                     "right, left, holes; P 3, nH 5; K / V hold NaN in the masked rows",
            "worst_e_kernel_over_bound": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.parity:
        rec = parity(dev)
        out = args.out or os.path.join(ROOT, "profiles", "t5_cross_group_mma_parity.json")
    else:
        rec = {"tool": "tools/t5_cross_group_mma_bench.py", "reps": args.reps, "device": torch.cuda.get_device_name(0),
               "timing": "HIP events around single calls, all routes interleaved, order shuffled per repetition",
               "waves_per_workgroup": {f"d{d}": P.t5_decode.t5_decode_cross_attention_grouped_mma_waves(d) for d in (64, 128)},
               "shapes": {}}
        rng = random.Random(8)
        for name, Pn, G, nH, d, pads in SHAPES:
            for padded in pads:
                key = f"{name}_S{S}" + ("_padded" if padded else "")
                rec["shapes"][key] = bench_shape(Pn, G, nH, d, padded, dev, args.reps, args.warmup, rng)
                print(key, json.dumps(rec["shapes"][key]), flush=True)
        rec["mma_does_not_win"] = [f"{key}: d {sh['d_grouped_mma']['median_us']} us, {sh['verdicts']['best_existing']} "
                                   f"{sh[sh['verdicts']['best_existing']]['median_us']} us ({sh['verdicts']['d_vs_best_existing']})"
                                   for key, sh in rec["shapes"].items() if sh["verdicts"]["d_vs_best_existing"] != "faster"]
        print("mma_does_not_win", json.dumps(rec["mma_does_not_win"]), flush=True)
        out = args.out or os.path.join(ROOT, "profiles", "t5_cross_group_mma_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec if args.parity else rec["waves_per_workgroup"]))


if __name__ == "__main__":
    main()
