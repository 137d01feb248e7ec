"""ILQL training-batch assembly at N = 4096 samples of U{8..64} tokens, batches of 128: the
reference's route (pad_sequence collate of per-sample host tensors, tests/ilql_store_checks.py,
then six `.to(device)` copies) against ILQLRolloutStorage.collate (one trlx_ilql_collate launch
on the device-resident ragged store).  The two routes alternate in one process on the same
index lists; each call is timed with the host clock around work that ends in a device
synchronise (the host route's cost is host work, which device events would not see).  One JSON
line is printed: medians and minima in ms, which route is faster (a difference inside 5 %, the
README's box-to-box spread, is "not faster"), and the store's device bytes against a padded
[N, Lmax] layout's (computed from the shapes, not timed).
GPU-box tool:  python tools/ilql_store_bench.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
import ilql_store_checks as C  # noqa: E402

N, LMIN, LMAX, BATCH, VOCAB = 4096, 8, 64, 128, 50257


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(LMIN, LMAX + 1, (N,), generator=g).tolist()
    ids = [torch.randint(0, VOCAB, (n,), generator=g) for n in lens]
    rewards = (3 * torch.randn(N, generator=g) + 1).tolist()
    lists = C.make_experience(ids, rewards)  # the reference's per-sample host tensors
    store = P.ILQLRolloutStorage.from_samples(ids, rewards, device=dev)
    order = torch.randperm(N, generator=g)
    order_dev, order_host = order.to(dev), order.numpy()
    nb = N // BATCH
    keep = {}

    def host_route(k):
        ix = order_host[k * BATCH:(k + 1) * BATCH].tolist()
        b = C.collate(lists, ix)
        keep["host"] = [b[f].to(dev) for f in C.FIELDS]

    def device_route(k):
        lo, hi = k * BATCH, (k + 1) * BATCH
        batch = store.collate(order_dev[lo:hi], order_host[lo:hi])
        keep["device"] = [getattr(batch, f) for f in C.FIELDS]

    routes = {"host": host_route, "device": device_route}
    ms = {k: [] for k in routes}
    same = True
    for rep in range(args.warmup + args.reps):
        k = rep % nb
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                ms[name].append(dt)
        for f, h, d in zip(C.FIELDS, keep["host"], keep["device"]):  # same batch, outside the timed windows
            if f == "rewards":
                same &= bool(torch.allclose(h, d, rtol=1e-5, atol=1e-6))
            else:
                same &= h.dtype == d.dtype and bool(torch.equal(h, d))

    len_L = np.asarray(lens)
    len_A, len_S = len_L - 1, len_L
    ragged = store.device_bytes()
    padded = N * (2 * 8 * int(len_L.max()) + 2 * 8 * int(len_S.max()) + (8 + 4) * int(len_A.max()))
    rec = {
        "tool": "ilql_store_bench",
        "shape": {"N": N, "lengths": f"U{{{LMIN}..{LMAX}}}", "batch": BATCH, "tokens": int(len_L.sum())},
        "device": torch.cuda.get_device_name(0),
        "collate": {k: summary(v) for k, v in ms.items()},
        "batches_agree": same,
        "store_bytes": {"ragged": ragged, "padded_N_by_Lmax": padded, "ragged_over_padded": round(ragged / padded, 4)},
    }
    c = rec["collate"]
    h, d = c["host"]["median_ms"], c["device"]["median_ms"]
    c["faster"] = "device" if d < 0.95 * h else "host" if h < 0.95 * d else "neither (inside 5 %)"
    c["host_over_device"] = round(h / d, 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
