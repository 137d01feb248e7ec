"""One PPO rollout chunk at the C2 shape (B 128, T 48, V 50257, bf16) and the C3 shard shape
(B 256, T 48, V 32128, bf16), the experience side on two routes:

  parent   T calls of ppo_sample_step, each step's policy and reference slab written into
           [B, T, V] tensors (what a teacher-forced second pass leaves behind), then
           PPOHotPath.experience on them
  record   T recording steps (ppo_sample_step with ref_logits= and a PPORolloutRecorder bound to
           the hot path), then PPOHotPath.experience_from_logprobs

and the recording step alone against the plain step alone (T calls each, reported per step
beside "plain step + one more [B, V] slab at the row rate").  The per-step slabs come from
seeded generators and are built once, outside the timed region.  The routes alternate in one
process; HIP events, medians of --reps.  One JSON line, also written to --out.
GPU-box tool:  python tools/rollout_record_bench.py [--reps N] [--out FILE]"""
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

SHAPES = {"c2": (128, 48, 50257), "c3_shard": (256, 48, 32128)}
# README "Measured", C2: the experience rows read 2 x 617 MB in about 186 us
ROW_RATE = 2 * 128 * 48 * 50257 * 2 / 186e-6  # bytes / s


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


def run_shape(name, B, T, V, reps, warmup, dev):
    dt, es = torch.bfloat16, 2
    g = torch.Generator(device=dev).manual_seed({"c2": 1, "c3_shard": 2}.get(name, 0))
    pol = torch.empty(T, B, V, dtype=dt, device=dev)
    ref = torch.empty(T, B, V, dtype=dt, device=dev)
    for t in range(T):  # per-step slabs (fp32 temporaries of one slab only)
        x = 3.0 * torch.randn(B, V, generator=g, device=dev)
        pol[t] = x.to(dt)
        ref[t] = (x + 0.3 * torch.randn(B, V, generator=g, device=dev)).to(dt)
    del x
    u = torch.rand(T, B, generator=g, device=dev)
    vals = torch.randn(T, B, generator=g, device=dev)
    scores = torch.rand(B, generator=g, device=dev) * 8 - 4
    cfg = P.PPOConfig()
    hp_parent = P.PPOHotPath(cfg, B, T, V, dt, dev, kl_coef=0.05)
    hp_record = P.PPOHotPath(cfg, B, T, V, dt, dev, kl_coef=0.05)
    rec = P.PPORolloutRecorder(B, T, dev, 0, None, hot_path=hp_record)
    btv, ref_btv = torch.empty(B, T, V, dtype=dt, device=dev), torch.empty(B, T, V, dtype=dt, device=dev)
    tokens = torch.zeros(B, T, dtype=torch.int64, device=dev)
    old_values = torch.empty(B, T, device=dev)
    out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    unf = torch.ones(B, dtype=torch.int64, device=dev)
    kw = dict(temperature=1.0, top_k=0, top_p=1.0, pad_token_id=0, out=out)
    stream = torch.cuda.current_stream(dev)

    def plain_steps(collect=False):
        unf.fill_(1)
        for t in range(T):
            ids, _ = P.ppo_sample_step(pol[t], u=u[t], unfinished=unf, cur_len=t, **kw)
            if collect:
                tokens[:, t].copy_(ids.view(B))
                old_values[:, t].copy_(vals[t])
                btv[:, t].copy_(pol[t])
                ref_btv[:, t].copy_(ref[t])

    def parent():
        plain_steps(collect=True)
        hp_parent.experience(btv, ref_btv, tokens, old_values, scores)

    def record_steps():
        rec.t = 0
        rec.unfinished.fill_(1)
        for t in range(T):
            P.ppo_sample_step(pol[t], u=u[t], cur_len=t, ref_logits=ref[t], recorder=rec, values=vals[t], **kw)

    def record():
        record_steps()
        hp_record.experience_from_logprobs(rec.tokens, rec.values, scores)

    ms = interleaved({"parent": parent, "record": record, "plain_steps": plain_steps, "record_steps": record_steps},
                     reps, warmup, stream)
    same_tokens = bool(torch.equal(tokens, rec.tokens))
    agree = {k: bool(torch.allclose(getattr(hp_parent, k), getattr(hp_record, k), rtol=1e-5, atol=1e-6))
             for k in ("rewards", "adv_raw", "returns")}
    r = {k: summary(v) for k, v in ms.items()}
    slab = B * V * es
    r["faster_route"] = "record" if r["record"]["median_ms"] < r["parent"]["median_ms"] else "parent"
    r["parent_over_record"] = round(r["parent"]["median_ms"] / r["record"]["median_ms"], 3)
    plain_us = r["plain_steps"]["median_ms"] / T * 1e3
    r["per_step_us"] = {"plain": round(plain_us, 2), "record": round(r["record_steps"]["median_ms"] / T * 1e3, 2),
                        "plain_plus_one_slab_at_row_rate": round(plain_us + slab / ROW_RATE * 1e6, 2)}
    small = B * T * (8 + 4 + 4 + 4)  # tokens, lp, ref_lp, values
    r["bytes"] = {"slab": slab,
                  "parent_moved": T * 5 * slab + 2 * T * slab,  # step read + two slab copies; experience re-read
                  "record_moved": T * 2 * slab + small,
                  "parent_held": 2 * T * slab + small, "record_held": small}
    r["same_tokens"], r["outputs_agree"] = same_tokens, agree
    r["shape"] = {"B": B, "T": T, "V": V, "dtype": "bfloat16"}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="c2,c3_shard")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_record_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"tool": "rollout_record_bench", "device": torch.cuda.get_device_name(0), "row_rate_TB_per_s":
           round(ROW_RATE / 1e12, 3)}
    for name in args.shapes.split(","):
        rec[name] = run_shape(name, *SHAPES[name], args.reps, args.warmup, dev)
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
