"""One decode step of the recording sampler with HF's prefix-aware processors, at the C2 decode
shape (B 128, V 50257, bf16) and the C3 shard decode shape (B 256, V 32128, bf16): a prefix of 24
tokens (the recorder's own columns), repetition_penalty 1.2, no_repeat_ngram_size 3 and 16
bad-word sequences.  Four routes on the same rows and u, interleaved in one process:

  record       (a) the plain recording step (trlx_ppo_sample_record)
  off          the new entry with every processor off (trlx_ppo_sample_proc -> the same kernel)
  proc         (b) the processing recording step (trlx_ppo_sample_proc, one launch)
  torch_edit   (c) what a caller had to do before: the processors as torch ops on a copy of the
               [B, V] slab (the unedited one is still needed for the log-probs), then (a) on it

Each timed region is --steps calls of the step (the recorder rewound to column 24 before each),
HIP events around it, reported per step: medians of --reps after warm-up, with min / max and the
quartiles as the run-to-run spread.  One JSON line, also written to --out.
GPU-box tool:  python tools/ppo_sample_proc_bench.py [--reps N] [--steps K] [--out FILE]"""
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

SHAPES = {"c2": (128, 50257), "c3_shard": (256, 32128)}
# README "Measured", C2: the experience rows read 2 x 617 MB in about 186 us
ROW_RATE = 2 * 128 * 48 * 50257 * 2 / 186e-6  # bytes / s
N_PREFIX, T, RP, NGRAM = 24, 48, 1.2, 3
NEG = float("-inf")


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


def summary(ms, steps):
    s = sorted(1e3 * m / steps for m in ms)
    q = lambda f: round(s[min(len(s) - 1, int(f * len(s)))], 2)  # noqa: E731
    return {"median_us": q(0.5), "min_us": round(s[0], 2), "q1_us": q(0.25), "q3_us": q(0.75),
            "max_us": round(s[-1], 2), "n": len(s)}


def torch_edit(x, prefix, words):
    """HF's three processors as torch ops on a copy of the slab (fp32 arithmetic on the gathered
    entries, written back in the slab's dtype as HF does)."""
    xe = x.clone()
    s = xe.gather(1, prefix).float()
    xe.scatter_(1, prefix, torch.where(s < 0, s * RP, s / RP).to(xe.dtype))
    wins = prefix.unfold(1, NGRAM, 1)
    match = (wins[:, :, :NGRAM - 1] == prefix[:, None, -(NGRAM - 1):]).all(-1)
    tgt = wins[:, :, NGRAM - 1]
    xe.scatter_(1, tgt, torch.where(match, torch.full_like(xe[:, :1], NEG), xe.gather(1, tgt)))
    for w in words:
        k = len(w) - 1
        if k == 0:
            xe[:, w[0]] = NEG
        else:
            m = (prefix[:, -k:] == torch.tensor(w[:k], device=x.device)).all(-1)
            xe[:, w[k]] = torch.where(m, torch.full_like(xe[:, 0], NEG), xe[:, w[k]])
    return xe


def run_shape(name, B, V, reps, warmup, steps, dev):
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed({"c2": 1, "c3_shard": 2}.get(name, 0))
    x = 3.0 * torch.randn(B, V, generator=g, device=dev)
    pol, ref = x.to(dt), (x + 0.3 * torch.randn(B, V, generator=g, device=dev)).to(dt)
    del x
    u = torch.rand(B, generator=g, device=dev)
    # prefixes from 40 tokens per row among the row's 200 largest logits: repeats, and edits that matter
    top = pol.float().topk(200, -1).indices
    pool = top.gather(1, torch.randint(0, 200, (B, 40), generator=g, device=dev))
    prefix = pool.gather(1, torch.randint(0, 40, (B, N_PREFIX), generator=g, device=dev))
    gw = torch.Generator().manual_seed(3)
    words = [[int(t) for t in torch.randint(2, V, (1 + i % 3,), generator=gw)] for i in range(16)]
    pr = P.PPOLogitsProcessors(V, dev, repetition_penalty=RP, no_repeat_ngram_size=NGRAM, bad_words_ids=words)
    off = P.PPOLogitsProcessors(V, dev)
    rec = P.PPORolloutRecorder(B, T, dev, 0, None)
    rec.tokens[:, :N_PREFIX] = prefix
    out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    kw = dict(temperature=1.0, top_k=0, top_p=1.0, out=out, u=u, cur_len=N_PREFIX, ref_logits=ref, recorder=rec)
    stream = torch.cuda.current_stream(dev)

    def loop(fn):
        def run():
            for _ in range(steps):
                rec.t = N_PREFIX
                fn()
        return run

    fns = {"record": loop(lambda: P.ppo_sample_step(pol, **kw)),
           "off": loop(lambda: P.ppo_sample_step(pol, processors=off, **kw)),
           "proc": loop(lambda: P.ppo_sample_step(pol, processors=pr, **kw)),
           "torch_edit": loop(lambda: P.ppo_sample_step(torch_edit(pol, prefix, words), **kw))}
    ms = interleaved(fns, reps, warmup, stream)
    r = {k: summary(v, steps) for k, v in ms.items()}
    # the two routes draw the same tokens (the torch route rounds the penalised logits to bf16,
    # so a tie or a boundary may move: reported, not required)
    fns["proc"]()
    tok_proc = rec.tokens[:, N_PREFIX].clone()
    fns["torch_edit"]()
    r["same_tokens_proc_vs_torch_edit"] = float((tok_proc == rec.tokens[:, N_PREFIX]).float().mean())
    slab = B * V * 2
    a, b, c, o = (r[k]["median_us"] for k in ("record", "proc", "torch_edit", "off"))
    r["proc_over_record_us"] = round(b - a, 2)
    r["off_minus_record_us"] = round(o - a, 2)
    r["record_spread_us"] = round(r["record"]["max_us"] - r["record"]["min_us"], 2)
    r["off_spread_us"] = round(r["off"]["max_us"] - r["off"]["min_us"], 2)
    r["one_slab_at_row_rate_us"] = round(slab / ROW_RATE * 1e6, 2)
    r["proc_faster_than_torch_edit"] = bool(b < c)
    r["torch_edit_over_proc"] = round(c / b, 2)
    r["shape"] = {"B": B, "V": V, "dtype": "bfloat16", "prefix": N_PREFIX, "repetition_penalty": RP,
                  "no_repeat_ngram_size": NGRAM, "bad_words": len(words), "steps_per_region": steps}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--shapes", default="c2,c3_shard")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_sample_proc_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"tool": "ppo_sample_proc_bench", "device": torch.cuda.get_device_name(0),
           "row_rate_TB_per_s": round(ROW_RATE / 1e12, 3)}
    for name in args.shapes.split(","):
        rec[name] = run_shape(name, *SHAPES[name], args.reps, args.warmup, args.steps, dev)
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
