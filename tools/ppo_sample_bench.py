"""PPO rollout sampling step (trlx_ppo_sample) vs a torch restatement of the same chain
(HF generate's sample path of transformers 4.21: temperature, top-k, top-p over a sort,
softmax, torch.multinomial, logprob of the token), HIP events, medians, interleaved.
GPU-box tool:  python tools/ppo_sample_bench.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()

SETTINGS = [dict(temperature=0.5, top_p=0.7, top_k=0), dict(temperature=1.0, top_p=1.0, top_k=1),
            dict(temperature=1.0, top_p=0.9, top_k=50)]
SHAPES = [(torch.float32, 50257), (torch.bfloat16, 50257), (torch.bfloat16, 32128)]


def torch_step(logits, temperature, top_k, top_p):
    scores = logits.float()
    if temperature != 1.0:
        scores = scores / temperature
    if top_k > 0:
        scores = scores.masked_fill(scores < torch.topk(scores, top_k)[0][..., -1, None], float("-inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=True)
        remove = sorted_logits.softmax(-1).cumsum(-1) > top_p
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = 0
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), float("-inf"))
    ids = torch.multinomial(F.softmax(scores, -1), num_samples=1)
    return ids, F.log_softmax(logits.float(), -1).gather(-1, ids).squeeze(-1)


def time_pair(fa, fb, reps=30):
    """Medians of two functions timed in alternation (same clocks, same cache state)."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ta)[reps // 2], sorted(tb)[reps // 2]


def main():
    dev = torch.device("cuda:0")
    lines = ["# us per decode step, median of 30, fused launch vs torch ops, interleaved; logits = 3 * randn"]
    for dt, V in SHAPES:
        for B in (16, 128):
            g = torch.Generator(device=dev).manual_seed(0)
            logits = (3 * torch.randn(B, V, generator=g, device=dev)).to(dt)
            u = torch.rand(B, generator=g, device=dev)
            out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
                   torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
            for kw in SETTINGS:
                ours, ref = time_pair(lambda: P.ppo_sample_step(logits, u=u, out=out, **kw),
                                      lambda: torch_step(logits, **kw))
                lines.append(f"{str(dt)[6:]:8s} B={B:4d} V={V} T={kw['temperature']} k={kw['top_k']:3d} p={kw['top_p']}: "
                             f"fused {ours:8.1f} us | torch {ref:8.1f} us | {ref / ours:6.2f}x "
                             f"| kept/row {float(out[3].float().mean()):8.1f}")
                print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
