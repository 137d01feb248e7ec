"""One decoder token through this project's calls, three ways: (a) eager with a host t, (b) eager
with the decode clock, (c) ONE captured step (torch.cuda.graph) replayed once per token.

The token: per layer t5_rmsnorm, a fused qkv matmul, t5_decode_self_attention, the `o` matmul,
t5_add_rmsnorm, the cross q matmul, t5_decode_cross_attention, its `o` matmul, t5_add_rmsnorm, the
packed wi matmul, t5_ff_act_packed, the wo matmul; then the residual add of the last layer with the final
norm, the lm_head matmuls of the policy and the reference rows, the recording sampling step and
clock.advance().  The projections are plain bf16 torch.matmuls on fixed weights.  Shapes: L 12,
nH 12, d_kv 64, D 768, F 2048 gated, V 32128, S 512, T 48, at B 256 and B 8.

The routes run interleaved in one process, their order shuffled per repetition; each sample is a
whole T-token rollout between two HIP events; the figure is the median of --reps rollouts, in ms
per token.  A wrapper that cannot be captured (probed one by one on a graph of its own) is left out
of all three routes and named in the output.

--parent-lib PATH: also the A/B of the entries that existed before the clock (trlx_t5_decode_attn,
self, T5-base B 256 t 47; the recording step at B 256, V 32128) against another build of the
library, in alternating child processes, four runs each: this tree's median must lie inside the
other build's own min-max spread, else it is reported as a regression with both spreads.

    python tools/t5_decode_graph_bench.py [--parent-lib other/libtrlx_t5_amd.so]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

P = __graft_entry__.load_package()
from trlx_t5_amd import _lib  # noqa: E402

L, NH, DKV, D, F, V, S, T = 12, 12, 64, 768, 2048, 32128, 512, 48
INNER = NH * DKV
DT = torch.bfloat16
WRAPPERS = ("t5_rmsnorm", "t5_add_rmsnorm", "t5_ff_act_packed", "t5_decode_cross_attention")


class Decoder:
    def __init__(self, B, dev, skip=()):
        g = torch.Generator(device=dev).manual_seed(B)

        def w(*shape, scale):
            return (torch.randn(*shape, generator=g, device=dev) * scale).to(DT)

        self.B, self.dev, self.skip = B, dev, set(skip)
        self.layers = [dict(qkv=w(D, 3 * INNER, scale=D ** -0.5), o=w(INNER, D, scale=INNER ** -0.5),
                            cq=w(D, INNER, scale=D ** -0.5), co=w(INNER, D, scale=INNER ** -0.5),
                            wi=w(D, 2 * F, scale=D ** -0.5), wo=w(F, D, scale=F ** -0.5),
                            ln=[torch.ones(D, dtype=DT, device=dev) for _ in range(3)],
                            k_enc=w(B, NH, S, DKV, scale=DKV ** -0.25), v_enc=w(B, NH, S, DKV, scale=1.0))
                       for _ in range(L)]
        self.final_ln = torch.ones(D, dtype=DT, device=dev)
        self.lm, self.ref_lm = w(D, V, scale=D ** -0.5), w(D, V, scale=D ** -0.5)
        self.mask = torch.ones(B, S, dtype=torch.int64, device=dev)
        self.mask[:, S - 37:] = 0
        self.table = P.t5_relative_bias_table(torch.randn(32, NH, generator=g, device=dev), T)
        self.x = w(B, D, scale=1.0)
        self.u = torch.rand(T, B, generator=g, device=dev)
        self.out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev),
                    torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev))

    def rollout_state(self, clocked):
        clock = P.T5DecodeClock(T, self.dev) if clocked else None
        caches = [P.T5DecodeKVCache(self.B, NH, DKV, T, DT, self.dev) for _ in range(L)]
        rec = P.PPORolloutRecorder(self.B, T, self.dev, pad_token_id=0, eos_token_id=None, clock=clock)
        return clock, caches, rec

    def norm(self, h, wt):
        return h if "t5_rmsnorm" in self.skip else P.t5_rmsnorm(h, wt)

    def add_norm(self, x, res, wt):
        if "t5_add_rmsnorm" in self.skip:
            return res, x
        return P.t5_add_rmsnorm(x, res, wt)

    def token(self, state, t):
        """One token; t: the host int of routes (a), or None with a clocked state."""
        clock, caches, rec = state
        h = self.x
        y = self.norm(h, self.layers[0]["ln"][0])
        for i, w in enumerate(self.layers):
            qkv = torch.matmul(y, w["qkv"])
            q, kn, vn = (qkv[:, j * INNER:(j + 1) * INNER] for j in range(3))
            a = P.t5_decode_self_attention(q, kn, vn, caches[i], clock if t is None else t, self.table)
            h, y = self.add_norm(torch.matmul(a, w["o"]), h, w["ln"][1])
            q2 = torch.matmul(y, w["cq"])
            c = q2 if "t5_decode_cross_attention" in self.skip else \
                P.t5_decode_cross_attention(q2, w["k_enc"], w["v_enc"], self.mask)
            h, y = self.add_norm(torch.matmul(c, w["co"]), h, w["ln"][2])
            uv = torch.matmul(y, w["wi"])
            f = uv[:, :F] if "t5_ff_act_packed" in self.skip else P.t5_ff_act_packed(uv)
            nxt = self.layers[i + 1]["ln"][0] if i + 1 < L else self.final_ln
            h, y = self.add_norm(torch.matmul(f, w["wo"]), h, nxt)
        logits, ref = torch.matmul(y, self.lm), torch.matmul(y, self.ref_lm)
        if t is None:
            P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, u=self.u, out=self.out, top_k=50, top_p=0.95)
            clock.advance()
        else:
            P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, u=self.u[t], out=self.out, top_k=50, top_p=0.95)


def capturable(fn):
    """Does fn() capture and replay on a graph of its own?  (fn has run eagerly once already.)"""
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return True, ""
    except Exception as e:  # noqa: BLE001 - whatever breaks the capture is the finding
        torch.cuda.synchronize()
        return False, f"{type(e).__name__}: {str(e)[:200]}"


def probe_wrappers(dev):
    B = 8
    h = torch.randn(B, D, device=dev).to(DT)
    wt = torch.ones(D, dtype=DT, device=dev)
    uv = torch.randn(B, 2 * F, device=dev).to(DT)
    q = torch.randn(B, INNER, device=dev).to(DT)
    kv = torch.randn(B, NH, 16, DKV, device=dev).to(DT)
    mask = torch.ones(B, 16, dtype=torch.int64, device=dev)
    calls = {"t5_rmsnorm": lambda: P.t5_rmsnorm(h, wt), "t5_add_rmsnorm": lambda: P.t5_add_rmsnorm(h, h, wt),
             "t5_ff_act_packed": lambda: P.t5_ff_act_packed(uv),
             "t5_decode_cross_attention": lambda: P.t5_decode_cross_attention(q, kv, kv, mask)}
    left_out = {}
    with torch.no_grad():
        for name in WRAPPERS:
            calls[name]()
            torch.cuda.synchronize()
            ok, why = capturable(calls[name])
            if not ok:
                left_out[name] = why
    return left_out


def run_shape(B, dev, reps, skip):
    dec = Decoder(B, dev, skip)
    sa, sb, sc = dec.rollout_state(False), dec.rollout_state(True), dec.rollout_state(True)

    def rearm(state):   # the position back to 0 without the recorder's fills (not what is timed)
        clock, _, rec = state
        rec.t = 0
        if clock is not None:
            clock.reset()

    def route_a():
        rearm(sa)
        for t in range(T):
            dec.token(sa, t)

    def route_b():
        rearm(sb)
        for _ in range(T):
            dec.token(sb, None)

    with torch.no_grad():
        route_a()
        route_b()
        dec.token(sc, None)   # warm-up of the captured state
        torch.cuda.synchronize()
        rearm(sc)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):   # one stream, a linear chain of launches
            dec.token(sc, None)

        def route_c():
            rearm(sc)
            for _ in range(T):
                graph.replay()

        routes = {"a_eager_host_t": route_a, "b_eager_clock": route_b, "c_graph_replay": route_c}
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        assert sc[0].t == T and sc[0].overrun == 0
        same = all(torch.equal(getattr(sa[2], f), getattr(sc[2], f)) and torch.equal(getattr(sa[2], f), getattr(sb[2], f))
                   for f in ("tokens", "logprobs", "ref_logprobs"))
        samples = {k: [] for k in routes}
        order = list(routes)
        rng = random.Random(B)
        for _ in range(reps):
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                routes[k]()
                e1.record()
                e1.synchronize()
                samples[k].append(e0.elapsed_time(e1) / T)
    res = {k: {"ms_per_token_median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}
    res["fastest"] = min(routes, key=lambda k: res[k]["ms_per_token_median"])
    res["routes_record_the_same_rollout"] = bool(same)
    res["launches_per_token_in_the_graph"] = "one replay"
    return res


# ------------------------------------------------------------------ the entries that existed before
def ab_child():
    """Per-call µs of the two existing entries on whatever library TRLX_T5_AMD_LIB names."""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:   # an older build lacks the clock entries
        del _lib.SIGNATURES[n]
    dev = torch.device("cuda:0")
    B, t = 256, 47
    g = torch.Generator(device=dev).manual_seed(3)
    cache = P.T5DecodeKVCache(B, NH, DKV, T, DT, dev)
    cache.k.copy_(torch.randn(cache.k.shape, generator=g, device=dev) * DKV ** -0.25)
    cache.v.copy_(torch.randn(cache.v.shape, generator=g, device=dev))
    qkv = (torch.randn(B, 3 * INNER, generator=g, device=dev) * DKV ** -0.25).to(DT)
    q, kn, vn = (qkv[:, j * INNER:(j + 1) * INNER] for j in range(3))
    table = P.t5_relative_bias_table(torch.randn(32, NH, generator=g, device=dev), T)
    logits = (3.0 * torch.randn(B, V, generator=g, device=dev)).to(DT)
    ref = (logits.float() + 0.3 * torch.randn(B, V, generator=g, device=dev)).to(DT)
    u = torch.rand(B, generator=g, device=dev)
    rec = P.PPORolloutRecorder(B, T, dev, pad_token_id=0, eos_token_id=None)
    out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))

    def attn():
        P.t5_decode_self_attention(q, kn, vn, cache, t, table)

    def record():
        rec.t = 7
        P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, u=u, out=out, top_k=50, top_p=0.95)

    res = {}
    for name, fn in (("t5_decode_attn_self_B256_t47", attn), ("ppo_sample_record_B256_V32128", record)):
        for _ in range(20):
            fn()
        per = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1000.0 / 20)
        res[name] = statistics.median(per)
    print("AB_CHILD " + json.dumps(res))


def existing_entries_ab(parent_lib, runs=4):
    sides = {"parent": os.path.abspath(parent_lib), "this_tree": _lib.LIB_PATH}
    got = {s: {} for s in sides}
    for _ in range(runs):
        for side, lib in sides.items():   # alternating child processes
            env = dict(os.environ, TRLX_T5_AMD_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child"], env=env, capture_output=True,
                               text=True, timeout=300, check=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB_CHILD ")][-1]
            for k, v in json.loads(line[len("AB_CHILD "):]).items():
                got[side].setdefault(k, []).append(v)
    out = {"unit": "us per call (HIP events around 20 calls, median of 30), one figure per child process",
           "criterion": "this tree's median inside the parent's own min-max spread"}
    for k in got["parent"]:
        p, c = got["parent"][k], got["this_tree"][k]
        med = statistics.median(c)
        out[k] = {"parent": p, "this_tree": c, "parent_spread": [min(p), max(p)], "this_tree_spread": [min(c), max(c)],
                  "this_tree_median": med, "inside_parent_spread": min(p) <= med <= max(p),
                  "verdict": "inside" if min(p) <= med <= max(p) else ("faster" if med < min(p) else "REGRESSION")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="256,8")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_decode_graph_bench.json"))
    args = ap.parse_args()
    if args.ab_child:
        return ab_child()
    result = {"tool": "tools/t5_decode_graph_bench.py",
              "shape": dict(L=L, n_heads=NH, d_kv=DKV, D=D, F=F, V=V, S=S, T=T, dtype="bf16"),
              "timing": f"HIP events around whole {T}-token rollouts, routes interleaved and shuffled per repetition, "
                        f"median of {args.reps}, ms per token"}
    if args.parent_lib:   # first: no GPU context in this process while the children run
        result["existing_entries_ab"] = existing_entries_ab(args.parent_lib)
    dev = torch.device("cuda:0")
    result["device"] = torch.cuda.get_device_name(0)
    left_out = probe_wrappers(dev)
    result["calls_left_out_of_all_routes"] = left_out
    for B in (int(b) for b in args.batches.split(",")):
        result[f"B{B}"] = run_shape(B, dev, args.reps, left_out)
        print(f"B {B}: " + json.dumps(result[f"B{B}"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in result if k.startswith("B") or k.startswith("calls")}))
    if "existing_entries_ab" in result:
        print(json.dumps(result["existing_entries_ab"]))


if __name__ == "__main__":
    main()
