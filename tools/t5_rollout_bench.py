"""The captured decode step of tools/t5_decode_graph_bench.py made autoregressive: the token drawn at
step t - 1 is fed back through the `shared` embedding table, and the rows that have finished are
skipped in both attentions.  Six routes, each ONE captured step (torch.cuda.graph) replayed once
per token:

  c0_torch_feedback   the feedback as torch ops (a gather of rec.tokens at an index tensor derived
                      from clock.record, a where for t == 0, F.embedding), then t5_rmsnorm; no skip
  c1_decode_embed     t5_decode_embed(clock): the gather, the embedding row and layer 0's first norm
                      in one launch; no skip
  c2_embed_live_skip  c1 plus live=rec.unfinished on the self- and the cross-attention of every layer
  c3_live_skip_kv8    c2 with the cross-attention over fp8 keys and values (t5_quantize_cross_kv once
                      per layer outside the step, t5_decode_cross_attention_kv8 inside it).  Lossy:
                      c3 does not record c2's rollout.  Its drift is reported beside its time: the
                      largest |difference| of the recorded policy log-probs against c2 over the
                      T-token rollout at live fraction 1.0 -- over all positions, and over the
                      positions up to each row's first differing token, where both routes still score
                      the same token after the same prefix -- and the share of tokens that differ

  c4_fused_projections  c2's step with the 8-launch layer (t5_decode_layer_fused): the six projections of a
                      layer on trlx_t5_decode_linear with the norms, the residual adds and the gated
                      activation inside them; the final norm, the lm_head matmuls and the sampler as in
                      c2.  It rounds differently, so it need not record c2's rollout: its drift against
                      c2 is reported by the method of c3's, beside its time and the launches per step

  c5_fused_rows_skip  c4 with split_rows=True and live=rec.unfinished in the six projections of every
                      layer (trlx_t5_decode_linear_rows): the rows spread over workgroups and the
                      finished rows' projections skipped on the device.  Per live row it computes c4's
                      bits; its drift against c2 is reported as c4's

  c2_expanded_G4 / c2_grouped_G4 (their own section of the output, B 256 = 64 prompts x 4 samples):
                      c2 fed the keys / values of 64 prompts repeat_interleave'd to 256 rows, and c2 with
                      t5_decode_cross_attention_grouped over the ONE copy of those 64 prompts in all
                      twelve layers.  The two must record one rollout bit for bit -- asserted before
                      anything is timed -- and the K / V memory each holds is reported beside its time

The decoder is the graph bench's (L 12, nH 12, d_kv 64, D 768, F 2048 gated, V 32128, S 512, T 48,
bf16, at B 256 and B 8) with a `shared` [V, D] table.  The recorder is built with eos_token_id=None
and rec.unfinished is preset to a fixed pattern, so the sampler never changes it; every route runs at
live fractions 1.0, 0.52 (the share of valid positions of the C3 ragged batch) and 0.25.

All (route, fraction) pairs run interleaved in one process, their order shuffled per repetition;
each sample is a whole T-token rollout between two HIP events; the figure is the median of --reps
rollouts with min-max, in ms per token.  No speed-up is assumed: the output names the fastest route
per shape and fraction and says where c2 does not beat c1 or c1 does not beat c0.

--parent-lib PATH: also the A/B of the entries that existed before (trlx_t5_decode_attn, self at
t 47 and cross at S 512 with the key mask, T5-base B 256; trlx_t5_decode_linear, norm -> qkv at
T5-base, M 8) against another build of the library, in
alternating child processes, four runs each: this tree's median must lie inside the other build's
own min-max spread, else it is reported as a regression with both spreads.

    python tools/t5_rollout_bench.py [--parent-lib other/libtrlx_t5_amd.so]
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import t5_decode_graph_bench as G  # noqa: E402  (the decoder; it loads the package)

P = G.P
_lib = G._lib
L, NH, DKV, D, FF, V, S, T, INNER, DT = G.L, G.NH, G.DKV, G.D, G.F, G.V, G.S, G.T, G.INNER, G.DT
FRACTIONS = (1.0, 0.52, 0.25)
START = 0


class RolloutDecoder(G.Decoder):
    """The graph bench's decoder with the token feedback in front of it."""

    def __init__(self, B, dev):
        super().__init__(B, dev)
        g = torch.Generator(device=dev).manual_seed(B + 1)
        self.shared = torch.randn(V, D, generator=g, device=dev).to(DT)
        self.start = torch.full((B,), START, dtype=torch.int64, device=dev)
        self.kv8 = [P.t5_quantize_cross_kv(w["k_enc"], w["v_enc"], self.mask) for w in self.layers]
        # c4: the same weights in nn.Linear.weight layout [N, K]
        self.blocks = [P.T5DecodeBlockWeights(*(w[k].t().contiguous() for k in ("qkv", "o", "cq", "co", "wi", "wo")),
                                              ln=w["ln"], gated=True) for w in self.layers]
        self.bufs = dict(qkv=torch.empty(B, 3 * INNER, dtype=DT, device=dev), cq=torch.empty(B, INNER, dtype=DT, device=dev),
                         ff=torch.empty(B, FF, dtype=DT, device=dev))

    def state(self):
        clock, caches, rec = self.rollout_state(True)
        out = (torch.empty(self.B, D, dtype=DT, device=self.dev), torch.empty(self.B, D, dtype=DT, device=self.dev))
        return clock, caches, rec, out

    def feed_torch(self, state):
        clock, _, rec, _ = state
        t = clock.record[0:1]
        idx = (t - 1).clamp_min(0).expand(self.B).unsqueeze(1)
        tok = torch.where(t == 0, self.start, rec.tokens.gather(1, idx).squeeze(1))
        h = F.embedding(tok, self.shared)
        return h, P.t5_rmsnorm(h, self.layers[0]["ln"][0])

    def feed_kernel(self, state):
        clock, _, rec, out = state
        return P.t5_decode_embed(self.shared, rec, clock, START, self.layers[0]["ln"][0], out=out)

    def token_fused(self, state, rows=False):
        clock, caches, rec, out = state
        h, _ = P.t5_decode_embed(self.shared, rec, clock, START, out=(out[0], None))
        kw = dict(live=rec.unfinished)
        lkw = dict(live=rec.unfinished, split_rows=True) if rows else {}
        for i, (w, blk) in enumerate(zip(self.layers, self.blocks)):
            P.t5_decode_layer_fused(
                h, blk, lambda q, kn, vn: P.t5_decode_self_attention(q, kn, vn, caches[i], clock, self.table, **kw),
                lambda q: P.t5_decode_cross_attention(q, w["k_enc"], w["v_enc"], self.mask, **kw), bufs=self.bufs, **lkw)
        y = P.t5_rmsnorm(h, self.final_ln)
        logits, ref = torch.matmul(y, self.lm), torch.matmul(y, self.ref_lm)
        P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, u=self.u, out=self.out, top_k=50, top_p=0.95)
        clock.advance()

    def share_prompts(self, G):
        """The first B / G prompts' keys, values and mask once ([P, ...]) and repeat_interleave'd to B rows."""
        Pn = self.B // G
        self.shared_kv = [(w["k_enc"][:Pn].contiguous(), w["v_enc"][:Pn].contiguous()) for w in self.layers]
        self.expanded_kv = [(k.repeat_interleave(G, 0).contiguous(), v.repeat_interleave(G, 0).contiguous())
                            for k, v in self.shared_kv]
        self.shared_mask = self.mask[:Pn].contiguous()
        self.expanded_mask = self.shared_mask.repeat_interleave(G, 0).contiguous()

    def token(self, state, route):
        if route in ("c4_fused_projections", "c5_fused_rows_skip"):
            return self.token_fused(state, rows=route == "c5_fused_rows_skip")
        clock, caches, rec, _ = state
        h, y = self.feed_torch(state) if route == "c0_torch_feedback" else self.feed_kernel(state)
        kw = dict(live=rec.unfinished) if route in ("c2_embed_live_skip", "c3_live_skip_kv8") + GROUP_ROUTES else {}
        for i, w in enumerate(self.layers):
            qkv = torch.matmul(y, w["qkv"])
            q, kn, vn = (qkv[:, j * INNER:(j + 1) * INNER] for j in range(3))
            a = P.t5_decode_self_attention(q, kn, vn, caches[i], clock, self.table, **kw)
            h, y = P.t5_add_rmsnorm(torch.matmul(a, w["o"]), h, w["ln"][1])
            if route == "c3_live_skip_kv8":
                c = P.t5_decode_cross_attention_kv8(torch.matmul(y, w["cq"]), self.kv8[i], self.mask, **kw)
            elif route == "c2_expanded_G4":
                c = P.t5_decode_cross_attention(torch.matmul(y, w["cq"]), *self.expanded_kv[i], self.expanded_mask, **kw)
            elif route == "c2_grouped_G4":
                c = P.t5_decode_cross_attention_grouped(torch.matmul(y, w["cq"]), *self.shared_kv[i], self.shared_mask, **kw)
            else:
                c = P.t5_decode_cross_attention(torch.matmul(y, w["cq"]), w["k_enc"], w["v_enc"], self.mask, **kw)
            h, y = P.t5_add_rmsnorm(torch.matmul(c, w["co"]), h, w["ln"][2])
            f = P.t5_ff_act_packed(torch.matmul(y, w["wi"]))
            nxt = self.layers[i + 1]["ln"][0] if i + 1 < L else self.final_ln
            h, y = P.t5_add_rmsnorm(torch.matmul(f, w["wo"]), h, nxt)
        logits, ref = torch.matmul(y, self.lm), torch.matmul(y, self.ref_lm)
        P.ppo_sample_step(logits, ref_logits=ref, recorder=rec, u=self.u, out=self.out, top_k=50, top_p=0.95)
        clock.advance()


GROUP_ROUTES = ("c2_expanded_G4", "c2_grouped_G4")
GROUP_G = 4
EXACT_ROUTES = ("c0_torch_feedback", "c1_decode_embed", "c2_embed_live_skip")   # these record one rollout
ROUTES = EXACT_ROUTES + ("c3_live_skip_kv8", "c4_fused_projections", "c5_fused_rows_skip")
# launches of one step, counted from the step's code: the feedback, 12 (or 8) per layer, the final norm of
# c4, two lm_head matmuls, the sampler, the clock
LAUNCHES = {"c0_torch_feedback": None, "c1_decode_embed": 1 + 12 * L + 4, "c2_embed_live_skip": 1 + 12 * L + 4,
            "c3_live_skip_kv8": 1 + 12 * L + 4, "c4_fused_projections": 1 + 8 * L + 1 + 4,
            "c5_fused_rows_skip": 1 + 8 * L + 1 + 4}


def kv8_drift(rec2, rec3):
    """c3's recorded rollout against c2's (both at live fraction 1.0)."""
    differ = rec2.tokens != rec3.tokens
    d = (rec2.logprobs.float() - rec3.logprobs.float()).abs()
    same_prefix = differ.long().cumsum(1) == 0                    # before the row's first differing token
    return {"max_abs_logprob_drift_all_positions": float(d.max()),
            "max_abs_logprob_drift_same_token_same_prefix": float(d[same_prefix].max()) if bool(same_prefix.any()) else None,
            "share_of_tokens_that_differ": float(differ.float().mean()),
            "share_of_rows_with_a_differing_token": float(differ.any(dim=1).float().mean()),
            "positions": int(differ.numel())}


def live_pattern(B, frac, dev):
    """round(B * frac) live rows at fixed, scattered places."""
    n = max(1, round(B * frac))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(17))
    live = torch.zeros(B, dtype=torch.int64)
    live[perm[:n]] = 1
    return live.to(dev), n / B


def run_shape(B, dev, reps):
    dec = RolloutDecoder(B, dev)
    patterns = {f: live_pattern(B, f, dev) for f in FRACTIONS}
    states, graphs = {}, {}
    with torch.no_grad():
        for r in ROUTES:
            st = states[r] = dec.state()
            dec.token(st, r)                                      # warm-up
            torch.cuda.synchronize()
            st[0].reset()
            graphs[r] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[r]):                     # one stream, a linear chain of launches
                dec.token(st, r)

        def rollout(r, f):
            clock, _, rec, _ = states[r]
            clock.reset()
            rec.unfinished.copy_(patterns[f][0])
            for _ in range(T):
                graphs[r].replay()

        # the three routes record the same tokens for the rows that are live (fraction 1.0: every row)
        for r in ROUTES:
            rollout(r, 1.0)
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(states[ROUTES[0]][2], f), getattr(states[r][2], f))
                   for r in EXACT_ROUTES[1:] for f in ("tokens", "logprobs", "ref_logprobs"))
        drift = kv8_drift(states["c2_embed_live_skip"][2], states["c3_live_skip_kv8"][2])
        drift4 = kv8_drift(states["c2_embed_live_skip"][2], states["c4_fused_projections"][2])
        drift5 = kv8_drift(states["c2_embed_live_skip"][2], states["c5_fused_rows_skip"][2])
        c5_is_c4 = all(torch.equal(getattr(states["c4_fused_projections"][2], f), getattr(states["c5_fused_rows_skip"][2], f))
                       for f in ("tokens", "logprobs", "ref_logprobs"))
        assert all(states[r][0].t == T and states[r][0].overrun == 0 for r in ROUTES)
        keys = [(r, f) for r in ROUTES for f in FRACTIONS]
        samples = {k: [] for k in keys}
        rng = random.Random(B)
        for _ in range(reps):
            rng.shuffle(keys)
            for r, f in keys:
                clock, _, rec, _ = states[r]
                clock.reset()
                rec.unfinished.copy_(patterns[f][0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(T):
                    graphs[r].replay()
                e1.record()
                e1.synchronize()
                samples[(r, f)].append(e0.elapsed_time(e1) / T)
    res = {"routes_record_the_same_rollout_at_fraction_1": bool(same), "c3_kv8_against_c2_at_fraction_1": drift,
           "c4_fused_projections_against_c2_at_fraction_1": drift4,
           "c5_fused_rows_skip_against_c2_at_fraction_1": drift5,
           "c5_records_c4s_rollout_at_fraction_1": bool(c5_is_c4),
           "launches_per_step_counted_from_the_code": LAUNCHES}
    for f in FRACTIONS:
        per = {r: {"ms_per_token_median": statistics.median(samples[(r, f)]), "min": min(samples[(r, f)]),
                   "max": max(samples[(r, f)])} for r in ROUTES}
        med = {r: per[r]["ms_per_token_median"] for r in ROUTES}
        per["live_fraction_actual"] = patterns[f][1]
        per["fastest"] = min(ROUTES, key=med.get)
        per["c1_beats_c0"] = med["c1_decode_embed"] < med["c0_torch_feedback"]
        per["c2_beats_c1"] = med["c2_embed_live_skip"] < med["c1_decode_embed"]
        per["c3_beats_c2"] = med["c3_live_skip_kv8"] < med["c2_embed_live_skip"]
        per["c3_over_c2"] = med["c3_live_skip_kv8"] / med["c2_embed_live_skip"]
        per["c4_beats_c2"] = med["c4_fused_projections"] < med["c2_embed_live_skip"]
        per["c4_over_c2"] = med["c4_fused_projections"] / med["c2_embed_live_skip"]
        per["c5_beats_c4"] = med["c5_fused_rows_skip"] < med["c4_fused_projections"]
        per["c5_over_c4"] = med["c5_fused_rows_skip"] / med["c4_fused_projections"]
        per["c5_beats_c2"] = med["c5_fused_rows_skip"] < med["c2_embed_live_skip"]
        per["c5_over_c2"] = med["c5_fused_rows_skip"] / med["c2_embed_live_skip"]
        res[f"live_{f}"] = per
    return res


def run_grouped(dev, reps, B=256):
    """c2 at B = P x G = 64 x 4: the expanded keys / values against the one shared copy."""
    dec = RolloutDecoder(B, dev)
    dec.share_prompts(GROUP_G)
    patterns = {f: live_pattern(B, f, dev) for f in FRACTIONS}
    states, graphs = {}, {}
    with torch.no_grad():
        for r in GROUP_ROUTES:
            st = states[r] = dec.state()
            dec.token(st, r)                                      # warm-up
            torch.cuda.synchronize()
            st[0].reset()
            graphs[r] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[r]):                     # one stream, a linear chain of launches
                dec.token(st, r)
        # before anything is timed: the two record one rollout, bit for bit, at every live fraction
        for f in FRACTIONS:
            for r in GROUP_ROUTES:
                clock, _, rec, _ = states[r]
                clock.reset()
                rec.unfinished.copy_(patterns[f][0])
                for _ in range(T):
                    graphs[r].replay()
            torch.cuda.synchronize()
            a, b = (states[r][2] for r in GROUP_ROUTES)
            for field in ("tokens", "logprobs", "ref_logprobs"):
                x, y = getattr(a, field), getattr(b, field)
                assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                   y.view(torch.int32) if y.dtype == torch.float32 else y), (f, field)
        assert all(states[r][0].t == T and states[r][0].overrun == 0 for r in GROUP_ROUTES)
        keys = [(r, f) for r in GROUP_ROUTES for f in FRACTIONS]
        samples = {k: [] for k in keys}
        rng = random.Random(B + GROUP_G)
        for _ in range(reps):
            rng.shuffle(keys)
            for r, f in keys:
                clock, _, rec, _ = states[r]
                clock.reset()
                rec.unfinished.copy_(patterns[f][0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(T):
                    graphs[r].replay()
                e1.record()
                e1.synchronize()
                samples[(r, f)].append(e0.elapsed_time(e1) / T)
    nbytes = lambda kv: sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in kv)  # noqa: E731
    res = {"P": B // GROUP_G, "G": GROUP_G, "B": B,
           "the_two_routes_record_one_rollout_bit_for_bit_at_every_fraction": True,
           "kv_bytes_held": {"c2_expanded_G4": nbytes(dec.expanded_kv), "c2_grouped_G4": nbytes(dec.shared_kv)}}
    for f in FRACTIONS:
        per = {r: {"ms_per_token_median": statistics.median(samples[(r, f)]), "min": min(samples[(r, f)]),
                   "max": max(samples[(r, f)])} for r in GROUP_ROUTES}
        per["live_fraction_actual"] = patterns[f][1]
        per["grouped_over_expanded"] = per["c2_grouped_G4"]["ms_per_token_median"] / per["c2_expanded_G4"]["ms_per_token_median"]
        per["grouped_beats_expanded"] = per["grouped_over_expanded"] < 1.0
        res[f"live_{f}"] = per
    return res


# ------------------------------------------------------------------ the entries that existed before
def ab_child():
    """Per-call µs of trlx_t5_decode_attn (self, cross) and trlx_t5_decode_linear (norm -> qkv, M 8) on
    whatever library TRLX_T5_AMD_LIB names."""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:   # an older build lacks the newer entries
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
    k_enc = (torch.randn(B, NH, S, DKV, generator=g, device=dev) * DKV ** -0.25).to(DT)
    v_enc = torch.randn(B, NH, S, DKV, generator=g, device=dev).to(DT)
    mask = torch.ones(B, S, dtype=torch.int64, device=dev)
    mask[:, S - 37:] = 0

    def self_attn():
        P.t5_decode_self_attention(q, kn, vn, cache, t, table)

    def cross_attn():
        P.t5_decode_cross_attention(q, k_enc, v_enc, mask)

    h8 = torch.randn(8, D, generator=g, device=dev).to(DT)
    w_qkv = (torch.randn(3 * INNER, D, generator=g, device=dev) * D ** -0.5).to(DT)
    ln = (1.0 + 0.1 * torch.randn(D, generator=g, device=dev)).to(DT)
    o_qkv = torch.empty(8, 3 * INNER, dtype=DT, device=dev)

    def norm_qkv():
        P.t5_decode_linear(h8, w_qkv, norm_weight=ln, out=o_qkv)

    res = {}
    for name, fn in (("t5_decode_attn_self_B256_t47", self_attn), ("t5_decode_attn_cross_B256_S512", cross_attn),
                     ("t5_decode_linear_norm_qkv_M8", norm_qkv)):
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
    ap.add_argument("--only-grouped", action="store_true",
                    help="run the G 4 section alone and replace it in the --out file, keeping the file's other sections")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_rollout_bench.json"))
    args = ap.parse_args()
    if args.ab_child:
        return ab_child()
    result = {"tool": "tools/t5_rollout_bench.py",
              "shape": dict(L=L, n_heads=NH, d_kv=DKV, D=D, F=FF, V=V, S=S, T=T, dtype="bf16"),
              "timing": f"HIP events around whole {T}-token rollouts, (route, live fraction) pairs interleaved and "
                        f"shuffled per repetition, median of {args.reps}, ms per token"}
    if args.parent_lib:   # first: no GPU context in this process while the children run
        result["existing_entries_ab"] = existing_entries_ab(args.parent_lib)
        print(json.dumps(result["existing_entries_ab"]))
    dev = torch.device("cuda:0")
    if args.only_grouped:
        kept = json.load(open(args.out)) if os.path.exists(args.out) else {}
        result = {**kept, **{k: v for k, v in result.items() if k == "existing_entries_ab"}}
    result["device"] = torch.cuda.get_device_name(0)
    for B in (() if args.only_grouped else (int(b) for b in args.batches.split(","))):
        result[f"B{B}"] = run_shape(B, dev, args.reps)
        print(f"B {B}: " + json.dumps(result[f"B{B}"]))
    result["grouped_P64_G4"] = run_grouped(dev, args.reps)
    print("grouped P 64 x G 4: " + json.dumps(result["grouped_P64_G4"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
