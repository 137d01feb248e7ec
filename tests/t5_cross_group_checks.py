"""The shared cases of the grouped decode cross-attention (trlx_t5_decode_attn_group,
csrc/t5_decode_attn_group.hip; tests/test_t5_cross_group_cpu.py, tests/test_gpu_t5_cross_group.py).

A case is cross_case of t5_decode_attn_checks read as P = 3 prompts with nH = 5 heads — its K, V
[P, nH, S, d] and its mask [P, S], per prompt — and a q of P * G rows of its own: seeded N(0, 1)
times d_kv^-1/4, the scale cross_case gives its q, so that q.k ~ N(0, 1).  Row p * G + g is sample g
of prompt p, so the tensors the existing kernel needs are repeat_interleave(G, 0) of K, V and mask.

  GS            both sides of each built query tile (1, 2, 4, 8) and remainder tiles (3, 5, 9)
  groups        NG of the kernel's geometry for a (dtype, d_kv)
  cross_s       CROSS_S of t5_decode_attn_checks plus both sides of one and of two rounds of the
                groups: NG - 1, NG, NG + 1, 2 NG - 1, 2 NG, 2 NG + 1
  live_sets     all live, all dead, one whole prompt dead, alternating, only the last row of each
                prompt live (the last row of a remainder tile when G is no multiple of the tile)

Test infrastructure only."""
import torch

import t5_decode_attn_checks as A

P, NH = A.B, A.NH
GS = (1, 2, 3, 4, 5, 8, 9)
TILES = (1, 2, 4, 8)


def groups(dtype, d_kv):
    """NG = 4 waves * (64 lanes / lanes per key row); a lane holds one 16-byte vector of the row."""
    epv = 8 if dtype == torch.bfloat16 else 4
    return 4 * (64 // (d_kv // epv))


def cross_s(dtype, d_kv):
    ng = groups(dtype, d_kv)
    return tuple(sorted(set(A.CROSS_S) | {ng - 1, ng, ng + 1, 2 * ng - 1, 2 * ng, 2 * ng + 1}))


def group_q(dtype, d_kv, S, kind, G):
    """q [P * G, nH * d] for the case (dtype, d_kv, S, kind) at G samples per prompt."""
    g = torch.Generator().manual_seed(9000 + 131 * G + 13 * S + d_kv + (7 if dtype == torch.float32 else 0)
                                      + A.MASKS.index(kind))
    return (torch.randn(P * G, NH * d_kv, generator=g) * d_kv ** -0.25).to(dtype)


def group_case(dtype, d_kv, S, kind, G):
    """dict(q [P*G, nH*d], K, V [P, nH, S, d], mask [P, S] or None), on the CPU."""
    c = A.cross_case(dtype, d_kv, S, kind)
    return dict(q=group_q(dtype, d_kv, S, kind, G), K=c["K"], V=c["V"], mask=c["mask"])


def expand(x, G):
    """What the existing kernel is fed: every prompt's rows G times, contiguous."""
    return None if x is None else x.repeat_interleave(G, 0).contiguous()


def live_sets(G):
    """name -> int64 [P * G] on the CPU."""
    n = P * G
    one_prompt = torch.ones(n, dtype=torch.int64)
    one_prompt[G:2 * G] = 0
    last = torch.zeros(n, dtype=torch.int64)
    last[G - 1::G] = 3
    return {"all_live": torch.ones(n, dtype=torch.int64), "all_dead": torch.zeros(n, dtype=torch.int64),
            "one_prompt_dead": one_prompt, "alternating": (torch.arange(n) % 2 == 0).to(torch.int64),
            "last_row_of_each_prompt": last}
