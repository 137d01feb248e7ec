// Host only: the checks of a TrlxT5DecodeAttnGroupArgs, which trlx_t5_decode_attn_group,
// trlx_t5_decode_attn_group_mma, trlx_t5_decode_attn_split and trlx_t5_decode_attn_group_d256 take alike.  Defined in
// t5_decode_attn_group.hip.
#pragma once

#include "common.h"

namespace trlx {

struct T5GroupChecked {
    int64_t ldq;      // the q row stride; a single row has none to speak of
    int64_t st[6];    // K then V over (p, h, s); a dimension of size 1 has no stride to speak of
    int gt;           // queries a tile
    int64_t tiles;    // ceil(G / gt)
};

// the cap trlx_t5_decode_attn_group_tile set, or the default
int t5_group_tile_cap();
// the built tile the grouped and split entries take for G under that cap
int t5_group_tile(int64_t G);

// Everything the entries refuse, in one order; `who` opens the messages.  f32_ok: fp32 is
// taken besides bf16.  rows_by_heads: P * G * heads must fit 32 bits too (the split entry's merge
// grid).  tile: the entry's fixed query tile, or 0 for t5_group_tile(G).  d_only: the one d_kv the
// entry takes, or 0 for 64 and 128.
int t5_group_check(const TrlxT5DecodeAttnGroupArgs* a, const char* who, bool f32_ok, bool rows_by_heads, int tile,
                   T5GroupChecked* c, int64_t d_only = 0);

}  // namespace trlx
