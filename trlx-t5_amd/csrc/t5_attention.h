// What the T5 full-sequence attention forward (t5_attention.hip) and backward
// (t5_attention_bwd.hip) share: the flag bits, the MFMA operand types, the transposed LDS read and
// the host-side operand checks.
#pragma once

#include <utility>

#include "common.h"

namespace trlx {

enum { kTaBias = 1, kTaMask = 2, kTaCausal = 4 };

typedef __bf16 ta_bf16x8 __attribute__((ext_vector_type(8)));
typedef short ta_s16x4 __attribute__((ext_vector_type(4)));
typedef float ta_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ ta_s16x4 ta_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) ta_s16x4*)(p));
}

// The A operand of a 32x32x16 MFMA whose 32 rows are COLUMNS of a row-major LDS tile (V^T from V,
// K^T from K, Q^T from Q, dO^T from dO) and whose 16 k-indices are tile rows in the permuted order
// the B operand has them in a 32x32 result's registers (row (j & 3) + 8 (j >> 2) + 4 (lane >> 5) of
// the 16).  Lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of a 4-row x
// 16-column block and receives its column (lane & 15) of the 4 rows.  `p0`: ta_tr_base(...) moved
// to the first of the 16 tile rows and to the 32-column block.  The forward (t5_attention.hip, the
// O^T += V^T·P^T loop) carries the same address arithmetic inline, from before these helpers: it was
// left as it is so that its instantiations compile to the code they had; a change to the layout has
// to be made in both places.
__device__ __forceinline__ const unsigned char* ta_tr_base(const unsigned char* tile, int stride, int lane) {
    return tile + (4 * (lane >> 5) + ((lane & 15) >> 2)) * stride + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
}
__device__ __forceinline__ ta_bf16x8 ta_tr_frag(const unsigned char* p0, int stride) {
    const ta_s16x4 v0 = ta_tr_read(p0), v1 = ta_tr_read(p0 + 8 * stride);
    return __builtin_bit_cast(ta_bf16x8, __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7));
}

static inline bool ta_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one operand's strides: whole 16-byte vectors, rows of d_kv elements that do not overlap, and the
// last element's offset (returned through *span) within the kernel's int64 arithmetic
static inline bool ta_strides_ok(int64_t B, int64_t T, int64_t nH, int64_t d, int64_t sb, int64_t st, int64_t sh,
                                 bool dense, int64_t* span) {
    const int64_t n[3] = {B, T, nH};
    const int64_t s[3] = {sb, st, sh};
    int64_t total = d - 1;
    for (int i = 0; i < 3; ++i) {
        if (n[i] == 1) continue;   // a single index has no stride to speak of
        if (s[i] % 8 != 0 || s[i] < 0) return false;
        if (i > 0 && s[i] < d) return false;
        int64_t ext;
        if (__builtin_mul_overflow(n[i] - 1, s[i], &ext) || __builtin_add_overflow(total, ext, &total)) return false;
    }
    if (total > (int64_t(1) << 61)) return false;
    if (dense) {   // written: no two (b, t, h) rows may share an element
        int order[3] = {0, 1, 2};
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 3; ++j)
                if (s[order[j]] < s[order[i]]) std::swap(order[i], order[j]);
        int64_t need = d;
        for (int i = 0; i < 3; ++i) {
            const int x = order[i];
            if (n[x] == 1) continue;
            if (s[x] < need) return false;
            need = s[x] * n[x];
        }
    }
    *span = total;
    return true;
}

}  // namespace trlx
