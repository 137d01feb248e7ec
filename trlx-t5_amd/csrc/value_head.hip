// Fused bf16 value head (C ABI: trlx_value_head_fwd / trlx_value_head_bwd in
// include/trlx_t5_amd.h): values, and the head's own gradients, straight from the hidden states.
//
//   v_t = Σ_j relu(bf16(h_t·W1_j + b1_j)) · w2_j + b2      make_head(n_embd, 1), ppo_models.py:216-222
//
// h [N, ldh] bf16 (row-strided), W1 [2H, H] bf16 (nn.Linear layout), b1, w2 [2H], b2 [1] bf16.
//
//   k_vhead<false>   forward.  A workgroup (4 waves, 2 x 2) owns 64 tokens and a contiguous slice
//                    of the 2H columns, walked in 128-column chunks; per chunk the K = H loop runs
//                    in 32-deep steps through a 3-slot LDS ring filled by buffer-resource LDS DMA
//                    (64-B rows, chunk-XOR swizzled: the staging of k_lmhead_s2), 8
//                    v_mfma_f32_16x16x32_bf16 per wave and step.  The chunk's epilogue rounds
//                    z = acc + b1 to bf16 (where torch's bf16 Linear rounds it), applies the ReLU
//                    and folds z·w2 into one fp32 accumulator per token and lane; z never leaves
//                    the registers.  One fp32 partial per (column split, token); with one split
//                    the values are written directly.
//   k_vhead_combine  S > 1: sums the S partials of a token in split order, adds b2, rounds once.
//   k_vhead<true>    backward.  The same main loop recomputes the z tile; the epilogue writes
//                    dz = bf16(dv·w2·1[z > 0]) as [N, 2H] bf16 and, per 32-token half block, the
//                    fp32 column sums Σ_t dv_t·relu(z_tj) and Σ_t dz_tj.
//   k_vhead_bwd_reduce  adds the half blocks' column sums in block order -> dw2, db1; db2 = Σ dv.
//
// dh = dz·W1 and dW1 = dzᵀ·h are plain GEMMs and stay with the caller's BLAS.  No atomics; every
// sum has an order fixed by (N, H, S), whatever the rows' stride or alignment.
#include <algorithm>

#include "common.h"

namespace trlx {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kVhBM = 64, kVhBN = 128, kVhBK = 32;
constexpr int kVhStage = (kVhBM + kVhBN) * kVhBK * 2;  // 12 KB: 64 token rows + 128 W1 rows of 64 B
constexpr int kVhVec = 3 * kVhStage;                   // b1 / w2 of a chunk: [3 chunks][4 waves][b1 64 | w2 64] bf16
constexpr int kVhCmb = kVhVec + 3 * 4 * 256;           // the two column halves' token sums: [2][64] fp32
constexpr int kVhLds = kVhCmb + 2 * kVhBM * 4;
constexpr int kVhUnit = 32;                            // column granularity of a split
constexpr int kVhMaxSplits = 64;

struct VHeadArgs {
    const uint16_t* h;   // [N, H] rows of ldh elements
    const uint16_t* w1;  // [C, H] contiguous
    const uint16_t* b1;  // [C]
    const uint16_t* w2;  // [C]
    const uint16_t* b2;  // [1]
    int64_t ldh;
    int N, H, C, S, ntb;  // C = 2H columns, S column splits, ntb token blocks
    // forward
    float* part;          // [S, N] (S > 1)
    void* values;         // [N]
    int v_dtype;
    // backward
    const void* dv;       // [N]
    int dv_dtype;
    uint16_t* dz;         // [N, C]
    float* colpart;       // [2][2·ntb][C]: Σ dv·relu(z), then Σ dz
};

// 64-B rows: physical 16-B chunk c ^ ((r >> 2) & 3), as k_lmhead_s2 (a quarter-wave ds_read_b128
// of one logical chunk over 16 consecutive rows covers all 64 banks once).
__device__ __forceinline__ bf16x8_t vh_frag(const char* tile, int r, int c) {
    return *reinterpret_cast<const bf16x8_t*>(tile + r * 64 + ((c ^ ((r >> 2) & 3)) * 16));
}

// All-reduce over each 16-lane DPP row by four row_ror rotations (callers use lane 0 of the row).
template <int CTRL>
__device__ __forceinline__ float vh_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float vh_row16_sum(float v) {
    v += vh_dpp<0x128>(v);
    v += vh_dpp<0x124>(v);
    v += vh_dpp<0x122>(v);
    return v + vh_dpp<0x121>(v);
}

template <bool BWD>
__global__ __launch_bounds__(256) void k_vhead(VHeadArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kVhLds];  // ONE LDS object (LDS-DMA waits)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // token blocks fastest: consecutive workgroups share the W1 slice (it stays in L2)
    const int tb = int(blockIdx.x) % a.ntb, s = int(blockIdx.x) / a.ntb;
    const int m0 = tb * kVhBM;
    const int nrow = min(kVhBM, a.N - m0);  // valid tokens of the block (>= 1)
    const int nu = a.C / kVhUnit;
    const int c0 = int(int64_t(s) * nu / a.S) * kVhUnit, c1 = int(int64_t(s + 1) * nu / a.S) * kVhUnit;
    const int fr = lane & 15, fc = lane >> 4;

    // acc[i][j][q] at lane l = z(token m0 + wr*32 + i*16 + (l>>4)*4 + q, column chunk + wc*64 + j*16 + (l&15))
    float dvr[2][4];
    if constexpr (BWD) {  // before any LDS DMA (an ordinary load beside them drains the ring)
        // clamped loads and a select, the dtype test outside: a load under a per-element branch
        // is waited for alone
        uint32_t raw[2][4];
        if (a.dv_dtype == TRLX_BF16) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    raw[i][q] = uint32_t(static_cast<const uint16_t*>(
                                    a.dv)[min(m0 + wr * 32 + i * 16 + fc * 4 + q, a.N - 1)]) << 16;
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    raw[i][q] = static_cast<const uint32_t*>(a.dv)[min(m0 + wr * 32 + i * 16 + fc * 4 + q, a.N - 1)];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                dvr[i][q] = m0 + wr * 32 + i * 16 + fc * 4 + q < a.N ? __uint_as_float(raw[i][q]) : 0.f;
    }

    // DMA groups of 16 rows x 64 B per wave instruction: group `wave` of the token tile, groups
    // wave and wave + 4 of the W1 tile.  Lane l -> row l >> 2, physical chunk l & 3, fetching
    // the logical chunk of that slot.  Both resources end with the operand: the token rows are
    // clamped to the block's last valid one, the W1 rows to row C - 1 (their columns are masked
    // in the epilogue), so no lane's 16 bytes start outside h or W1 even at N = 1.
    const int rl = lane >> 2;
    const int lc = (lane & 3) ^ ((lane >> 4) & 3);
    const __amdgpu_buffer_rsrc_t rA =
        make_rsrc(a.h + int64_t(m0) * a.ldh, uint32_t((int64_t(nrow - 1) * a.ldh + a.H) * 2));
    const __amdgpu_buffer_rsrc_t rB = make_rsrc(a.w1, uint32_t(int64_t(a.C) * a.H * 2));
    const int voffA = (min(wave * 16 + rl, nrow - 1) * int(a.ldh) + lc * 8) * 2;
    const int nk = a.H / kVhBK;
    const int nchunk = (c1 - c0 + kVhBN - 1) / kVhBN;
    const int total = nchunk * nk;
    // b1 / w2 of a chunk travel by LDS DMA too (an ordinary load beside the ring would be waited
    // for with vmcnt(0)): one 4-byte DMA per wave with a chunk's first K step, lanes 0..31 the
    // wave's 64 b1 columns in pairs, lanes 32..63 its w2 columns (pairs clamped to C - 2; the
    // columns past the slice are masked).  Slot = chunk mod 3: at most the next two chunks'
    // vectors are in flight while a chunk's own are still to be read.
    const uint16_t* vsrc = lane < 32 ? a.b1 : a.w2;
    int ich = 0, ikt = 0, islot = 0, ivs = 0;  // the next step to issue: chunk, K step, ring slot, vector slot
    auto issue = [&]() {
        char* stage = smem + islot * kVhStage;
        const int soff = ikt * kVhBK * 2;
        if (ikt == 0) {
            const int col = min(c0 + ich * kVhBN + wc * 64 + (lane & 31) * 2, a.C - 2);
            __builtin_amdgcn_global_load_lds(
                vsrc + col, (__attribute__((address_space(3))) void*)(smem + kVhVec + (ivs * 4 + wave) * 256), 4, 0, 0);
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)(stage + wave * 1024),
                                                 16, voffA, soff, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int g = i * 4 + wave;
            const int col = min(c0 + ich * kVhBN + g * 16 + rl, a.C - 1);
            const int voffB = (col * a.H + lc * 8) * 2;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rB, (__attribute__((address_space(3))) void*)(stage + kVhBM * 64 + g * 1024), 16, voffB, soff, 0, 0);
        }
        islot = islot == 2 ? 0 : islot + 1;
        if (++ikt == nk) {
            ikt = 0;
            ++ich;
            ivs = ivs == 2 ? 0 : ivs + 1;
        }
    };

    f32x4_t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float vacc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) vacc[i][q] = 0.f;
    // K loop over the flattened (chunk, K step) sequence, one raw barrier per step: retire step
    // st (own vmcnt, leaving at most the three tile DMAs of st + 1 in flight; then the barrier:
    // every wave's part landed AND every wave is done reading st - 1), issue st + 2 into
    // st - 1's slot, read, 8 MFMAs.
    issue();
    if (total > 1) issue();
    int ch = 0, kt = 0, slot = 0, vs = 0;
    for (int st = 0; st < total; ++st) {
        if (st + 1 < total)
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (st + 2 < total) issue();
        const char* At = smem + slot * kVhStage;
        const char* Bt = At + kVhBM * 64;
        bf16x8_t af[2], bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = vh_frag(Bt, wc * 64 + j * 16 + fr, fc);
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = vh_frag(At, wr * 32 + i * 16 + fr, fc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        slot = slot == 2 ? 0 : slot + 1;
        if (++kt < nk) continue;

        // ---- the chunk's epilogue: z rounded to bf16 after the bias, ReLU, second contraction
        const int cb = c0 + ch * kVhBN + wc * 64 + fr;  // this lane's column j = 0 of the chunk
        const uint16_t* vec = reinterpret_cast<const uint16_t*>(smem + kVhVec + (vs * 4 + wave) * 256);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = cb + j * 16;
            const bool ok = col < c1;
            const float b1j = ok ? bf2f(vec[j * 16 + fr]) : 0.f;
            const float w2j = ok ? bf2f(vec[64 + j * 16 + fr]) : 0.f;
            float sw = 0.f, sb = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float zb = bf2f(f2bf(add_rn(acc[i][j][q], b1j)));
                    const float r = zb < 0.f ? 0.f : zb;  // NaN stays NaN, as torch's relu
                    if constexpr (!BWD) {
                        vacc[i][q] = fmaf(ok ? r : 0.f, w2j, vacc[i][q]);
                    } else {
                        const int t = m0 + wr * 32 + i * 16 + fc * 4 + q;
                        if (ok && t < a.N) {
                            const uint16_t g = zb > 0.f ? f2bf(mul_rn(dvr[i][q], w2j)) : uint16_t(0);
                            a.dz[int64_t(t) * a.C + col] = g;
                            sw = fmaf(dvr[i][q], r, sw);
                            sb = add_rn(sb, bf2f(g));
                        }
                    }
                }
            if constexpr (BWD) {  // the four 4-token groups of the wave's 32 tokens
                sw += __shfl_xor(sw, 16, kWave);
                sw += __shfl_xor(sw, 32, kWave);
                sb += __shfl_xor(sb, 16, kWave);
                sb += __shfl_xor(sb, 32, kWave);
                if (fc == 0 && ok) {
                    const int64_t pb = int64_t(tb) * 2 + wr;
                    a.colpart[pb * a.C + col] = sw;
                    a.colpart[(int64_t(a.ntb) * 2 + pb) * a.C + col] = sb;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        kt = 0;
        ++ch;
        vs = vs == 2 ? 0 : vs + 1;
    }

    if constexpr (!BWD) {
        // per token: the 16 column lanes, then the two column halves of the workgroup, in order
        float* cmb = reinterpret_cast<float*>(smem + kVhCmb);  // [2][64]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = vh_row16_sum(vacc[i][q]);
                if (fr == 0) cmb[wc * kVhBM + wr * 32 + i * 16 + fc * 4 + q] = v;
            }
        __syncthreads();
        if (tid < nrow) {
            const float p = add_rn(cmb[tid], cmb[kVhBM + tid]);
            if (a.S == 1)
                st_any(a.values, a.v_dtype, m0 + tid, add_rn(p, bf2f(a.b2[0])));
            else
                a.part[int64_t(s) * a.N + m0 + tid] = p;
        }
    }
}

__global__ __launch_bounds__(256) void k_vhead_combine(VHeadArgs a) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= a.N) return;
    float v = a.part[t];
    for (int s = 1; s < a.S; ++s) v = add_rn(v, a.part[int64_t(s) * a.N + t]);
    st_any(a.values, a.v_dtype, t, add_rn(v, bf2f(a.b2[0])));
}

// Blocks 0 .. ceil(C/256)-1: one column per thread, the 2·ntb half-block sums in block order;
// the last block: db2 = Σ_t dv_t (strided per thread, then the fixed block order).
__global__ __launch_bounds__(256) void k_vhead_bwd_reduce(VHeadArgs a, void* dw2, void* db1, void* db2,
                                                           int g_dtype) {
    __shared__ float sh[4];
    if (blockIdx.x == gridDim.x - 1) {
        float sv = 0.f;
        for (int t = threadIdx.x; t < a.N; t += 256) sv = add_rn(sv, ld_any(a.dv, a.dv_dtype, t));
        sv = block_sum(sv, sh);
        if (threadIdx.x == 0) st_any(db2, g_dtype, 0, sv);
        return;
    }
    const int col = int(blockIdx.x) * 256 + threadIdx.x;
    if (col >= a.C) return;
    const int np = a.ntb * 2;
    const float* pw = a.colpart + col;
    const float* pb = a.colpart + int64_t(np) * a.C + col;
    float sw = 0.f, sb = 0.f;  // (a half block without a valid token wrote zeros)
    for (int p = 0; p < np; ++p) {
        sw = add_rn(sw, pw[int64_t(p) * a.C]);
        sb = add_rn(sb, pb[int64_t(p) * a.C]);
    }
    st_any(dw2, g_dtype, col, sw);
    st_any(db1, g_dtype, col, sb);
}

static TuneKnob g_vh_splits{0};  // tuning "vhead_splits" (0 = auto)

int vhead_set_tuning(const char* key, int64_t value, bool* handled) {
    *handled = key && !__builtin_strcmp(key, "vhead_splits");
    if (!*handled) return TRLX_OK;
    TRLX_REQUIRE(value >= 0 && value <= kVhMaxSplits, TRLX_ERR_ARG, "vhead_splits: 0 auto, 1..%d", kVhMaxSplits);
    g_vh_splits = int(value);
    return TRLX_OK;
}

static int vh_ncu() {
    static thread_local int dev = -1, ncu = 0;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return 256;
    if (d != dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
        dev = d;
        ncu = n;
    }
    return ncu;
}

static bool vh_shape_ok(int64_t N, int64_t H) {
    return H >= 32 && H <= 8192 && H % 32 == 0 && N >= 1 && N <= (int64_t(1) << 30);
}
static int vh_max_splits(int64_t H) { return int(std::min<int64_t>(2 * H / kVhUnit, kVhMaxSplits)); }
static int64_t vh_blocks(int64_t N) { return (N + kVhBM - 1) / kVhBM; }
// Column splits: enough workgroups for every compute unit once, at most one per 32 columns.
static int vh_splits(int64_t N, int64_t H) {
    const int forced = g_vh_splits;
    const int64_t ntb = vh_blocks(N);
    const int64_t want = forced ? forced : (vh_ncu() + ntb - 1) / ntb;
    return int(std::max<int64_t>(1, std::min<int64_t>(want, vh_max_splits(H))));
}

static int vh_common(VHeadArgs& a, const void* h, int64_t ldh, const void* w1, const void* b1, const void* w2,
                     int64_t N, int64_t H) {
    TRLX_REQUIRE(vh_shape_ok(N, H), TRLX_ERR_SHAPE,
                 "value head: N=%lld H=%lld (N >= 1, 32 <= H <= 8192, H a multiple of 32)", (long long)N,
                 (long long)H);
    TRLX_REQUIRE(h && w1 && b1 && w2, TRLX_ERR_ARG, "value head: NULL h / W1 / b1 / w2");
    if (N == 1) ldh = H;
    TRLX_REQUIRE(ldh >= H && ldh % 8 == 0 && ldh <= (int64_t(1) << 24), TRLX_ERR_STRIDE,
                 "value head: row stride %lld (>= H, a multiple of 8 elements, <= 2^24)", (long long)ldh);
    TRLX_REQUIRE(((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w1)) & 15u) == 0, TRLX_ERR_ARG,
                 "value head: h and W1 must be 16-byte aligned");
    TRLX_REQUIRE(((reinterpret_cast<uintptr_t>(b1) | reinterpret_cast<uintptr_t>(w2)) & 3u) == 0, TRLX_ERR_ARG,
                 "value head: b1 and w2 must be 4-byte aligned");
    a.h = static_cast<const uint16_t*>(h);
    a.w1 = static_cast<const uint16_t*>(w1);
    a.b1 = static_cast<const uint16_t*>(b1);
    a.w2 = static_cast<const uint16_t*>(w2);
    a.ldh = ldh;
    a.N = int(N);
    a.H = int(H);
    a.C = int(2 * H);
    a.ntb = int(vh_blocks(N));
    a.S = vh_splits(N, H);
    TRLX_REQUIRE(int64_t(a.ntb) * a.S <= 0x7fffffffLL, TRLX_ERR_SHAPE, "value head: too many tokens");
    return TRLX_OK;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_value_head_splits(int64_t N, int64_t H) { return vh_shape_ok(N, H) ? vh_splits(N, H) : 0; }

extern "C" int64_t trlx_value_head_workspace_bytes(int64_t N, int64_t H) {
    return vh_shape_ok(N, H) ? int64_t(vh_max_splits(H)) * N * 4 : 0;
}

extern "C" int64_t trlx_value_head_bwd_workspace_bytes(int64_t N, int64_t H) {
    return vh_shape_ok(N, H) ? 2 * (2 * vh_blocks(N)) * (2 * H) * 4 : 0;
}

extern "C" int trlx_value_head_fwd(const void* h, int64_t ldh, const void* w1, const void* b1, const void* w2,
                                   const void* b2, int64_t N, int64_t H, void* values, int values_dtype,
                                   void* workspace, void* stream) {
    VHeadArgs a = {};
    const int rc = vh_common(a, h, ldh, w1, b1, w2, N, H);
    if (rc) return rc;
    TRLX_REQUIRE(values_dtype == TRLX_F32 || values_dtype == TRLX_BF16, TRLX_ERR_DTYPE, "values dtype %d",
                 values_dtype);
    TRLX_REQUIRE(b2 && values, TRLX_ERR_ARG, "value head: NULL b2 / values");
    TRLX_REQUIRE(a.S == 1 || workspace, TRLX_ERR_ARG, "value head: NULL workspace with %d column splits", a.S);
    a.b2 = static_cast<const uint16_t*>(b2);
    a.part = static_cast<float*>(workspace);
    a.values = values;
    a.v_dtype = values_dtype;
    hipLaunchKernelGGL(k_vhead<false>, dim3(unsigned(a.ntb * a.S)), dim3(256), 0, (hipStream_t)stream, a);
    int lrc = check_launch("k_vhead_fwd");
    if (lrc || a.S == 1) return lrc;
    hipLaunchKernelGGL(k_vhead_combine, dim3(unsigned((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("k_vhead_combine");
}

extern "C" int trlx_value_head_bwd(const void* h, int64_t ldh, const void* w1, const void* b1, const void* w2,
                                   const void* dv, int dv_dtype, int64_t N, int64_t H, void* dz, void* dw2,
                                   void* db1, void* db2, int grad_dtype, void* workspace, void* stream) {
    VHeadArgs a = {};
    const int rc = vh_common(a, h, ldh, w1, b1, w2, N, H);
    if (rc) return rc;
    TRLX_REQUIRE((dv_dtype == TRLX_F32 || dv_dtype == TRLX_BF16) && (grad_dtype == TRLX_F32 || grad_dtype == TRLX_BF16),
                 TRLX_ERR_DTYPE, "value head backward: dv dtype %d, gradient dtype %d", dv_dtype, grad_dtype);
    TRLX_REQUIRE(dv && dz && dw2 && db1 && db2 && workspace, TRLX_ERR_ARG,
                 "value head backward: NULL dv / dz / dw2 / db1 / db2 / workspace");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(dz) & 1u) == 0 &&
                     (reinterpret_cast<uintptr_t>(dv) & (dv_dtype == TRLX_BF16 ? 1u : 3u)) == 0 &&
                     (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
                 TRLX_ERR_ARG, "value head backward: dv / dz / workspace not aligned to their element size");
    a.dv = dv;
    a.dv_dtype = dv_dtype;
    a.dz = static_cast<uint16_t*>(dz);
    a.colpart = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_vhead<true>, dim3(unsigned(a.ntb * a.S)), dim3(256), 0, (hipStream_t)stream, a);
    const int lrc = check_launch("k_vhead_bwd");
    if (lrc) return lrc;
    hipLaunchKernelGGL(k_vhead_bwd_reduce, dim3(unsigned((a.C + 255) / 256 + 1)), dim3(256), 0, (hipStream_t)stream,
                       a, dw2, db1, db2, grad_dtype);
    return check_launch("k_vhead_bwd_reduce");
}
