// The fp8 quantiser of the encoder's keys and values for the decode cross-attention: one launch
// per layer and rollout, K and V in the same launch, one workgroup per (batch row, head).  See
// trlx_t5_cross_kv_quantize in trlx_t5_amd.h; the reader is k_t5_decode_attn_kv8, further down.
//
// Two passes over the (b, h) block.  Pass 1: the largest |x| over the live keys, as the maximum of
// the bf16 bit patterns with the sign cleared (an integer maximum: exact, order-free, and a
// non-finite element is any pattern >= 0x7f80).  From it the power-of-two scale 2^e.  Pass 2: each
// lane reads one 16-byte vector of 8 bf16 again (the block is cache-resident by then), multiplies
// by 2^-e (exact in fp32), rounds to e4m3fn in integer arithmetic and stores 8 bytes.  The
// rounding restates torch's cast (c10 fp8e4m3fn_from_fp32_value) step for step, so the bytes are
// torch's for every input, ties and subnormals included; v_cvt_pk_fp8_f32 is not used.
#include "common.h"

namespace trlx {

constexpr int kQ8Threads = 256;
constexpr int kQ8Waves = kQ8Threads / kWave;

struct Q8Args {
    const uint16_t* k;
    const uint16_t* v;
    const int64_t* mask;   // [B, S] or NULL
    uint8_t* k8;
    uint8_t* v8;
    float* k_scale;
    float* v_scale;
    int64_t k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
    int nH, S;
};

// fp32 -> e4m3fn byte, round to nearest even; at or above 480 (and NaN) -> 0x7f.  torch's cast.
__device__ __forceinline__ uint32_t f32_to_e4m3fn(float f) {
    uint32_t b = __float_as_uint(f);
    const uint32_t sign = b & 0x80000000u;
    b ^= sign;
    uint32_t r;
    if (b >= (1087u << 20)) {
        r = 0x7fu;
    } else if (b < (121u << 23)) {   // below 2^-6: the subnormals, rounded by an fp32 add
        const uint32_t magic = 141u << 23;
        r = __float_as_uint(__fadd_rn(__uint_as_float(b), __uint_as_float(magic))) - magic;
    } else {
        const uint32_t odd = (b >> 20) & 1u;
        b += (uint32_t(7 - 127) << 23) + 0x7ffffu;
        b += odd;
        r = b >> 20;
    }
    return (r | (sign >> 24)) & 0xffu;
}

// the exponent e of the scale from the bf16 pattern of amax (finite): the smallest e with
// amax * 2^-e <= 448, 0 for amax == 0, clamped to [-100, 119]
__device__ __forceinline__ int q8_exponent(uint32_t amax_bits) {
    if (amax_bits == 0) return 0;
    const int E = int(amax_bits >> 7), M = int(amax_bits & 0x7fu);
    if (E == 0) return -100;                       // a bf16 subnormal: far below the clamp
    const int e = (E - 126) - (M <= 96 ? 9 : 8);   // frexp: m = (1 + M / 128) / 2 <= 0.875 iff M <= 96
    return e < -100 ? -100 : e > 119 ? 119 : e;
}

__device__ __forceinline__ uint32_t q8_absmax(const vec4u& x, uint32_t m) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m = max(m, w[i] & 0x7fffu);
        m = max(m, (w[i] >> 16) & 0x7fffu);
    }
    return m;
}

__device__ __forceinline__ uint32_t q8_pack4(uint32_t lo, uint32_t hi, float inv) {
    return f32_to_e4m3fn(__fmul_rn(bf_lo(lo), inv)) | (f32_to_e4m3fn(__fmul_rn(bf_hi(lo), inv)) << 8) |
           (f32_to_e4m3fn(__fmul_rn(bf_lo(hi), inv)) << 16) | (f32_to_e4m3fn(__fmul_rn(bf_hi(hi), inv)) << 24);
}

template <int DKV>
__global__ __launch_bounds__(kQ8Threads) void k_t5_cross_kv_quantize(const Q8Args a) {
    constexpr int VPR = DKV / 8;   // 16-byte vectors per key row
    __shared__ uint32_t s_max[2 * kQ8Waves];

    const int bh = blockIdx.x;
    const int b = bh / a.nH, h = bh - b * a.nH;
    const uint16_t* K = a.k + int64_t(b) * a.k_sb + int64_t(h) * a.k_sh;
    const uint16_t* V = a.v + int64_t(b) * a.v_sb + int64_t(h) * a.v_sh;
    const int64_t* mask = a.mask ? a.mask + int64_t(b) * a.S : nullptr;
    const int nvec = a.S * VPR;    // S <= 2^31 / 128

    uint32_t mk = 0, mv = 0;
#pragma unroll 1
    for (int i = threadIdx.x; i < nvec; i += kQ8Threads) {
        const int row = i / VPR, c = (i - row * VPR) * 8;
        if (mask && mask[row] == 0) continue;   // a masked row is not read
        mk = q8_absmax(*reinterpret_cast<const vec4u*>(K + int64_t(row) * a.k_ss + c), mk);
        mv = q8_absmax(*reinterpret_cast<const vec4u*>(V + int64_t(row) * a.v_ss + c), mv);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mk = max(mk, uint32_t(__shfl_xor(int(mk), off, kWave)));
        mv = max(mv, uint32_t(__shfl_xor(int(mv), off, kWave)));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_max[threadIdx.x / kWave] = mk;
        s_max[kQ8Waves + threadIdx.x / kWave] = mv;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kQ8Waves; ++w) {
        mk = max(mk, s_max[w]);
        mv = max(mv, s_max[kQ8Waves + w]);
    }
    // a live Inf / NaN: the scale is NaN and every live byte of that tensor's block is the NaN byte
    const bool bad_k = mk >= 0x7f80u, bad_v = mv >= 0x7f80u;
    const int ek = bad_k ? 0 : q8_exponent(mk), ev = bad_v ? 0 : q8_exponent(mv);
    const float inv_k = __uint_as_float(uint32_t(127 - ek) << 23), inv_v = __uint_as_float(uint32_t(127 - ev) << 23);
    if (threadIdx.x == 0) {
        a.k_scale[bh] = bad_k ? __uint_as_float(0x7fc00000u) : __uint_as_float(uint32_t(127 + ek) << 23);
        a.v_scale[bh] = bad_v ? __uint_as_float(0x7fc00000u) : __uint_as_float(uint32_t(127 + ev) << 23);
    }

    uint8_t* K8 = a.k8 + int64_t(bh) * a.S * DKV;
    uint8_t* V8 = a.v8 + int64_t(bh) * a.S * DKV;
#pragma unroll 1
    for (int i = threadIdx.x; i < nvec; i += kQ8Threads) {
        const int row = i / VPR, c = (i - row * VPR) * 8;
        uint2 ok = make_uint2(0u, 0u), ov = ok;   // a masked row: zero bytes
        if (!mask || mask[row] != 0) {
            const vec4u x = *reinterpret_cast<const vec4u*>(K + int64_t(row) * a.k_ss + c);
            const vec4u y = *reinterpret_cast<const vec4u*>(V + int64_t(row) * a.v_ss + c);
            ok = bad_k ? make_uint2(0x7f7f7f7fu, 0x7f7f7f7fu) : make_uint2(q8_pack4(x.x, x.y, inv_k), q8_pack4(x.z, x.w, inv_k));
            ov = bad_v ? make_uint2(0x7f7f7f7fu, 0x7f7f7f7fu) : make_uint2(q8_pack4(y.x, y.y, inv_v), q8_pack4(y.z, y.w, inv_v));
        }
        const int64_t o = int64_t(row) * DKV + c;
        *reinterpret_cast<uint2*>(K8 + o) = ok;
        *reinterpret_cast<uint2*>(V8 + o) = ov;
    }
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_cross_kv_quantize(const TrlxT5CrossKvQuantArgs* a, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 cross kv quantize: NULL arguments");
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 cross kv quantize: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(a->B >= 1 && a->n_heads >= 1 && a->S >= 1 && a->B * a->n_heads <= 0x7fffffffLL &&
                     a->S <= 0x7fffffffLL / 128 && a->n_heads <= 0x7fffffffLL / 128,
                 TRLX_ERR_ARG, "t5 cross kv quantize: B %lld, heads %lld, S %lld", (long long)a->B,
                 (long long)a->n_heads, (long long)a->S);
    TRLX_REQUIRE(a->k && a->v && a->k8 && a->v8 && a->k_scale && a->v_scale, TRLX_ERR_ARG,
                 "t5 cross kv quantize: NULL k / v / k8 / v8 / k_scale / v_scale");
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(a->k, 15) && !mis(a->v, 15) && !mis(a->k8, 15) && !mis(a->v8, 15), TRLX_ERR_ARG,
                 "t5 cross kv quantize: k, v, k8 and v8 must be 16-byte aligned");
    TRLX_REQUIRE(!mis(a->k_scale, 3) && !mis(a->v_scale, 3) && !mis(a->key_mask, 7), TRLX_ERR_ARG,
                 "t5 cross kv quantize: scales not aligned to 4 bytes or key_mask not aligned to 8");
    // a dimension of size 1 has no stride to speak of
    const int64_t st[6] = {a->B > 1 ? a->k_stride_b : 0, a->n_heads > 1 ? a->k_stride_h : 0, a->S > 1 ? a->k_stride_s : 0,
                           a->B > 1 ? a->v_stride_b : 0, a->n_heads > 1 ? a->v_stride_h : 0, a->S > 1 ? a->v_stride_s : 0};
    for (int i = 0; i < 6; ++i)
        TRLX_REQUIRE(st[i] >= 0 && st[i] % 8 == 0, TRLX_ERR_ARG,
                     "t5 cross kv quantize: stride %lld (non-negative, whole 16-byte vectors)", (long long)st[i]);
    TRLX_REQUIRE((a->S == 1 || (st[2] >= a->d_kv && st[5] >= a->d_kv)) && (a->n_heads == 1 || (st[1] >= a->d_kv && st[4] >= a->d_kv)),
                 TRLX_ERR_ARG, "t5 cross kv quantize: key and head strides must be at least d_kv");
    Q8Args q = {};
    q.k = static_cast<const uint16_t*>(a->k);
    q.v = static_cast<const uint16_t*>(a->v);
    q.mask = a->key_mask;
    q.k8 = static_cast<uint8_t*>(a->k8);
    q.v8 = static_cast<uint8_t*>(a->v8);
    q.k_scale = a->k_scale;
    q.v_scale = a->v_scale;
    q.k_sb = st[0], q.k_sh = st[1], q.k_ss = st[2];
    q.v_sb = st[3], q.v_sh = st[4], q.v_ss = st[5];
    q.nH = int(a->n_heads);
    q.S = int(a->S);
    hipLaunchKernelGGL(a->d_kv == 64 ? k_t5_cross_kv_quantize<64> : k_t5_cross_kv_quantize<128>,
                       dim3(unsigned(a->B * a->n_heads)), dim3(kQ8Threads), 0, (hipStream_t)stream, q);
    return check_launch("k_t5_cross_kv_quantize");
}

// ---------------------------------------------------------------- fp8 encoder keys / values
// trlx_t5_decode_attn_kv8: the cross step over the bytes of trlx_t5_cross_kv_quantize (e4m3fn, one
// power-of-two scale per (b, h) and tensor).  A 16-byte vector is 16 elements, so a key row takes
// LPR = d_kv / 16 lanes (4 at d_kv 64, 8 at 128), a wave-wide load covers KPW = 64 / LPR rows (16 /
// 8) and the workgroup has NG = 4 * KPW groups (64 / 32).  Each group keeps kKv8Flight = 4 columns
// in flight (4 x 2 x 16 B, twice the bf16 kernel's bytes), so one trip of the loop covers 4 * NG
// columns (256 / 128).  The bytes are converted to fp32 two at a time in hardware
// (v_cvt_pk_f32_fp8); the arithmetic is the bf16 kernel's: fp32 dot, butterfly inside the group,
// times k_scale, online fp32 softmax, fp32 P·V; v_scale multiplies at the merge, before the
// division and the one rounding.  Same fixed merge order.  Kernels and an argument block of their
// own in a translation unit of their own: t5_decode_attn.hip and its code object are as they were.
constexpr int kKv8Flight = 4;
constexpr int kT5Threads = 256;   // as in t5_decode_attn.hip
constexpr int kT5Waves = kT5Threads / kWave;

struct T5AttnKv8Args {
    const void* q;
    const void* k;          // bytes
    const void* v;
    const int64_t* mask;    // [B, max_len] or NULL
    void* out;
    int64_t ldq;
    int nH, max_len;
    const float* k_scale;   // [B, nH]
    const float* v_scale;   // [B, nH]
    const int64_t* live;    // [B] or NULL (LIVE = false)
};

__device__ __forceinline__ void kv8_unpack(const vec4u& v, float (&f)[16]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(int(w[i]), false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(int(w[i]), true);
        f[4 * i] = lo[0];
        f[4 * i + 1] = lo[1];
        f[4 * i + 2] = hi[0];
        f[4 * i + 3] = hi[1];
    }
}

template <int DKV, bool MASKED, bool LIVE>
__global__ __launch_bounds__(kT5Threads) void k_t5_decode_attn_kv8(const T5AttnKv8Args args) {
    const T5AttnKv8Args& a = args;
    constexpr int EPV = 16;
    constexpr int LPR = DKV / EPV;
    constexpr int KPW = kWave / LPR;
    constexpr int NG = kT5Waves * KPW;
    constexpr int NF = kKv8Flight;
    __shared__ float s_acc[NG * DKV];
    __shared__ float s_m[NG];
    __shared__ float s_l[NG];

    const int bh = blockIdx.x;
    const int b = bh / a.nH, h = bh - b * a.nH;
    if constexpr (LIVE) {
        if (args.live[b] == 0) {   // block-uniform: zeros to out[b, h, :]
            if (threadIdx.x < DKV / 2)
                *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(a.out) + int64_t(bh) * DKV + 2 * threadIdx.x) = 0u;
            return;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sl = lane % LPR;
    const int gg = wave * KPW + lane / LPR;
    const float ks = args.k_scale[bh], vs = args.v_scale[bh];

    float qf[EPV];
    {
        const uint16_t* qp = static_cast<const uint16_t*>(a.q) + int64_t(b) * a.ldq + h * DKV + sl * EPV;
        float lo[8], hi[8];
        BF16T::unpack(*reinterpret_cast<const vec4u*>(qp), lo);
        BF16T::unpack(*reinterpret_cast<const vec4u*>(qp + 8), hi);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qf[e] = lo[e];
            qf[8 + e] = hi[e];
        }
    }
    const int64_t base = int64_t(bh) * a.max_len * DKV + sl * EPV;   // bytes
    const uint8_t* K = static_cast<const uint8_t*>(a.k) + base;
    const uint8_t* V = static_cast<const uint8_t*>(a.v) + base;
    const int64_t* mask = MASKED ? a.mask + int64_t(b) * a.max_len : nullptr;

    float m = -INFINITY, l = 0.f, acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;

    auto step = [&](const vec4u& kv, const vec4u& vv) {
        float kf[EPV], vf[EPV];
        kv8_unpack(kv, kf);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < EPV; ++e) s = fmaf(qf[e], kf[e], s);
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        s *= ks;
        const float mn = fmaxf(m, s);
        const float sc = expf(m - mn), p = expf(s - mn);
        l = fmaf(l, sc, p);
        kv8_unpack(vv, vf);
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] = fmaf(acc[e], sc, p * vf[e]);
        m = mn;
    };

    const int n = a.max_len;
#pragma unroll 1
    for (int j0 = gg; j0 < n; j0 += NF * NG) {
        bool on[NF];
        vec4u kk[NF], vv[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int j = j0 + f * NG;
            on[f] = j < n;
            if (MASKED) on[f] = on[f] && mask[on[f] ? j : j0] != 0;
            kk[f] = vec4u_make(0, 0, 0, 0);
            vv[f] = kk[f];
            if (on[f]) {
                kk[f] = *reinterpret_cast<const vec4u*>(K + int64_t(j) * DKV);
                vv[f] = *reinterpret_cast<const vec4u*>(V + int64_t(j) * DKV);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (on[f]) step(kk[f], vv[f]);
    }

#pragma unroll
    for (int e = 0; e < EPV; ++e) s_acc[gg * DKV + sl * EPV + e] = acc[e];
    if (sl == 0) {
        s_m[gg] = m;
        s_l[gg] = l;
    }
    __syncthreads();
    if (threadIdx.x < DKV / 2) {
        const int d = 2 * threadIdx.x;
        float M = s_m[0];
        for (int g = 1; g < NG; ++g) M = fmaxf(M, s_m[g]);
        float L = 0.f, o0 = 0.f, o1 = 0.f;
        for (int g = 0; g < NG; ++g) {
            // a group that saw no live key: l is exactly 0 (one live key makes it >= 1, and a NaN
            // scale makes it NaN, which must reach the output)
            if (s_l[g] == 0.f) continue;
            const float w = expf(s_m[g] - M);
            L = fmaf(s_l[g], w, L);
            o0 = fmaf(s_acc[g * DKV + d], w, o0);
            o1 = fmaf(s_acc[g * DKV + d + 1], w, o1);
        }
        const bool any = L > 0.f || L != L;   // no live key at all: zeros
        o0 = any ? (o0 * vs) / L : 0.f;
        o1 = any ? (o1 * vs) / L : 0.f;
        *reinterpret_cast<uint32_t*>(static_cast<uint16_t*>(a.out) + int64_t(bh) * DKV + d) = pack_bf2(o0, o1);
    }
}

typedef void (*t5_kv8_kernel_t)(const T5AttnKv8Args);
template <int DKV>
static t5_kv8_kernel_t t5_pick_kv8_d(bool masked, bool live) {
    if (live) return masked ? k_t5_decode_attn_kv8<DKV, true, true> : k_t5_decode_attn_kv8<DKV, false, true>;
    return masked ? k_t5_decode_attn_kv8<DKV, true, false> : k_t5_decode_attn_kv8<DKV, false, false>;
}

extern "C" int trlx_t5_decode_attn_kv8(const TrlxT5DecodeAttnArgs* a, const float* k_scale, const float* v_scale,
                                       const int64_t* live, void* stream) {
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "t5 decode attention, fp8 keys: NULL arguments");
    TRLX_REQUIRE(a->mode == TRLX_T5_ATTN_CROSS, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys: mode %d (the cross-attention only)", a->mode);
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_ARG, "t5 decode attention, fp8 keys: dtype %d (bf16 q and out only)",
                 a->dtype);
    TRLX_REQUIRE(k_scale && v_scale, TRLX_ERR_ARG, "t5 decode attention, fp8 keys: NULL k_scale / v_scale");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(k_scale) & 3u) == 0 && (reinterpret_cast<uintptr_t>(v_scale) & 3u) == 0,
                 TRLX_ERR_ARG, "t5 decode attention, fp8 keys: the scales are not aligned to 4 bytes");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(live) & 7u) == 0, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys: live is not aligned to 8 bytes");
    // what the cross mode of trlx_t5_decode_attn refuses
    TRLX_REQUIRE(a->d_kv == 64 || a->d_kv == 128, TRLX_ERR_ARG, "t5 decode attention, fp8 keys: d_kv %lld (64 and 128 only)",
                 (long long)a->d_kv);
    TRLX_REQUIRE(a->B >= 1 && a->n_heads >= 1 && a->max_len >= 1 && a->B * a->n_heads <= 0x7fffffffLL &&
                     a->max_len <= 0x7fffffffLL / 128 && a->n_heads <= 0x7fffffffLL / 128,
                 TRLX_ERR_ARG, "t5 decode attention, fp8 keys: B %lld, heads %lld, max_len %lld", (long long)a->B,
                 (long long)a->n_heads, (long long)a->max_len);
    TRLX_REQUIRE(a->q && a->k && a->v && a->out, TRLX_ERR_ARG, "t5 decode attention, fp8 keys: NULL q / K / V / out");
    const int64_t inner = a->n_heads * a->d_kv;
    const int64_t ldq = a->B == 1 ? inner : a->ldq;   // a single row has no stride to speak of
    TRLX_REQUIRE(ldq >= inner && ldq % 8 == 0, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys: q row stride %lld (>= heads * d_kv = %lld, whole 16-byte vectors)",
                 (long long)ldq, (long long)inner);
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(a->q, 15) && !mis(a->k, 15) && !mis(a->v, 15) && !mis(a->out, 15), TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys: q, K, V and out must be 16-byte aligned");
    TRLX_REQUIRE(!a->k_new && !a->v_new && !a->bias_by_distance, TRLX_ERR_ARG,
                 "t5 decode attention, fp8 keys: k_new / v_new / bias_by_distance are for the self-attention only");
    TRLX_REQUIRE(!mis(a->key_mask, 7), TRLX_ERR_ARG, "t5 decode attention, fp8 keys: key_mask not aligned to 8 bytes");
    T5AttnKv8Args k = {};
    k.q = a->q;
    k.k = a->k;
    k.v = a->v;
    k.mask = a->key_mask;
    k.out = a->out;
    k.ldq = ldq;
    k.nH = int(a->n_heads);
    k.max_len = int(a->max_len);
    k.k_scale = k_scale;
    k.v_scale = v_scale;
    k.live = live;
    const bool masked = a->key_mask != nullptr;
    hipLaunchKernelGGL(a->d_kv == 64 ? t5_pick_kv8_d<64>(masked, live != nullptr) : t5_pick_kv8_d<128>(masked, live != nullptr),
                       dim3(unsigned(a->B * a->n_heads)), dim3(kT5Threads), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_attn_kv8");
}
