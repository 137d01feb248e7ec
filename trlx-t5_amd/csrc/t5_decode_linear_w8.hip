// fp8 weights for the decode-step projections: the quantiser and a streaming skinny GEMM.
//   out = epilogue( prologue(x) . (scale (.) W8)^T )      x [M, K] bf16, W8 [N, K] e4m3fn bytes,
//                                                          scale [N] fp32 powers of two, out [M, N] bf16
// The prologue (none / T5's RMSNorm with t5_rmsnorm's bits) and the epilogues (none, + residual,
// act(u), act(u) * v over a packed [2N, K] weight) are trlx_t5_decode_linear's.  At M <= 256 a
// projection is a read of its weight; this form halves the bytes and is blocked to keep HBM busy.
//
// Quantiser (k_t5_linear_w8_quantize).  k_t5_cross_kv_quantize's scheme over a weight row: one wave
// per row, two passes.  Pass 1 takes the integer maximum of the sign-cleared bf16 patterns, from it
// q8_exponent gives e; pass 2 reads the row again (cache-resident), multiplies by 2^-e (exact) and
// casts with f32_to_e4m3fn: torch's (w.float() * 2**-e).to(float8_e4m3fn), bit for bit.  A row with
// an Inf / NaN gets a NaN scale and 0x7f in every byte, the kv8 quantiser's rule.
//
// Projection (k_t5_decode_linear_w8).  A workgroup is WV waves, WV in {4, 8, 16}, and owns 16 output
// columns (both slabs of them when gated) and every row, in passes of MT 16-row tiles.
//   Loads.  K is cut into chunks of 64.  Lane (fr, fc) = (lane & 15, lane >> 4) reads the 16 bytes
//     k = 64 c + 16 fc .. + 15 of weight row n0 + fr: one global_load_dwordx4.  The bytes become bf16
//     in registers (v_cvt_pk_f32_fp8, then the upper halves: exact, e4m3 is a subset of bf16) and the
//     two 8-element halves feed two v_mfma_f32_16x16x32_bf16 with the weight as the first operand.
//     The x fragment of a lane is the same 16 k of its token row, so inside a chunk both operands
//     see the same permutation of k and the dot product is that of the chunk.
//   Turns.  A turn is four chunks, 256 B of each weight row.  Turn j belongs to wave j % WV.  A wave
//     issues the loads of its next turn before the converts and MFMAs of the current one (two
//     register buffers), so 8 loads of 16 B per slab are in flight per lane.
//   Merge.  The waves' partial accumulators of a tile go through LDS to the tile's owner wave (tile
//     mt belongs to wave mt % WV), which adds them in wave order p0 + p1 + ... : a fixed order, no
//     atomics, no workspace.  At WV 16 the tiles take the LDS in rounds of four.
//   Scale.  The owner multiplies the merged fp32 sums by the row's power-of-two scale (exact barring
//     overflow / underflow), then runs the epilogue on fp32 and rounds once.
// A row's bits depend on its x row, the weight row, K and WV -- not on M, N or where the row sits.
#include "common.h"
#include "t5_q8.h"
#include "t5_row_math.h"

namespace trlx {

typedef __bf16 w8_bf16x8 __attribute__((ext_vector_type(8)));
typedef float w8_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t w8_vec2u __attribute__((ext_vector_type(2)));

constexpr int kW8BN = 16;                 // output columns per workgroup
constexpr int kW8BM = 16;                 // rows per tile
constexpr int kW8CK = 64;                 // K per chunk: one 16-byte weight load per lane, two MFMAs
constexpr int kW8KU = 4;                  // chunks per turn
constexpr int kW8TurnK = kW8CK * kW8KU;
constexpr int kW8MaxTiles = 8;            // accumulator tiles (row tiles x slabs) of a wave
constexpr int kW8MaxWaves = 16;
constexpr int kW8LdsTiles = 60;           // KB of partial tiles in LDS at a time (1 KB a tile and wave)
constexpr int kW8NormMaxK = 8192;         // t5_rmsnorm's limit
constexpr int kW8WaveRowMaxK = 1024;      // up to here the norm's sum takes one wave per row
constexpr int kW8MaxK = 16384;
constexpr int kW8Cus = 256;               // the chip the default WV is sized for

enum { kW8Plain = 0, kW8Residual = 1, kW8Act = 2 };

struct W8Args {
    const uint16_t* x;
    const uint8_t* w;
    const float* scale;
    const uint16_t *nw, *res;
    uint16_t* out;
    int64_t ld_x, ld_w, ld_res, ld_out, M;
    int K, N, act;   // N: output columns (F of the gated form)
    float eps;
};

__device__ __forceinline__ vec4u w8_ld16(const void* p) { return *reinterpret_cast<const vec4u*>(p); }

// four e4m3fn bytes to four bf16 (two words): the fp32 of the hardware convert, upper halves kept
__device__ __forceinline__ void w8_cvt4(uint32_t b, uint32_t& lo, uint32_t& hi) {
    const auto p = __builtin_amdgcn_cvt_pk_f32_fp8(int(b), false);
    const auto q = __builtin_amdgcn_cvt_pk_f32_fp8(int(b), true);
    lo = __builtin_amdgcn_perm(__float_as_uint(p[1]), __float_as_uint(p[0]), 0x07060302u);
    hi = __builtin_amdgcn_perm(__float_as_uint(q[1]), __float_as_uint(q[0]), 0x07060302u);
}

__device__ __forceinline__ w8_bf16x8 w8_cvt8(uint32_t b0, uint32_t b1) {
    vec4u r;
    uint32_t a, b, c, d;
    w8_cvt4(b0, a, b);
    w8_cvt4(b1, c, d);
    r.x = a, r.y = b, r.z = c, r.w = d;
    return __builtin_bit_cast(w8_bf16x8, r);
}

__device__ __forceinline__ float w8_sumsq_unit(float s, const uint16_t* p) {
    float f[8];
    BF16T::unpack(w8_ld16(p), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += f[i] * f[i];
    return s;
}

// bf16(nw * (x * rstd)) of one 16-byte vector: t5_rmsnorm's product and its one rounding
__device__ __forceinline__ vec4u w8_norm8(const vec4u& xv, const vec4u& g, float rs) {
    float f[8], gf[8];
    BF16T::unpack(xv, f);
    BF16T::unpack(g, gf);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = gf[i] * (f[i] * rs);
    return BF16T::pack(f);
}

__device__ __forceinline__ float w8_act(int act, float u) {
    float a, d;
    if (act == TRLX_T5_ACT_RELU) fa_eval<TRLX_T5_ACT_RELU, false>(u, a, d);
    else if (act == TRLX_T5_ACT_GELU_NEW) fa_eval<TRLX_T5_ACT_GELU_NEW, false>(u, a, d);
    else fa_eval<TRLX_T5_ACT_SILU, false>(u, a, d);
    return a;
}

template <int WV, int MT, int NB, int EPI, bool NORM>
__global__ __launch_bounds__(WV* kWave) void k_t5_decode_linear_w8(const W8Args a) {
    constexpr int NT = MT * NB;                                     // accumulator tiles of a wave
    // 16 waves are 1024 threads and 128 registers a lane: the x loads of one tile at a time, and with
    // two slabs no second weight buffer (the 16 waves' loads overlap each other instead)
    constexpr bool kFence = WV == kW8MaxWaves || (MT == 8 && NORM);
    constexpr bool kAhead = !(WV == kW8MaxWaves && NB == 2);
    constexpr int TRmax = kW8LdsTiles / (WV - 1) >= kW8MaxTiles ? kW8MaxTiles : 4;
    constexpr int TR = NT < TRmax ? NT : TRmax;                     // tiles per merge round
    static_assert(NT <= kW8MaxTiles && (NB == 1 || EPI == kW8Act) && NT % TR == 0 && TR % NB == 0, "tile budget");
    static_assert(TR * (WV - 1) <= kW8LdsTiles, "LDS budget");
    __shared__ w8_f32x4 part[TR * (WV - 1) * kWave];                // [tile of the round][wave slot][lane]
    __shared__ float s_rstd[NORM ? MT * kW8BM : 1];
    __shared__ float s_ws[NORM ? MT * kW8BM * 4 : 1];               // a row's four wave sums
    const int tid = int(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
    const int fr = lane & 15, fc = lane >> 4;
    const int n0 = int(blockIdx.x) * kW8BN;
    const int nchunk = a.K / kW8CK;
    const int nturn = (nchunk + kW8KU - 1) / kW8KU;
    const uint8_t* wrow[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) wrow[s] = a.w + (int64_t(s) * a.N + n0 + fr) * a.ld_w + fc * 16;

    // the 16-byte loads of turn jt: a chunk past the end is clamped (loaded, not used)
    auto load_turn = [&](vec4u(&d)[NB][kW8KU], int jt) {
#pragma unroll
        for (int u = 0; u < kW8KU; ++u) {
            const int c = jt * kW8KU + u < nchunk ? jt * kW8KU + u : nchunk - 1;
#pragma unroll
            for (int s = 0; s < NB; ++s) d[s][u] = w8_ld16(wrow[s] + c * kW8CK);
        }
    };

#pragma unroll 1
    for (int64_t m0 = 0; m0 < a.M; m0 += MT * kW8BM) {
        const int rows = int(a.M - m0 < MT * kW8BM ? a.M - m0 : MT * kW8BM);
        __syncthreads();                                            // the pass before is done with part and s_rstd
        // this wave's first turn is on its way while the norm's sums run
        vec4u wf[NB][kW8KU];
        if (kAhead && wave < nturn) load_turn(wf, wave);
        if constexpr (NORM) {
            // the sum of k_t5_rmsnorm_fwd for D = K: one wave per row up to 1024, a team of four waves above
            if (a.K <= kW8WaveRowMaxK) {
#pragma unroll 1
                for (int r = wave; r < rows; r += WV) {
                    const uint16_t* xr = a.x + (m0 + r) * a.ld_x;
                    float s = 0.f;
                    for (int c = lane * 8; c < a.K; c += kWave * 8) s = w8_sumsq_unit(s, xr + c);
                    s = wave_sum(s);
                    if (lane == 0) s_rstd[r] = rn_rstd(s, a.K, a.eps);
                }
            } else {
                const int tt = tid & 255;
#pragma unroll 1
                for (int r = wave >> 2; r < rows; r += WV / 4) {
                    const uint16_t* xr = a.x + (m0 + r) * a.ld_x;
                    float s = 0.f;
                    for (int c = tt * 8; c < a.K; c += 256 * 8) s = w8_sumsq_unit(s, xr + c);
                    s = wave_sum(s);
                    if (lane == 0) s_ws[r * 4 + (wave & 3)] = s;
                }
                __syncthreads();
                for (int r = tid; r < rows; r += WV * kWave)
                    s_rstd[r] = rn_rstd(((s_ws[r * 4] + s_ws[r * 4 + 1]) + s_ws[r * 4 + 2]) + s_ws[r * 4 + 3], a.K, a.eps);
            }
            __syncthreads();
        }

        // this lane's token row of every tile, clamped to the pass's last row (its results are dropped)
        const uint16_t* xrow[MT];
        float rs[NORM ? MT : 1];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int lr = mt * kW8BM + fr < rows ? mt * kW8BM + fr : rows - 1;
            xrow[mt] = a.x + (m0 + lr) * a.ld_x + fc * 16;
            if constexpr (NORM) rs[mt] = s_rstd[lr];
        }
        w8_f32x4 acc[MT][NB];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int s = 0; s < NB; ++s) acc[mt][s] = w8_f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
        for (int j = wave; j < nturn; j += WV) {
            vec4u wn[kAhead ? NB : 1][kW8KU];
            if constexpr (!kAhead) {
                load_turn(wf, j);
            } else if (j + WV < nturn) {                            // wave-uniform: the next turn's loads first
                load_turn(wn, j + WV);
            } else {
#pragma unroll
                for (int u = 0; u < kW8KU; ++u)
#pragma unroll
                    for (int s = 0; s < NB; ++s) wn[s][u] = wf[s][u];
            }
#pragma unroll
            for (int u = 0; u < kW8KU; ++u) {
                const int c = j * kW8KU + u;
                if (c >= nchunk) break;                             // wave-uniform: a partial last turn
                w8_bf16x8 wa[NB], wb[NB];
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    wa[s] = w8_cvt8(wf[s][u].x, wf[s][u].y);
                    wb[s] = w8_cvt8(wf[s][u].z, wf[s][u].w);
                }
                vec4u g0, g1;
                if constexpr (NORM) {
                    g0 = w8_ld16(a.nw + c * kW8CK + fc * 16);
                    g1 = w8_ld16(a.nw + c * kW8CK + fc * 16 + 8);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if constexpr (kFence) __builtin_amdgcn_sched_barrier(0);
                    vec4u x0 = w8_ld16(xrow[mt] + c * kW8CK), x1 = w8_ld16(xrow[mt] + c * kW8CK + 8);
                    if constexpr (NORM) {
                        if constexpr (kFence) launder(g0);          // unpacked per tile, not held as 16 floats
                        x0 = w8_norm8(x0, g0, rs[mt]);
                        if constexpr (kFence) __builtin_amdgcn_sched_barrier(0), launder(g1);
                        x1 = w8_norm8(x1, g1, rs[mt]);
                    }
#pragma unroll
                    for (int s = 0; s < NB; ++s) {
                        acc[mt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[s], __builtin_bit_cast(w8_bf16x8, x0), acc[mt][s], 0, 0, 0);
                        acc[mt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[s], __builtin_bit_cast(w8_bf16x8, x1), acc[mt][s], 0, 0, 0);
                    }
                }
            }
            if constexpr (kAhead) {
#pragma unroll
                for (int u = 0; u < kW8KU; ++u)
#pragma unroll
                    for (int s = 0; s < NB; ++s) wf[s][u] = wn[s][u];
            }
        }

        // the partial sums of a tile go to its owner wave, which adds all WV in wave order
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += TR) {
            if (t0) __syncthreads();                                // the round before has been read
#pragma unroll
            for (int t = t0; t < t0 + TR; ++t) {
                const int mt = t / NB, s = t % NB, owner = mt % WV;
                if (wave != owner) part[((t - t0) * (WV - 1) + (wave < owner ? wave : wave - 1)) * kWave + lane] = acc[mt][s];
            }
            __syncthreads();
#pragma unroll
            for (int mt = t0 / NB; mt < (t0 + TR) / NB; ++mt) {
                const int owner = mt % WV;
                if (wave != owner) continue;
                const int lr = mt * kW8BM + fr;
                const int n = n0 + fc * 4;
                w8_f32x4 sum[NB];
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    const int t = mt * NB + s;
                    w8_f32x4 v = w8_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                    for (int w = 0; w < WV; ++w) {                  // four LDS reads in flight, not WV - 1
                        w8_f32x4 p = acc[mt][s];
                        if (w != owner) p = part[((t - t0) * (WV - 1) + (w < owner ? w : w - 1)) * kWave + lane];
                        v = w == 0 ? p : v + p;
                    }
                    sum[s] = v * *reinterpret_cast<const w8_f32x4*>(a.scale + int64_t(s) * a.N + n);
                }
                if (lr >= rows) continue;
                const int64_t m = m0 + lr;
                float y[4];
                if constexpr (EPI == kW8Residual) {
                    const w8_vec2u rv = *reinterpret_cast<const w8_vec2u*>(a.res + m * a.ld_res + n);
                    y[0] = sum[0][0] + bf_lo(rv.x), y[1] = sum[0][1] + bf_hi(rv.x);
                    y[2] = sum[0][2] + bf_lo(rv.y), y[3] = sum[0][3] + bf_hi(rv.y);
                } else if constexpr (EPI == kW8Act) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float act = w8_act(a.act, sum[0][q]);
                        y[q] = NB == 2 ? act * sum[NB - 1][q] : act;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) y[q] = sum[0][q];
                }
                w8_vec2u o;
                o.x = pack_bf2(y[0], y[1]), o.y = pack_bf2(y[2], y[3]);
                *reinterpret_cast<w8_vec2u*>(a.out + m * a.ld_out + n) = o;
            }
        }
    }
}

typedef void (*w8_kernel_t)(const W8Args);

// accumulator tiles of a wave: 16 waves are 1024 threads, 128 registers each, and hold half as many,
// a quarter with the norm's product in the loop
constexpr int w8_max_tiles(int wv, bool norm) { return wv == kW8MaxWaves ? kW8MaxTiles / (norm ? 4 : 2) : kW8MaxTiles; }

template <int WV, int MT, int NB, int EPI>
static w8_kernel_t w8_pick_one(bool norm) {
    if (norm) {
        if constexpr (MT * NB <= w8_max_tiles(WV, true)) return k_t5_decode_linear_w8<WV, MT, NB, EPI, true>;
    } else {
        if constexpr (MT * NB <= w8_max_tiles(WV, false)) return k_t5_decode_linear_w8<WV, MT, NB, EPI, false>;
    }
    return nullptr;   // not reached: w8_row_tiles stays under the cap
}

template <int WV, int NB, int EPI>
static w8_kernel_t w8_pick_mt(int mt, bool norm) {
    switch (mt) {
        case 1: return w8_pick_one<WV, 1, NB, EPI>(norm);
        case 2: return w8_pick_one<WV, 2, NB, EPI>(norm);
        case 4: return w8_pick_one<WV, 4, NB, EPI>(norm);
        default: return w8_pick_one<WV, 8 / NB, NB, EPI>(norm);
    }
}

template <int WV>
static w8_kernel_t w8_pick_epi(int epi, bool gated, int mt, bool norm) {
    if (epi == kW8Act) return gated ? w8_pick_mt<WV, 2, kW8Act>(mt, norm) : w8_pick_mt<WV, 1, kW8Act>(mt, norm);
    return epi == kW8Residual ? w8_pick_mt<WV, 1, kW8Residual>(mt, norm) : w8_pick_mt<WV, 1, kW8Plain>(mt, norm);
}

// row tiles per pass for M rows and NB slabs
static int w8_row_tiles(int64_t M, int nb, int wv, bool norm) {
    const int64_t tiles = (M + kW8BM - 1) / kW8BM;
    const int cap = w8_max_tiles(wv, norm) / nb;
    const int mt = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
    return mt < cap ? mt : cap;
}

// The default WV, a pure function of (N, K, gated): the smallest of 4, 8, 16 that puts four waves on
// every SIMD (N / 16 workgroups over kW8Cus CUs of four SIMDs), and no more waves than K has turns.
// Set from profiles/t5_decode_linear_w8_bench.json: within about an eighth of the fastest WV at 8 rows
// on every call measured; a gated weight is not counted twice, the table does not bear that out.
static int w8_default_waves(int64_t N, int64_t K, bool gated) {
    (void)gated;
    const int64_t turns = (K + kW8TurnK - 1) / kW8TurnK;
    const int64_t want = 4 * 4 * kW8Cus;
    int wv = 4;
    while (wv < kW8MaxWaves && (N / kW8BN) * wv < want && 2 * wv <= turns) wv *= 2;
    return wv;
}

constexpr int kWqThreads = 256;
constexpr int kWqRows = kWqThreads / kWave;   // one wave per weight row

__global__ __launch_bounds__(kWqThreads) void k_t5_linear_w8_quantize(const uint16_t* w, int64_t ld_w, uint8_t* w8, float* scale,
                                                                      int N, int K) {
    const int lane = threadIdx.x & (kWave - 1);
    const int n = int(blockIdx.x) * kWqRows + int(threadIdx.x) / kWave;
    if (n >= N) return;                                             // wave-uniform, no barrier below
    const uint16_t* row = w + int64_t(n) * ld_w;
    uint32_t m = 0;
#pragma unroll 1
    for (int c = lane * 8; c < K; c += kWave * 8) m = q8_absmax(w8_ld16(row + c), m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, uint32_t(__shfl_xor(int(m), off, kWave)));
    // an Inf / NaN in the row: the scale is NaN and every byte of the row is the NaN byte
    const bool bad = m >= 0x7f80u;
    const int e = bad ? 0 : q8_exponent(m);
    const float inv = __uint_as_float(uint32_t(127 - e) << 23);
    if (lane == 0) scale[n] = bad ? __uint_as_float(0x7fc00000u) : __uint_as_float(uint32_t(127 + e) << 23);
    uint8_t* o = w8 + int64_t(n) * K;
#pragma unroll 1
    for (int c = lane * 8; c < K; c += kWave * 8) {
        const vec4u x = w8_ld16(row + c);
        *reinterpret_cast<uint2*>(o + c) = bad ? make_uint2(0x7f7f7f7fu, 0x7f7f7f7fu)
                                               : make_uint2(q8_pack4(x.x, x.y, inv), q8_pack4(x.z, x.w, inv));
    }
}

struct W8Op {
    const char* name;
    const void* p;
    int64_t ld, rows, cols;
    int esize;
    uintptr_t lo, hi;
};

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_t5_linear_w8_quantize(const void* w, int64_t ld_w, void* w8, float* scale, int64_t N, int64_t K,
                                          void* stream) {
    const char* who = "t5 linear w8 quantize";
    TRLX_REQUIRE(w && w8 && scale, TRLX_ERR_ARG, "%s: NULL w / w8 / scale", who);
    TRLX_REQUIRE(N >= 1 && N <= (int64_t(1) << 30), TRLX_ERR_SHAPE, "%s: N %lld (1 to 2^30)", who, (long long)N);
    TRLX_REQUIRE(K >= 8 && K % 8 == 0 && K <= kW8MaxK, TRLX_ERR_SHAPE, "%s: K %lld (a multiple of 8, 8 to %d)", who,
                 (long long)K, kW8MaxK);
    const int64_t ld = N == 1 ? K : ld_w;   // a single row has no stride to speak of
    TRLX_REQUIRE(ld >= K && ld % 8 == 0 && ld <= (int64_t(1) << 40), TRLX_ERR_STRIDE,
                 "%s: w row stride %lld (at least K = %lld, whole 16-byte vectors)", who, (long long)ld, (long long)K);
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    TRLX_REQUIRE(!mis(w, 15) && !mis(w8, 15) && !mis(scale, 15), TRLX_ERR_ARG, "%s: w, w8 and scale must be 16-byte aligned", who);
    hipLaunchKernelGGL(k_t5_linear_w8_quantize, dim3(unsigned((N + kWqRows - 1) / kWqRows)), dim3(kWqThreads), 0,
                       (hipStream_t)stream, static_cast<const uint16_t*>(w), ld, static_cast<uint8_t*>(w8), scale, int(N), int(K));
    return check_launch("k_t5_linear_w8_quantize");
}

extern "C" int trlx_t5_decode_linear_w8_geometry(int64_t N, int64_t K, int gated, TrlxT5DecodeLinearW8Geometry* g) {
    TRLX_REQUIRE(g, TRLX_ERR_ARG, "t5 decode linear w8 geometry: NULL geometry");
    TRLX_REQUIRE(N >= 1 && K >= 1, TRLX_ERR_SHAPE, "t5 decode linear w8 geometry: N %lld, K %lld", (long long)N, (long long)K);
    g->waves = w8_default_waves(N, K, gated != 0);
    g->turns = int((K + kW8TurnK - 1) / kW8TurnK);
    g->cols_per_block = kW8BN;
    g->rows_per_tile = kW8BM;
    g->k_per_chunk = kW8CK;
    g->chunks_per_wave_turn = kW8KU;
    g->max_row_tiles = kW8MaxTiles;
    g->max_k = kW8MaxK;
    g->norm_max_k = kW8NormMaxK;
    g->norm_wave_row_max_k = kW8WaveRowMaxK;
    return TRLX_OK;
}

extern "C" int trlx_t5_decode_linear_w8(const trlx_t5_decode_linear_w8_args* a, void* stream) {
    const char* who = "t5 decode linear w8";
    TRLX_REQUIRE(a, TRLX_ERR_ARG, "%s: NULL arguments", who);
    TRLX_REQUIRE(a->x && a->weight8 && a->scale && a->out, TRLX_ERR_ARG, "%s: NULL x / weight8 / scale / out", who);
    TRLX_REQUIRE(a->dtype == TRLX_BF16, TRLX_ERR_DTYPE, "%s: dtype %d (bfloat16 x and out only)", who, a->dtype);
    const bool has_act = a->act != TRLX_T5_ACT_NONE, gated = a->gated != 0, norm = a->norm_weight != nullptr;
    TRLX_REQUIRE(!has_act || a->act == TRLX_T5_ACT_RELU || a->act == TRLX_T5_ACT_GELU_NEW || a->act == TRLX_T5_ACT_SILU,
                 TRLX_ERR_ARG, "%s: activation %d (none -1, relu 0, gelu_new 1, silu 2)", who, a->act);
    TRLX_REQUIRE(!gated || has_act, TRLX_ERR_ARG, "%s: gated without an activation", who);
    TRLX_REQUIRE(!(has_act && a->residual), TRLX_ERR_ARG, "%s: a residual and an activation (one epilogue at most)", who);
    TRLX_REQUIRE(a->waves == 0 || a->waves == 4 || a->waves == 8 || a->waves == 16, TRLX_ERR_ARG,
                 "%s: waves %d (0 for the default, 4, 8 or 16)", who, a->waves);
    TRLX_REQUIRE(a->M >= 1 && a->M <= 0x7fffffffLL, TRLX_ERR_SHAPE, "%s: M %lld (1 to 2^31 - 1)", who, (long long)a->M);
    TRLX_REQUIRE(a->K >= kW8CK && a->K % kW8CK == 0 && a->K <= kW8MaxK, TRLX_ERR_SHAPE,
                 "%s: K %lld (a multiple of %d, %d to %d)", who, (long long)a->K, kW8CK, kW8CK, kW8MaxK);
    TRLX_REQUIRE(!norm || a->K <= kW8NormMaxK, TRLX_ERR_SHAPE, "%s: K %lld with a norm weight (at most %d, t5_rmsnorm's limit)",
                 who, (long long)a->K, kW8NormMaxK);
    TRLX_REQUIRE(a->N >= kW8BN && a->N % kW8BN == 0 && a->N <= (int64_t(1) << 30), TRLX_ERR_SHAPE,
                 "%s: N %lld (output columns: a multiple of %d, %d to 2^30)", who, (long long)a->N, kW8BN, kW8BN);
    TRLX_REQUIRE(!norm || a->eps == a->eps, TRLX_ERR_ARG, "%s: eps is NaN", who);
    const int nb = gated ? 2 : 1;
    const int64_t wrows = a->N * nb;
    W8Op ops[6] = {{"x", a->x, a->ld_x, a->M, a->K, 2, 0, 0},
                   {"weight8", a->weight8, a->ld_w, wrows, a->K, 1, 0, 0},
                   {"out", a->out, a->ld_out, a->M, a->N, 2, 0, 0},
                   {"residual", a->residual, a->ld_residual, a->M, a->N, 2, 0, 0},
                   {"norm_weight", a->norm_weight, a->K, 1, a->K, 2, 0, 0},
                   {"scale", a->scale, wrows, 1, wrows, 4, 0, 0}};
    for (int i = 0; i < 6; ++i) {
        W8Op& o = ops[i];
        if (!o.p) continue;
        const uintptr_t p = reinterpret_cast<uintptr_t>(o.p);
        TRLX_REQUIRE(p % 16 == 0, TRLX_ERR_ARG, "%s: %s not aligned to 16 bytes", who, o.name);
        TRLX_REQUIRE(o.ld >= o.cols, TRLX_ERR_STRIDE, "%s: %s row stride %lld below its %lld columns", who, o.name, (long long)o.ld,
                     (long long)o.cols);
        TRLX_REQUIRE(o.ld * o.esize % 16 == 0, TRLX_ERR_STRIDE, "%s: %s row stride %lld off the 16-byte grid", who, o.name,
                     (long long)o.ld);
        int64_t span;
        TRLX_REQUIRE(!__builtin_mul_overflow(o.rows - 1, o.ld, &span) && span <= (int64_t(1) << 59), TRLX_ERR_STRIDE,
                     "%s: %s rows %lld apart do not fit the address space", who, o.name, (long long)o.ld);
        o.lo = p, o.hi = p + uintptr_t((span + o.cols) * o.esize);
    }
    // out shares no byte range with x, the weight, its scales or norm_weight; with residual only as the very same rows
    const W8Op& out = ops[2];
    for (int i = 0; i < 6; ++i) {
        if (i == 2 || !ops[i].p || out.hi <= ops[i].lo || ops[i].hi <= out.lo) continue;
        const bool same_rows = i == 3 && a->residual == a->out && a->ld_residual == a->ld_out;
        TRLX_REQUIRE(same_rows, TRLX_ERR_ARG, "%s: out overlaps %s%s", who, ops[i].name,
                     i == 3 ? " (taken only as the very same rows: same pointer, same stride)" : "");
    }
    W8Args k = {};
    k.x = static_cast<const uint16_t*>(a->x), k.w = static_cast<const uint8_t*>(a->weight8), k.scale = a->scale;
    k.nw = static_cast<const uint16_t*>(a->norm_weight), k.res = static_cast<const uint16_t*>(a->residual);
    k.out = static_cast<uint16_t*>(a->out);
    k.ld_x = a->ld_x, k.ld_w = a->ld_w, k.ld_res = a->ld_residual, k.ld_out = a->ld_out, k.M = a->M;
    k.K = int(a->K), k.N = int(a->N), k.act = a->act, k.eps = a->eps;
    const int wv = a->waves ? a->waves : w8_default_waves(a->N, a->K, gated);
    const int mt = w8_row_tiles(a->M, nb, wv, norm);
    const int epi = has_act ? kW8Act : a->residual ? kW8Residual : kW8Plain;
    const w8_kernel_t fn = wv == 4 ? w8_pick_epi<4>(epi, gated, mt, norm)
                                   : wv == 8 ? w8_pick_epi<8>(epi, gated, mt, norm) : w8_pick_epi<16>(epi, gated, mt, norm);
    TRLX_REQUIRE(fn, TRLX_ERR_ARG, "%s: no kernel for %d row tiles at %d waves", who, mt, wv);
    hipLaunchKernelGGL(fn, dim3(unsigned(a->N / kW8BN)), dim3(unsigned(wv * kWave)), 0, (hipStream_t)stream, k);
    return check_launch("k_t5_decode_linear_w8");
}
