// The decode clock: the device record {t, T, cur_len0, overrun, 0, 0, 0, 0} (int64) that the
// device-clock entries of the decode step read where the host entries take t by value, and the
// one-thread launch that advances it.  See trlx_decode_clock_init in trlx_t5_amd.h.  A decode
// step that reads t from here has the same launch arguments at every token, so a graph captured
// once replays the whole rollout.
#include "common.h"

namespace trlx {

__global__ __launch_bounds__(kWave) void k_decode_clock_init(int64_t* clock, int64_t T, int64_t cur_len0) {
    if (threadIdx.x != 0) return;
    clock[TRLX_CLOCK_T] = 0;
    clock[TRLX_CLOCK_CAP] = T;
    clock[TRLX_CLOCK_CUR_LEN0] = cur_len0;
    clock[TRLX_CLOCK_OVERRUN] = 0;
    for (int i = TRLX_CLOCK_OVERRUN + 1; i < TRLX_CLOCK_WORDS; ++i) clock[i] = 0;
}

__global__ __launch_bounds__(kWave) void k_decode_clock_advance(int64_t* clock) {
    if (threadIdx.x != 0) return;
    const int64_t t = clock[TRLX_CLOCK_T];
    if (t < clock[TRLX_CLOCK_CAP]) clock[TRLX_CLOCK_T] = t + 1;
    else clock[TRLX_CLOCK_OVERRUN] = clock[TRLX_CLOCK_OVERRUN] + 1;
}

static int check_clock(const int64_t* clock) {
    TRLX_REQUIRE(clock, TRLX_ERR_ARG, "decode clock: NULL record");
    TRLX_REQUIRE((reinterpret_cast<uintptr_t>(clock) & 7u) == 0, TRLX_ERR_ARG,
                 "decode clock: the record is not aligned to 8 bytes");
    return TRLX_OK;
}

}  // namespace trlx

using namespace trlx;

extern "C" int trlx_decode_clock_init(int64_t* clock, int64_t T, int64_t cur_len0, void* stream) {
    const int rc = check_clock(clock);
    if (rc) return rc;
    TRLX_REQUIRE(T >= 1, TRLX_ERR_ARG, "decode clock: capacity T %lld (at least one step)", (long long)T);
    TRLX_REQUIRE(cur_len0 >= 0, TRLX_ERR_ARG, "decode clock: cur_len0 %lld must be >= 0", (long long)cur_len0);
    hipLaunchKernelGGL(k_decode_clock_init, dim3(1), dim3(kWave), 0, (hipStream_t)stream, clock, T, cur_len0);
    return check_launch("k_decode_clock_init");
}

extern "C" int trlx_decode_clock_advance(int64_t* clock, void* stream) {
    const int rc = check_clock(clock);
    if (rc) return rc;
    hipLaunchKernelGGL(k_decode_clock_advance, dim3(1), dim3(kWave), 0, (hipStream_t)stream, clock);
    return check_launch("k_decode_clock_advance");
}
