// Burnt-in UNIX time stamps of camera frames, read on the device.
//
// Replaces timestamp_utilities.parse_frame_timestamp (timestamp_utilities.py:46-115) as the loaders call it per frame
// (util_track/mp_loader.py:230, datareader.py:59-63): the strip frame[y0:y0+h, x0:x0+n*w] is turned to gray, thresholded
// at 127, cut into n cells of w columns, and every cell but the decimal point (cell 10) is looked up by its six-area
// checksum -- the white pixels in the row bands [0,h13) [h13,h23) [h23,h) crossed with the column halves [0,w12) [w12,w).
// A cell reads as the FIRST table entry equal in all six counts (min() over the dict's order at error 0); a cell
// without one fails the set.  Up to RN_TS_MAX_SETS (geometry, table) sets are tried in the caller's order
// (Camera_Wrapper's try-both); a frame nobody reads takes prev + 1/30.0 (both callers' fall-back) or NaN.
//
// The gray rule is OpenCV's published 8-bit BGR2GRAY, (3735 B + 19235 G + 9798 R + 16384) >> 15, restated below in ONE
// place: cv2 is not installed where this project is built, so parity with cv2 itself is unpinned ("4K frames").
//
// Latency-bound (a strip is about 30 x 250 pixels): one workgroup per frame walks the sets; its four waves take the
// cells j = wave, wave + 4, ...; the lanes stride over a cell's h*w pixels and the six counts are popcounts of ballots;
// the table sits in LDS, lane k compares entry k and a ballot picks the lowest.  No atomics; every loop has a fixed
// bound.  Every lane forms an address inside the frame (clamped coordinate) and masks the VALUE.
#include <stdint.h>

#include "common.h"

#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / RN_WAVE)

// OpenCV's 8-bit BGR -> gray: fixed point, 15 fractional bits, rounded
__device__ __forceinline__ unsigned ts_gray(unsigned blue, unsigned green, unsigned red) {
    return (3735u * blue + 19235u * green + 9798u * red + 16384u) >> 15;
}
#define TS_THRESHOLD 127u                          // cv2.threshold(gray, 127, 255, THRESH_BINARY): white when gray > 127

struct TsArgs {
    const uint8_t *frames;
    int64_t frame_stride, row_stride;              // bytes
    int B, H, W, G, swap_rb;
    rn_ts_geometry set[RN_TS_MAX_SETS];
    const int32_t *tables;                         // [G, RN_TS_MAX_KEYS, RN_TS_ROW]
    const double *prev;
    double *times;
    int32_t *status, *set_index, *fail_cell;
    int8_t *digits;
    uint8_t *mask;
};

__global__ __launch_bounds__(TS_THREADS) void ts_parse_kernel(const TsArgs a) {
    __shared__ int tab[RN_TS_MAX_KEYS * RN_TS_ROW];
    __shared__ int cell[RN_TS_MAX_CELLS], first[RN_TS_MAX_CELLS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t *f = a.frames + (int64_t)b * a.frame_stride;
    int used = -1, used_n = 0, first_fail = -1;
    for (int g = 0; g < RN_TS_MAX_SETS; ++g) {
        if (g >= a.G) break;
        const rn_ts_geometry s = a.set[g];
        __syncthreads();                                                         // the last set's tab / cell are read out
        for (int i = threadIdx.x; i < RN_TS_MAX_KEYS * RN_TS_ROW; i += TS_THREADS)
            tab[i] = a.tables[(int64_t)g * RN_TS_MAX_KEYS * RN_TS_ROW + i];
        if (threadIdx.x < RN_TS_MAX_CELLS) cell[threadIdx.x] = -1;
        __syncthreads();
        const int hw = s.h * s.w;
        const bool want_mask = g == 0 && a.mask != nullptr;
        for (int jj = 0; jj < RN_TS_MAX_CELLS / TS_WAVES; ++jj) {
            const int j = wv + TS_WAVES * jj;
            if (j >= s.n) break;
            const bool point = j == 10;
            if (point && !want_mask) continue;
            int cnt[6] = {0, 0, 0, 0, 0, 0};
            for (int it = 0; it < RN_TS_MAX_CELL_PIXELS / RN_WAVE; ++it) {
                if (it * RN_WAVE >= hw) break;
                const int p = it * RN_WAVE + lane;
                const bool act = p < hw;
                const int pc = act ? p : hw - 1;
                const int r = pc / s.w, c = pc - r * s.w;
                const int y = s.y0 + r, x = s.x0 + j * s.w + c;
                const bool inside = y < a.H && x < a.W;                          // outside the frame: dark (numpy's clamped slice)
                const int yc = y < a.H ? y : a.H - 1, xc = x < a.W ? x : a.W - 1;
                const uint8_t *q = f + (int64_t)yc * a.row_stride + (int64_t)xc * 3;
                const unsigned v0 = q[0], v1 = q[1], v2 = q[2];
                const unsigned gray = a.swap_rb ? ts_gray(v2, v1, v0) : ts_gray(v0, v1, v2);
                const bool white = act && inside && gray > TS_THRESHOLD;
                const int area = (r < s.h13 ? 0 : r < s.h23 ? 2 : 4) + (c < s.w12 ? 0 : 1);
#pragma unroll
                for (int k = 0; k < 6; ++k) cnt[k] += __popcll(__ballot(white && area == k));
                if (want_mask && act)
                    a.mask[((int64_t)b * s.h + r) * ((int64_t)s.n * s.w) + (int64_t)j * s.w + c] = white ? 255 : 0;
            }
            if (point) continue;
            const int *e = tab + lane * RN_TS_ROW;
            const bool eq = lane < s.K && e[0] == cnt[0] && e[1] == cnt[1] && e[2] == cnt[2] && e[3] == cnt[3] &&
                            e[4] == cnt[4] && e[5] == cnt[5];
            const unsigned long long m = __ballot(eq);
            if (lane == 0) cell[j] = m ? __ffsll((long long)m) - 1 : -1;         // the first equal entry
        }
        __syncthreads();
        int fail = -1;                                                           // every thread reads the same words: uniform
        for (int j = RN_TS_MAX_CELLS - 1; j >= 0; --j)
            if (j < s.n && j != 10 && cell[j] < 0) fail = j;
        if (g == 0) {
            first_fail = fail;
            if (threadIdx.x < RN_TS_MAX_CELLS) first[threadIdx.x] = cell[threadIdx.x];
        }
        if (fail < 0) {
            used = g;
            used_n = s.n;
            break;
        }
    }
    __syncthreads();
    if (threadIdx.x < RN_TS_MAX_CELLS) a.digits[b * RN_TS_MAX_CELLS + threadIdx.x] = (int8_t)(used >= 0 ? cell[threadIdx.x] : first[threadIdx.x]);
    if (threadIdx.x != 0) return;
    double t;
    int st;
    if (used >= 0) {
        long long D = 0;
        for (int j = 0; j < RN_TS_MAX_CELLS; ++j)
            if (j < used_n && j != 10) D = D * 10 + tab[cell[j] * RN_TS_ROW + 6];
        double p10 = 1.0;                                                        // 10^F, F = max(n - 11, 0) <= 5: exact
        for (int j = 11; j < RN_TS_MAX_CELLS; ++j)
            if (j < used_n) p10 *= 10.0;
        t = (double)D / p10;                                                 // both exact (<= 15 digits): the correctly rounded decimal
        st = RN_TS_READ;
    } else if (a.prev) {
        t = a.prev[b] + (1 / 30.0);
        st = RN_TS_FELL_BACK;
    } else {
        t = __longlong_as_double(0x7ff8000000000000ll);
        st = RN_TS_FAILED;
    }
    a.times[b] = t;
    a.status[b] = st;
    a.set_index[b] = used;
    a.fail_cell[b] = first_fail;
}

extern "C" int rn_parse_frame_timestamps(const uint8_t *frames, int B, int H, int W, int64_t frame_stride,
                                         int64_t row_stride, int swap_rb, const rn_ts_geometry *sets, int G,
                                         const int32_t *tables, const double *prev, double *times, int32_t *status,
                                         int32_t *set_index, int8_t *digits, int32_t *fail_cell, uint8_t *mask,
                                         void *stream) {
    if (!frames || !sets || !tables || !times || !status || !set_index || !digits || !fail_cell) return RN_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || H > RN_TS_MAX_COORD || W > RN_TS_MAX_COORD || G < 1 || G > RN_TS_MAX_SETS) return RN_EINVAL;
    if (row_stride < (int64_t)W * 3 || frame_stride < 0 || (B > 1 && frame_stride < (int64_t)(H - 1) * row_stride + (int64_t)W * 3))
        return RN_EINVAL;
    TsArgs a;
    for (int g = 0; g < G; ++g) {
        const rn_ts_geometry &s = sets[g];
        if (s.n < 1 || s.n > RN_TS_MAX_CELLS || s.K < 1 || s.K > RN_TS_MAX_KEYS) return RN_EINVAL;
        if (s.x0 < 0 || s.y0 < 0 || s.x0 > RN_TS_MAX_COORD || s.y0 > RN_TS_MAX_COORD) return RN_EINVAL;
        if (s.w < 1 || s.h < 1 || (int64_t)s.w * s.h > RN_TS_MAX_CELL_PIXELS) return RN_EINVAL;
        if (s.h13 < 0 || s.h13 > s.h23 || s.h23 > s.h || s.w12 < 0 || s.w12 > s.w) return RN_EINVAL;
        a.set[g] = s;
    }
    for (int g = G; g < RN_TS_MAX_SETS; ++g) a.set[g] = sets[0];
    a.frames = frames; a.frame_stride = frame_stride; a.row_stride = row_stride;
    a.B = B; a.H = H; a.W = W; a.G = G; a.swap_rb = swap_rb ? 1 : 0;
    a.tables = tables; a.prev = prev; a.times = times; a.status = status; a.set_index = set_index;
    a.fail_cell = fail_cell; a.digits = digits; a.mask = mask;
    hipLaunchKernelGGL(ts_parse_kernel, dim3(B), dim3(TS_THREADS), 0, (hipStream_t)stream, a);
    RN_LAUNCH_CHECK();
    return RN_OK;
}
