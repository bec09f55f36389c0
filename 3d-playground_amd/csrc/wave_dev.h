// Wave- and workgroup-level building blocks of the analysis kernels (calibration, filter fitting, AP, MOT, the data reader, time-stamp
// bias, label_*): scans, min / max, arg-reductions on a (value, index) total order, the status flag.  Device-only; wave_sum and the DPP
// helpers stay in common.h.  Every kernel that uses these is launched with a one-dimensional workgroup: lane = threadIdx.x & 63.
#pragma once
#include "common.h"

// "no candidate": an index behind every real one, so that a lane without a candidate loses every tie
#define RN_NO_INDEX 0x7fffffff

__device__ __forceinline__ void rn_flag(int32_t *status, int bit) { atomicOr(status, bit); }

// element k of np.linspace(start, stop, grid) in T: arange * step + start, the last element is stop itself
template <typename T>
__device__ __forceinline__ T rn_linspace(T start, T stop, T step, int k, int grid) {
    return k == grid - 1 ? stop : (T)k * step + start;
}

// ------------------------------------------------------------------------------------------------ scans (int, long long)
// Inclusive scan over the wave: lane l gets v(0) + ... + v(l); lane 63 holds the wave's total.
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & (RN_WAVE - 1);
#pragma unroll
    for (int d = 1; d < RN_WAVE; d <<= 1) {
        const T o = __shfl_up(v, d, RN_WAVE);
        if (lane >= d) v += o;
    }
    return v;
}

// Inclusive scan over a workgroup of NW waves: thread t gets v(0) + ... + v(t), every thread gets the workgroup's sum in `total`.
// `part` holds NW values of LDS.  The WHOLE workgroup must call it: it contains two barriers, and the second one frees `part` for the
// next call.  It may therefore not stand behind a wave-uniform exit that is not also workgroup-uniform; a kernel whose waves leave on
// their own (one wave per item) takes wave_scan_incl only.
template <int NW, typename T>
__device__ __forceinline__ T block_scan_incl(T v, T *part, T &total) {
    const int lane = threadIdx.x & (RN_WAVE - 1), w = threadIdx.x >> 6;
    v = wave_scan_incl(v);
    if (lane == RN_WAVE - 1) part[w] = v;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const T p = part[k];
        if (k < w) before += p;
        total += p;
    }
    __syncthreads();
    return v + before;
}

// ------------------------------------------------------------------------------------------------ min / max
// Every lane gets the wave's minimum / maximum.  double: fmin / fmax, which drop a NaN beside a number; int (maximum only: no kernel
// takes an integer minimum): w > v ? w : v.
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, RN_WAVE));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, RN_WAVE));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, RN_WAVE);
        v = w > v ? w : v;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ arg-reductions
// before(va, ia, vb, ib): does candidate (va, ia) come before (vb, ib)?  Each of these is a strict total order on pairs with distinct
// indices (RN_NO_INDEX last among equals), so a reduction gives the same winner whatever its shape.
// strict <, equal values go to the lower index, a NaN never wins
template <typename T>
struct rn_lt_first {
    __device__ __forceinline__ bool operator()(T va, int ia, T vb, int ib) const { return va < vb || (va == vb && ia < ib); }
};
// strict >, equal values go to the lower index, a NaN never wins
template <typename T>
struct rn_gt_first {
    __device__ __forceinline__ bool operator()(T va, int ia, T vb, int ib) const { return va > vb || (va == vb && ia < ib); }
};
// torch.argmin's order: a NaN is smaller than every number, equal values go to the lower index
template <typename T>
struct torch_argmin_before {
    __device__ __forceinline__ bool operator()(T va, int ia, T vb, int ib) const {
        if (va != va) return (vb != vb) ? ia < ib : true;
        if (vb != vb) return false;
        return va == vb ? ia < ib : va < vb;
    }
};
// torch.argmax's order: a NaN is larger than every number, equal values go to the lower index
template <typename T>
struct torch_argmax_before {
    __device__ __forceinline__ bool operator()(T va, int ia, T vb, int ib) const {
        if (va != va) return (vb != vb) ? ia < ib : true;
        if (vb != vb) return false;
        return va == vb ? ia < ib : va > vb;
    }
};

// Every lane gets the wave's first (val, idx) in the order `before`.
template <typename T, class Before>
__device__ __forceinline__ void wave_arg_first(T &val, int &idx, Before before) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(val, o, RN_WAVE);
        const int oi = __shfl_xor(idx, o, RN_WAVE);
        const bool take = before(ov, oi, val, idx);
        val = take ? ov : val;
        idx = take ? oi : idx;
    }
}
// Every thread of a workgroup of NW waves gets the workgroup's first (val, idx): the wave reduction, one slot per wave in LDS (`sv`,
// `si`: NW entries each), then the slots in wave order.  Called by the whole workgroup; its second barrier frees the slots.
template <int NW, typename T, class Before>
__device__ __forceinline__ void block_arg_first(T &val, int &idx, Before before, T *sv, int *si) {
    wave_arg_first(val, idx, before);
    if ((threadIdx.x & (RN_WAVE - 1)) == 0) { sv[threadIdx.x >> 6] = val; si[threadIdx.x >> 6] = idx; }
    __syncthreads();
    val = sv[0]; idx = si[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const T ov = sv[w];
        const int oi = si[w];
        const bool take = before(ov, oi, val, idx);
        val = take ? ov : val;
        idx = take ? oi : idx;
    }
    __syncthreads();
}
