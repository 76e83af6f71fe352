// true_peak.hip -- the true-peak ceiling of ragged rows of 24 kHz audio on the device, the last stage of the post-processing chain (kernels.h
// DspRow, DSP_TP rows; true_peak.h).  dsp_launch (dsp_device.cpp) launches both behind the table's last kernel, k_tp_peak alone for a measurement.
//
//   k_tp_peak    grid (tile, row), kTpThreads = 256 threads.  A tile is kDspTile samples on the row's own grid.  The workgroup stages its tile
//                with the 26 samples in front and the 27 behind into LDS, zeros outside [0, n); lane l then takes the samples l, l + 256, ... of
//                the tile -- eight of them, so neighbouring lanes read neighbouring LDS words -- and runs true_peak.h's tp_step on all eight
//                side by side: 64 independent fmaf chains, each window word shared by a sample's eight phases and each tap by all 64.  There
//                is no recurrence and no loop: the taps come by value in the kernel arguments and are the same in every lane, so a step's
//                eight are loaded by scalar loads where it needs them, and no more than a few steps' taps are held at a time.  wave_max, the waves' maxima through
//                LDS, then one atomicMax on the row's zeroed word -- non-negative floats order like their uint32 images, as in k_dsp_peak.
//                NaNs never win.
//   k_tp_scale   grid (tile, row).  Rows whose word is <= the ceiling c return at once; the others become x * g with g = c / TP (an IEEE f32
//                division), 16-byte loads and stores where the row's alignment allows.
// A max has no order and an fmaf chain rounds where the host's rounds: a row's word is ptts_true_peak's bits and its samples are
// ptts_true_peak_limit's.  Nothing at or beyond n is read or written.
#include "device_util.h"
#include "true_peak.h"

namespace ptts {

namespace {

// the tile's window in LDS: its samples from word kTpBody on (16-byte aligned, for the 16-byte loads), the halo in front of and behind them
constexpr int kTpBody = 28, kTpWindow = kTpBody + kDspTile + 28;
static_assert(kTpBody >= kTpBefore && kTpBody % 4 == 0 && kTpWindow % 4 == 0 && kTpWindow >= kTpBody + kDspTile + kTpAfter, "the halo fits");
constexpr int kTpThreads = 256, kTpEach = (kDspTile + kTpThreads - 1) / kTpThreads;   // samples per lane: 8 (the last of them in half the lanes)
static_assert(kTpBefore + kTpAfter <= kTpThreads, "a lane per halo sample");

__global__ __launch_bounds__(kTpThreads) void k_tp_peak(const DspRow* __restrict__ rows, const TpTaps taps) {
    __shared__ float4 win4[kTpWindow / 4];
    __shared__ float part[kTpThreads / WAVE];
    float* win = reinterpret_cast<float*>(win4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_TP) || base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base), l = threadIdx.x;
    if (l < kTpBefore) {
        const int64_t i = base - kTpBefore + l;
        win[kTpBody - kTpBefore + l] = i >= 0 ? r.x[i] : 0.0f;
    } else if (l < kTpBefore + kTpAfter) {
        const int64_t i = base + cnt + (l - kTpBefore);
        win[kTpBody + cnt + (l - kTpBefore)] = i < n ? r.x[i] : 0.0f;
    }
    const float* src = r.x + base;
    const bool vec = ((uintptr_t)src & 15) == 0;
    for (int q = l * 4; q < cnt; q += kTpThreads * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(win + kTpBody + q) = *reinterpret_cast<const float4*>(src + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) win[kTpBody + q + u] = src[q + u];
    }
    __syncthreads();
    // the lane's samples; one past the tile's end stands for the tile's last sample again, which changes no maximum.  The window of sample i
    // starts kTpBefore words in front of it.
    const float* w[kTpEach];
    float acc[kTpEach][kTpPhases], pk = 0.0f;
#pragma unroll
    for (int j = 0; j < kTpEach; j++) {
        const int i = min(l + j * kTpThreads, cnt - 1);
        w[j] = win + kTpBody - kTpBefore + i;
        const float a = fabsf(win[kTpBody + i]);
        if (a > pk) pk = a;
#pragma unroll
        for (int p = 0; p < kTpPhases; p++) acc[j][p] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < kTpTaps; k++) {
        float xv[kTpEach];
#pragma unroll
        for (int j = 0; j < kTpEach; j++) xv[j] = w[j][k];
        tp_step<kTpEach>(acc, xv, taps.h[k]);
    }
    pk = wave_max(tp_fold<kTpEach>(acc, pk));   // (pk is never NaN)
    if ((l & (WAVE - 1)) == 0) part[l / WAVE] = pk;
    __syncthreads();
    if (l == 0) {
        for (int v = 1; v < kTpThreads / WAVE; v++) pk = fmaxf(pk, part[v]);
        if (pk > 0.0f) atomicMax(r.tp, __float_as_uint(pk));
    }
}

__global__ __launch_bounds__(kDspLanes) void k_tp_scale(const DspRow* __restrict__ rows) {
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_TP) || base >= n) return;
    const float tp = __uint_as_float(*r.tp), c = r.ceiling;
    if (!(tp > c)) return;   // under the ceiling: the row is not written
    const float g = __fdiv_rn(c, tp);
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    float* dst = r.x + base;
    const bool vec = ((uintptr_t)dst & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) {
            float4 v = *reinterpret_cast<const float4*>(dst + q);
            v.x = v.x * g; v.y = v.y * g; v.z = v.z * g; v.w = v.w * g;
            *reinterpret_cast<float4*>(dst + q) = v;
        } else {
            for (int u = 0; u < 4 && q + u < cnt; u++) dst[q + u] = dst[q + u] * g;
        }
    }
}

}  // namespace

void launch_tp_peak(const DspRow* rows_dev, int n, int max_tiles, const TpTaps& taps, hipStream_t stream) {
    note_launch("k_tp_peak");
    hipLaunchKernelGGL(k_tp_peak, dim3((unsigned)max_tiles, (unsigned)n), dim3(kTpThreads), 0, stream, rows_dev, taps);
}

void launch_tp_scale(const DspRow* rows_dev, int n, int max_tiles, hipStream_t stream) {
    note_launch("k_tp_scale");
    hipLaunchKernelGGL(k_tp_scale, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev);
}

}  // namespace ptts
