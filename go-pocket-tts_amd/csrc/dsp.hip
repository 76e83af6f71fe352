// dsp.hip -- ptts_dsp_apply's chain on the device (kernels.h DspRow): peak normalise, DC block, fade in, fade out
// on ragged rows of decoded 24 kHz audio, in place, in front of k_resample.
//
//   k_dsp_peak     normalise rows: max |x| of the row.  A max is order-independent and non-negative floats order like their bit patterns, so
//                  the workgroups' atomicMax on the uint32 image gives the host's peak whatever the schedule.  NaNs never win (as on the host).
//   k_dsp_summary  DC rows: one workgroup per full tile that another tile follows; lane l runs run l from zero state, lane 0 folds the 64
//                  end states in run order into E_f (dsp_block.h).
//   k_dsp_carry    DC rows: one workgroup per row; S_0 = 0, S_(f+1) = A^1920 S_f + E_f in tile order.
//   k_dsp_apply    every tile: gain (an IEEE f32 division, one f32 product per sample), the runs' recurrence from their entering states
//                  (t_0 = S_f, t_(l+1) = A^30 t_l + e_l in run order), the rounding to f32, the two fade gains as two f32 products, one store.
// The filter's input is the f32 product x * gain wherever it is read, so the peak is complete before k_dsp_summary starts (stream order).
// Tiles lie on the row's own grid: a row's bits are a function of the row alone.  Nothing at or beyond n is read or written.
// A loudness row (DSP_LOUD, loudness.hip) has its gain in a word k_loud_gate wrote; k_dsp_summary and k_dsp_apply are templates on whether the
// table has such a row, so a table without one launches the instantiation that does not know the flag: the code it ran before the flag existed.
#include "device_util.h"
#include "dsp_block.h"

namespace ptts {

namespace {

constexpr int kPeakThreads = 256, kPeakChunk = 4 * kDspTile;

struct Gain { bool on; float g; };
template <bool LOUD>
__device__ __forceinline__ Gain row_gain(const DspRow& r) {   // dsp_peak_normalize: gain = 1.0f / peak, a row of zeros stays as it is
    if (LOUD && (r.flags & DSP_LOUD)) {   // loud_measure_gain's: a gain of 1 leaves the samples as they are
        const float g = *reinterpret_cast<const float*>(r.loud + 1);
        return Gain{g != 1.0f, g};
    }
    if (!(r.flags & DSP_NORMALIZE)) return Gain{false, 1.0f};
    const float peak = __uint_as_float(*r.peak);
    if (peak == 0.0f) return Gain{false, 1.0f};
    return Gain{true, __fdiv_rn(1.0f, peak)};
}

// samples [base, base + cnt) of the row into tile[0, cnt), times the gain; 16-byte loads where the row's alignment allows
__device__ __forceinline__ void load_tile(const DspRow& r, int64_t base, int cnt, float* tile, const Gain g) {
    const float* src = r.x + base;
    const bool vec = ((uintptr_t)src & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) {
            float4 v = *reinterpret_cast<const float4*>(src + q);
            if (g.on) { v.x = v.x * g.g; v.y = v.y * g.g; v.z = v.z * g.g; v.w = v.w * g.g; }
            *reinterpret_cast<float4*>(tile + q) = v;
        } else {
            for (int u = 0; u < 4 && q + u < cnt; u++) tile[q + u] = g.on ? src[q + u] * g.g : src[q + u];
        }
    }
}

__global__ __launch_bounds__(kPeakThreads) void k_dsp_peak(const DspRow* __restrict__ rows) {
    __shared__ float part[kPeakThreads / WAVE];
    const DspRow& r = rows[blockIdx.y];
    if (!(r.flags & (DSP_NORMALIZE | DSP_LOUD))) return;
    const int64_t i0 = (int64_t)blockIdx.x * kPeakChunk;
    if (i0 >= r.n) return;
    const int64_t i1 = min(i0 + (int64_t)kPeakChunk, r.n);
    const bool vec = ((uintptr_t)r.x & 15) == 0;
    float pk = 0.0f;
    for (int64_t q = i0 + (int64_t)threadIdx.x * 4; q < i1; q += kPeakThreads * 4) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec && q + 4 <= i1) {
            const float4 w = *reinterpret_cast<const float4*>(r.x + q);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
            for (int u = 0; u < 4 && q + u < i1; u++) v[u] = r.x[q + u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { const float a = fabsf(v[u]); if (a > pk) pk = a; }
    }
    pk = wave_max(pk);   // (pk is never NaN)
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = pk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kPeakThreads / WAVE; w++) pk = fmaxf(pk, part[w]);
        if (pk > 0.0f) atomicMax(r.peak, __float_as_uint(pk));
    }
}

template <bool LOUD>
__global__ __launch_bounds__(kDspLanes) void k_dsp_summary(const DspRow* __restrict__ rows, const DspScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes][2];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_DC) || base + kDspTile >= r.n) return;   // only a full tile that another one follows hands a state on
    load_tile(r, base, kDspTile, tile, row_gain<LOUD>(r));
    __syncthreads();
    const int l = threadIdx.x;
    double z1 = 0.0, z2 = 0.0;
    dsp_run(sc.c, tile + l * kDspRun, nullptr, kDspRun, z1, z2);
    e[l][0] = z1; e[l][1] = z2;
    __syncthreads();
    if (l == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < kDspLanes; j++) dsp_advance(sc.a_run, s1, s2, e[j][0], e[j][1]);
        r.tiles[(int64_t)blockIdx.x * 4 + 0] = s1;
        r.tiles[(int64_t)blockIdx.x * 4 + 1] = s2;
    }
}

__global__ __launch_bounds__(kDspLanes) void k_dsp_carry(const DspRow* __restrict__ rows, const DspScan sc) {
    __shared__ double ein[kDspLanes][2], sout[kDspLanes][2];
    const DspRow& r = rows[blockIdx.x];
    if (!(r.flags & DSP_DC) || r.n <= 0) return;
    const int64_t F = (r.n + kDspTile - 1) / kDspTile;
    const int l = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;   // lane 0's: the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < F - 1) { ein[l][0] = r.tiles[f * 4 + 0]; ein[l][1] = r.tiles[f * 4 + 1]; }
        __syncthreads();
        if (l == 0) {
            const int m = (int)min((int64_t)kDspLanes, F - c0);
            for (int j = 0; j < m; j++) {
                sout[j][0] = s1; sout[j][1] = s2;
                if (c0 + j < F - 1) dsp_advance(sc.a_tile, s1, s2, ein[j][0], ein[j][1]);
            }
        }
        __syncthreads();
        if (f < F) { r.tiles[f * 4 + 2] = sout[l][0]; r.tiles[f * 4 + 3] = sout[l][1]; }
        __syncthreads();
    }
}

template <bool LOUD>
__global__ __launch_bounds__(kDspLanes) void k_dsp_apply(const DspRow* __restrict__ rows, const DspScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes][2], t[kDspLanes][2];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const Gain g = row_gain<LOUD>(r);
    const bool dc = (r.flags & DSP_DC) != 0;
    const int64_t fin = r.fade_in, fout0 = n - r.fade_out;   // fade in below fin, fade out from fout0 on
    if (!g.on && !dc && base >= fin && base + cnt <= fout0) return;   // a tile that no step changes
    load_tile(r, base, cnt, tile, g);
    __syncthreads();
    if (dc) {
        const int l = threadIdx.x;
        const int c = max(0, min(kDspRun, cnt - l * kDspRun));
        double z1 = 0.0, z2 = 0.0;
        dsp_run(sc.c, tile + l * kDspRun, nullptr, c, z1, z2);
        e[l][0] = z1; e[l][1] = z2;
        __syncthreads();
        if (l == 0) {   // (behind a run that is not full no run follows: its t is not read)
            double s1 = r.tiles[(int64_t)blockIdx.x * 4 + 2], s2 = r.tiles[(int64_t)blockIdx.x * 4 + 3];
            for (int j = 0; j < kDspLanes; j++) {
                t[j][0] = s1; t[j][1] = s2;
                dsp_advance(sc.a_run, s1, s2, e[j][0], e[j][1]);
            }
        }
        __syncthreads();
        z1 = t[l][0]; z2 = t[l][1];
        dsp_run(sc.c, tile + l * kDspRun, tile + l * kDspRun, c, z1, z2);
        __syncthreads();
    }
    float* dst = r.x + base;
    const bool vec = ((uintptr_t)dst & 15) == 0;
    const float fin_f = (float)fin, fout_f = (float)r.fade_out;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        float v[4];
        const int nv = min(4, cnt - q);
        for (int u = 0; u < nv; u++) {
            const int64_t i = base + q + u;
            float s = tile[q + u];
            if (i < fin) s = s * __fdiv_rn((float)i, fin_f);                      // dsp_fade_in
            if (i >= fout0) s = s * __fdiv_rn((float)(n - 1 - i), fout_f);        // dsp_fade_out
            v[u] = s;
        }
        if (vec && nv == 4) *reinterpret_cast<float4*>(dst + q) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int u = 0; u < nv; u++) dst[q + u] = v[u];
    }
}

}  // namespace

void launch_dsp(const DspRow* rows_dev, int n, int max_tiles, bool any_norm, bool any_dc, const DspScan& scan, hipStream_t stream, bool any_loud,
                const LoudScan* loud, bool apply) {
    if (n <= 0 || max_tiles <= 0) return;
    if (any_norm || (any_loud && apply)) {   // (a measurement alone has no ceiling to keep)
        note_launch("k_dsp_peak");
        hipLaunchKernelGGL(k_dsp_peak, dim3((unsigned)((max_tiles + 3) / 4), (unsigned)n), dim3(kPeakThreads), 0, stream, rows_dev);
    }
    if (any_loud) launch_loudness(rows_dev, n, max_tiles, *loud, stream);
    if (!apply) return;
    if (any_dc) {
        if (max_tiles > 1) {
            note_launch("k_dsp_summary");
            hipLaunchKernelGGL(any_loud ? k_dsp_summary<true> : k_dsp_summary<false>, dim3((unsigned)(max_tiles - 1), (unsigned)n), dim3(kDspLanes), 0, stream,
                               rows_dev, scan);
        }
        note_launch("k_dsp_carry");
        hipLaunchKernelGGL(k_dsp_carry, dim3((unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
    }
    note_launch("k_dsp_apply");
    hipLaunchKernelGGL(any_loud ? k_dsp_apply<true> : k_dsp_apply<false>, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
}

}  // namespace ptts
