// formant.hip -- "keep the formants" around the pitch's resampling step of the parts of a joined text, on ragged rows of 24 kHz audio (kernels.h
// FormantRow; formant.h has the rule and the chains, formant.cpp is the host statement and gives the bits).
//
//   k_formant_analyse  workgroup (x, y) of 256 threads: wave w on frame 4 x + w of row y.  The wave stages its windowed frame in LDS as float64
//                      (v[j] = (double)x * w[j], the table from the host), lanes 0 .. 24 run the 25 lag chains -- lane l reads v[j] beside its
//                      neighbours and v[j - l] as a broadcast -- and lane 0 runs Levinson-Durbin in registers (every index static) and stores the frame's 24 floats.
//   k_formant_whiten   workgroup (x, y) of 256 threads on tile x of row y: the samples [240 x - 120, 240 x + 120), which have one frame pair
//                      (x - 1, x, clamped).  The row's window (24 samples in front of the tile too) and both coefficient sets sit in LDS; thread t
//                      runs both chains of sample 240 x - 120 + t and mixes them.
//   k_formant_shape    workgroup (x, y) of ONE wave on 16 consecutive output tiles of row y: lane 4 i + s runs the recursion of the s-th frame that
//                      tile 16 x + i names, 960 samples of 24 dependent fused multiply-adds, its 24-sample history in registers under static
//                      indices (the sample loop is unrolled by 24).  The 16 tiles' residual, [240 (16 x) - 720, 240 (16 x + 16)), is staged in LDS
//                      once, with one unused float behind every 240: at a step the 16 tiles read 241 floats apart, on 16 different banks (240
//                      apart would be 4 banks), and a tile's four lanes read one word.  Over a tile's last 240 steps the four lanes exchange
//                      their samples (a lane shuffle inside the quad), every lane mixes the pair the output names, lane s == 0 keeps it in LDS,
//                      and the wave stores the 16 tiles coalesced at the end.
// Nothing is atomic and nothing is cleared beforehand; every sample and coefficient is written once, by one thread; nothing outside a row is
// read and nothing behind it is written.  Sample indices are 64-bit.  Every fused multiply-add is written as such; contraction is off elsewhere.
#include "device_util.h"
#include "formant.h"
#include "kernels.h"

namespace ptts {

namespace {

constexpr int kAnalyseWaves = kFormantAnalyseThreads / 64;
constexpr int kShapeSeg = kFormantHop + 1;                                         // a tile's floats in LDS and the unused one behind them
constexpr int kShapeSegs = kFormantShapeTiles + kFormantWarm / kFormantHop;        // the segments a wave's window holds
constexpr int kShapeBlocks = (kFormantWarm + kFormantHop) / kFormantOrder;         // runs of 24 samples a recursion takes
constexpr int kShapeQuiet = kFormantWarm / kFormantOrder;                          // ... of which the first warm up and store nothing
static_assert(kFormantHop % kFormantOrder == 0 && kFormantWarm % kFormantHop == 0, "a run of 24 samples stays inside one segment");
static_assert(kFormantSlots == 4 && kFormantShapeTiles * kFormantSlots == 64, "a quad of lanes a tile, one wave a workgroup");

__global__ __launch_bounds__(kFormantAnalyseThreads) void k_formant_analyse(const FormantRow* __restrict__ rows, const double* __restrict__ tables) {
    __shared__ double v[kAnalyseWaves][kFormantWin];
    __shared__ double lags[kAnalyseWaves][kFormantOrder + 1];
    const FormantRow r = rows[blockIdx.y];
    if ((int64_t)blockIdx.x * kAnalyseWaves >= r.K) return;   // (the same for the whole workgroup)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * kAnalyseWaves + wv;
    const bool on = f < r.K;
    if (on) {
        const int64_t at = kFormantHop * f - kFormantHop;
        for (int j = lane; j < kFormantWin; j += 64) {
            const int64_t i = at + j;
            const float s = i >= 0 && i < r.n ? r.x[i] : 0.0f;
            v[wv][j] = (double)s * tables[j];
        }
    }
    __syncthreads();
    if (on && lane <= kFormantOrder) lags[wv][lane] = formant_lag(v[wv], lane);
    __syncthreads();
    if (on && lane == 0)
        formant_solve(lags[wv], tables + kFormantWin, tables + kFormantWin + kFormantOrder + 1, r.coeffs + f * kFormantOrder);
}

__global__ __launch_bounds__(kFormantWhitenThreads) void k_formant_whiten(const FormantRow* __restrict__ rows) {
    __shared__ float win[kFormantOrder + kFormantHop];
    __shared__ float ca[kFormantOrder], cb[kFormantOrder];
    const FormantRow r = rows[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * kFormantHop - kFormantHop / 2;
    if (i0 >= r.n) return;   // (the same for the whole workgroup)
    const int t = threadIdx.x;
    const int64_t K = r.K;
    for (int k = t; k < kFormantOrder + kFormantHop; k += kFormantWhitenThreads) {
        const int64_t at = i0 - kFormantOrder + k;
        win[k] = at >= 0 && at < r.n ? r.x[at] : 0.0f;
    }
    const FormantPair tile = formant_pair(i0 < 0 ? 0 : i0, K);   // (the pair of every sample of the tile)
    if (t < kFormantOrder) ca[t] = r.coeffs[tile.fa * kFormantOrder + t];
    else if (t < 2 * kFormantOrder) cb[t - kFormantOrder] = r.coeffs[tile.fb * kFormantOrder + (t - kFormantOrder)];
    __syncthreads();
    const int64_t i = i0 + t;
    if (t >= kFormantHop || i < 0 || i >= r.n) return;
    const auto at = [&](int64_t m) { return win[(int)(m - i0) + kFormantOrder]; };
    const float A = formant_residual(ca, at, i);
    const float B = formant_residual(cb, at, i);
    r.e[i] = formant_mix(A, B, formant_pair(i, K).u);
}

// one run of 24 samples of a lane's recursion: src the run's residual, na the negated coefficients, h the history (h[u]: the run's sample u, and
// the sample 24 in front of it until that is computed).  EMIT: the run lies in the lane's tile, rr0 is its first output there
template <bool EMIT>
__device__ __forceinline__ void shape_run(const float* src, const float (&na)[kFormantOrder], float (&h)[kFormantOrder], int rr0, int lane, int slot,
                                          int32_t p, int64_t tq, uint32_t tr, int64_t K, int64_t f_lo, float* keep) {
#pragma unroll
    for (int u = 0; u < kFormantOrder; u++) {
        float acc = src[u];
#pragma unroll
        for (int k = 1; k <= kFormantOrder; k++) acc = __builtin_fmaf(na[k - 1], h[(u - k + 2 * kFormantOrder) % kFormantOrder], acc);
        h[u] = acc;
        if (EMIT) {
            // formant_pair of tau = (j * p) / 1000, in 32 bits: tau is below 2^31 (a row's length is), and the integers are the same
            const int rr = rr0 + u;
            const int tau = (int)(tq + (int64_t)((tr + (uint32_t)rr * (uint32_t)p) / 1000u));
            const int b = tau - kFormantHop / 2;
            const int f0 = b >= 0 ? b / kFormantHop : -((-b + kFormantHop - 1) / kFormantHop);
            const int rho = b - kFormantHop * f0;
            const int64_t fa = f0 < 0 ? 0 : f0 > K - 1 ? K - 1 : f0;
            const int64_t fb = f0 + 1 < 0 ? 0 : f0 + 1 > K - 1 ? K - 1 : f0 + 1;
            const float ya = __shfl(acc, (lane & ~3) + ((int)(fa - f_lo) & 3));
            const float yb = __shfl(acc, (lane & ~3) + ((int)(fb - f_lo) & 3));
            const float o = formant_mix(ya, yb, __fdiv_rn((float)rho, 240.0f));
            if (slot == 0) keep[rr] = o;
        }
    }
}

__global__ __launch_bounds__(64) void k_formant_shape(const FormantRow* __restrict__ rows) {
    __shared__ float win[kShapeSegs * kShapeSeg];
    __shared__ float obuf[kFormantShapeTiles * kShapeSeg];
    const FormantRow r = rows[blockIdx.y];
    const int64_t t0 = (int64_t)blockIdx.x * kFormantShapeTiles;
    if (t0 * kFormantHop >= r.n_r) return;   // (the same for the whole workgroup)
    const int lane = threadIdx.x, ti = lane >> 2, slot = lane & 3;
    const int64_t w0 = t0 * kFormantHop - kFormantWarm;
    for (int k = lane; k < kShapeSegs * kFormantHop; k += 64) {
        const int64_t m = w0 + k;
        win[k + k / kFormantHop] = m >= 0 && m < r.n_r ? r.er[m] : 0.0f;
    }
    const int64_t K = r.K;
    const int64_t j0 = (t0 + ti) * kFormantHop;
    const int64_t f_lo = j0 < r.n_r ? formant_tile_first(j0, r.p, K) : 0;
    const int64_t f = f_lo + slot > K - 1 ? K - 1 : f_lo + slot;
    float na[kFormantOrder], h[kFormantOrder];
#pragma unroll
    for (int k = 0; k < kFormantOrder; k++) {
        na[k] = -r.coeffs[f * kFormantOrder + k];
        h[k] = 0.0f;
    }
    const int64_t c0 = j0 * (int64_t)r.p, tq = c0 / 1000;
    const uint32_t tr = (uint32_t)(c0 - tq * 1000);
    __syncthreads();
    const float* const mine = win + kShapeSeg * ti;   // the lane's first sample: 720 in front of its tile
    float* const keep = obuf + kShapeSeg * ti;
    for (int b = 0; b < kShapeQuiet; b++)
        shape_run<false>(mine + kFormantOrder * b + b / (kFormantHop / kFormantOrder), na, h, 0, lane, slot, r.p, tq, tr, K, f_lo, keep);
    for (int b = kShapeQuiet; b < kShapeBlocks; b++)
        shape_run<true>(mine + kFormantOrder * b + b / (kFormantHop / kFormantOrder), na, h, kFormantOrder * (b - kShapeQuiet), lane, slot, r.p, tq, tr, K, f_lo, keep);
    __syncthreads();
    for (int i = 0; i < kFormantShapeTiles; i++) {
        const int64_t at = (t0 + i) * kFormantHop;
        for (int rr = lane; rr < kFormantHop; rr += 64)
            if (at + rr < r.n_r) r.out[at + rr] = obuf[kShapeSeg * i + rr];
    }
}

}  // namespace

void launch_formant_analyse(const FormantRow* rows_dev, int n, int64_t max_frames, const double* tables_dev, hipStream_t stream) {
    if (n <= 0 || max_frames <= 0) return;
    note_launch("k_formant_analyse");
    hipLaunchKernelGGL(k_formant_analyse, dim3((unsigned)((max_frames + kAnalyseWaves - 1) / kAnalyseWaves), (unsigned)n), dim3(kFormantAnalyseThreads), 0, stream,
                       rows_dev, tables_dev);
}

void launch_formant_whiten(const FormantRow* rows_dev, int n, int64_t max_tiles, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_formant_whiten");
    hipLaunchKernelGGL(k_formant_whiten, dim3((unsigned)max_tiles, (unsigned)n), dim3(kFormantWhitenThreads), 0, stream, rows_dev);
}

void launch_formant_shape(const FormantRow* rows_dev, int n, int64_t max_tiles, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_formant_shape");
    hipLaunchKernelGGL(k_formant_shape, dim3((unsigned)((max_tiles + kFormantShapeTiles - 1) / kFormantShapeTiles), (unsigned)n), dim3(64), 0, stream, rows_dev);
}

}  // namespace ptts
