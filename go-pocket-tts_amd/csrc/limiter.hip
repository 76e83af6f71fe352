// limiter.hip -- a request's look-ahead peak limiter on ragged rows of 24 kHz audio, in place, behind the DSP kernels and in front of k_tp_peak
// (kernels.h LimRow; limiter.h).  Four launches: one wave per workgroup, lane l owns run l of its tile; the
// release is the compressor's (max, times) scan, whose fold, carry and launch pair are dsp_tile.h's (fold_enter_max, carry_max, launch_scan_pair).
//
//   k_lim_summary   one workgroup per full tile that another tile follows: the tile's magnitudes with L samples of halo AHEAD in LDS (8 KB),
//                   every run's hold (lim_hold) and its release end state from p = 0, folded in run order with max (cmp_fold_p) into E_f.
//   k_lim_carry     one workgroup per row: S_0 = 0, S_(f+1) = max(rho^1920 S_f, E_f) in tile order.
//   k_lim_gain      every tile: the hold again, the fold from the tile's entering state, then the run itself -- the release and the required
//                   gain r, one IEEE division rounded once to f32 -- into the row's scratch, one word per sample.
//   k_lim_apply     every tile: r of the tile and of the L samples in front of it (r[0] in front of the row) and the tile's samples in LDS
//                   (16 KB), the box mean in its fixed order (lim_box), one product and one store per sample.  A lane whose windows hold
//                   nothing but 1.0f takes the sum as what it is, L + 1 (lim_box_ones): the same bits.
// The split into gain and apply is what keeps the stage in place without a race: a tile's gain needs x up to 2 L samples beyond its edges, so
// the three kernels that read x across a tile's edge write scratch only, and k_lim_apply, the only one that writes x, reads x in its own
// tile only.  Stream order has each launch complete before the next reads what it wrote.  Nothing at or beyond n is read or written.
#include "device_util.h"
#include "dsp_tile.h"
#include "limiter.h"

namespace ptts {

namespace {

constexpr int kLimLds = kDspTile + kLimMaxAhead;   // floats: a tile and the longest halo

// the magnitudes of samples [base, base + kDspTile + L) into ax; zero at and beyond n
__device__ __forceinline__ void lim_load_mag(const LimRow& r, int64_t base, int L, float* ax) {
    const int have = (int)min((int64_t)(kDspTile + L), r.n - base);
    const float* src = r.x + base;
    for (int q = threadIdx.x; q < kDspTile + L; q += kDspLanes) ax[q] = (q < have) ? lim_mag(src[q]) : 0.0f;
}

__global__ __launch_bounds__(kDspLanes) void k_lim_summary(const LimRow* __restrict__ rows, const LimScan* __restrict__ designs) {
    __shared__ float ax[kLimLds];
    __shared__ double e[kDspLanes];
    const LimRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    const LimScan d = designs[r.design];
    lim_load_mag(r, (int64_t)blockIdx.x * kDspTile, d.L, ax);
    __syncthreads();
    const int l = threadIdx.x;
    float m[kDspRun];
    lim_hold(ax + l * kDspRun, d.L, m);
    e[l] = lim_run_p(d, m, kDspRun, 0.0);
    __syncthreads();
    double E;
    fold_enter_max(d.rho_run, e, 0.0, &E);
    if (l == 0) scan_E<1>(r.p_tiles, blockIdx.x)[0] = E;
}

__global__ __launch_bounds__(kDspLanes) void k_lim_carry(const LimRow* __restrict__ rows, const LimScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const LimRow& r = rows[blockIdx.x];
    if (r.n <= 0) return;
    carry_max(designs[r.design].rho_tile, scan_tiles(r.n), r.p_tiles, ein, nullptr, false);
}

__global__ __launch_bounds__(kDspLanes) void k_lim_gain(const LimRow* __restrict__ rows, const LimScan* __restrict__ designs) {
    __shared__ float ax[kLimLds];
    __shared__ double e[kDspLanes];
    const LimRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const LimScan d = designs[r.design];
    lim_load_mag(r, base, d.L, ax);
    __syncthreads();
    const int l = threadIdx.x, c = run_count(cnt);
    float m[kDspRun];
    lim_hold(ax + l * kDspRun, d.L, m);
    e[l] = lim_run_p(d, m, c, 0.0);
    __syncthreads();   // (every lane has read its windows: ax may be written)
    double behind;
    const double tp = fold_enter_max(d.rho_run, e, scan_S<1>(r.p_tiles, blockIdx.x)[0], &behind);
    lim_run_r(d, m, c, tp, ax + l * kDspRun);
    __syncthreads();
    float* dst = r.r + base;
    for (int q = threadIdx.x; q < cnt; q += kDspLanes) dst[q] = ax[q];
}

__global__ __launch_bounds__(kDspLanes) void k_lim_apply(const LimRow* __restrict__ rows, const LimScan* __restrict__ designs) {
    __shared__ float rr[kLimLds];      // r[base - L, base + cnt) at rr[0, L + cnt)
    __shared__ float tile[kDspTile];
    const LimRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const LimScan d = designs[r.design];
    const int L = d.L;
    for (int q = threadIdx.x; q < L + cnt; q += kDspLanes) {
        const int64_t i = base - L + q;
        rr[q] = r.r[i < 0 ? 0 : i];
    }
    float* x = r.x + base;
    for (int q = threadIdx.x; q < cnt; q += kDspLanes) tile[q] = x[q];
    __syncthreads();
    const int l = threadIdx.x, c = run_count(cnt);
    if (c > 0) {
        const float* mine = rr + l * kDspRun;   // the run's windows: mine[0, L + c)
        bool ones = true;
        for (int q = 0; q < L + c; q++) ones = ones && (mine[q] == 1.0f);
        float* run = tile + l * kDspRun;
        if (ones) {
            const double g = lim_box_ones(d);
            for (int i = 0; i < c; i++) run[i] = lim_out(d, run[i], g);
        } else {
            for (int i = 0; i < c; i++) run[i] = lim_out(d, run[i], lim_box(d, mine + L + i));
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < cnt; q += kDspLanes) x[q] = tile[q];
}

}  // namespace

void launch_limiter(const LimRow* rows_dev, int n, int max_tiles, const LimScan* designs_dev, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    const dim3 tiles((unsigned)max_tiles, (unsigned)n), lanes(kDspLanes);
    launch_scan_pair("k_lim_summary", k_lim_summary, "k_lim_carry", k_lim_carry, max_tiles - 1, n, stream, rows_dev, designs_dev);
    note_launch("k_lim_gain");
    hipLaunchKernelGGL(k_lim_gain, tiles, lanes, 0, stream, rows_dev, designs_dev);
    note_launch("k_lim_apply");
    hipLaunchKernelGGL(k_lim_apply, tiles, lanes, 0, stream, rows_dev, designs_dev);
}

}  // namespace ptts
