// compressor.hip -- a request's dynamic range compressor on ragged rows of decoded 24 kHz audio, in place, in front of the DSP kernels (kernels.h
// CmpRow; compressor.h).  Five launches, shaped like dsp.hip's k_eq_*: one wave per workgroup, lane l owns run l of
// its tile, the tile sits in LDS (7.5 KB, plus 0.5 KB of run states).
//
//   k_cmp_summary_p   one workgroup per full tile that another tile follows: every run's detector end state from p = 0, folded in run order with
//                     max (cmp_fold_p) into E_f.
//   k_cmp_carry_p     one workgroup per row: S_0 = 0, S_(f+1) = max(rho^1920 S_f, E_f) in tile order.
//   k_cmp_summary_s   the same tiles: the detector state entering every run (the fold from S_f), every run's smoothing end state from s = 0 with
//                     the detector recomputed from its entering state, folded in run order (scan_advance<1>) into the smoothing's E_f.
//   k_cmp_carry_s     one workgroup per row: S_0 = 0, S_(f+1) = alpha^1920 S_f + E_f in tile order.
//   k_cmp_apply       every tile: both folds again from the tile's entering states, then the run itself -- detector, smoothing, the gain curve,
//                     the product rounded once to f32 -- and one store.
// Every fold is evaluated by all 64 lanes alike from LDS (a broadcast read; one product and one max or sum per step), lane l keeping the value
// it meets at step l: the order is the host's (compressor.cpp cmp_apply_blocked), and so are the bits.  The stride-30 run access is the 2-way
// bank pattern k_eq_apply lives with.  Stream order has each launch complete before the next reads what it wrote; the summaries and k_cmp_apply
// read the raw samples, only k_cmp_apply writes them, every workgroup its own tile.  Nothing at or beyond n is read or written.
// A launch may cover a window of a row (kernels.h CmpRow::t0, ::open, ::carry; dsp_tile.h): both carries start from the states the window in front
// left and leave theirs behind an open window's last tile, which the summaries then cover; nothing in front of the window is written.
#include "device_util.h"
#include "dsp_tile.h"

namespace ptts {

namespace {

__global__ __launch_bounds__(kDspLanes) void k_cmp_summary_p(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes];
    const CmpRow& r = rows[blockIdx.y];
    if (!tile_hands_on(r.t0, r.n, r.open)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    tile_load(r.x + (r.t0 + blockIdx.x) * kDspTile, kDspTile, tile);
    __syncthreads();
    const CmpScan d = designs[r.design];
    const int l = threadIdx.x;
    e[l] = cmp_run_p(d, tile + l * kDspRun, kDspRun, 0.0);
    __syncthreads();
    double E;
    fold_enter_max(d.rho_run, e, 0.0, &E);
    if (l == 0) scan_E<1>(r.p_tiles, blockIdx.x)[0] = E;
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_carry_p(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const CmpRow& r = rows[blockIdx.x];
    if (win_tiles(r.t0, r.n) <= 0) return;
    carry_one<true>(designs[r.design].rho_tile, win_tiles(r.t0, r.n), r.p_tiles, ein, r.carry ? r.carry + kCarryCmpP : nullptr, r.open);
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_summary_s(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes];
    const CmpRow& r = rows[blockIdx.y];
    if (!tile_hands_on(r.t0, r.n, r.open)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    tile_load(r.x + (r.t0 + blockIdx.x) * kDspTile, kDspTile, tile);
    __syncthreads();
    const CmpScan d = designs[r.design];
    const int l = threadIdx.x;
    const float* run = tile + l * kDspRun;
    e[l] = cmp_run_p(d, run, kDspRun, 0.0);
    __syncthreads();
    double behind;
    const double tp = fold_enter_max(d.rho_run, e, scan_S<1>(r.p_tiles, blockIdx.x)[0], &behind);
    __syncthreads();
    e[l] = cmp_run_s(d, run, kDspRun, tp, 0.0);
    __syncthreads();
    double E;
    fold_enter_sum(d.alpha_run, e, 0.0, &E);
    if (l == 0) scan_E<1>(r.s_tiles, blockIdx.x)[0] = E;
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_carry_s(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const CmpRow& r = rows[blockIdx.x];
    if (win_tiles(r.t0, r.n) <= 0) return;
    carry_one<false>(designs[r.design].alpha_tile, win_tiles(r.t0, r.n), r.s_tiles, ein, r.carry ? r.carry + kCarryCmpS : nullptr, r.open);
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_apply(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes];
    const CmpRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (r.t0 + blockIdx.x) * kDspTile;
    if (base >= n) return;
    float* tile = reinterpret_cast<float*>(tile4);
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    tile_load(r.x + base, cnt, tile);
    __syncthreads();
    const CmpScan d = designs[r.design];
    const int l = threadIdx.x, c = run_count(cnt);
    float* run = tile + l * kDspRun;
    e[l] = cmp_run_p(d, run, c, 0.0);
    __syncthreads();
    double behind;
    const double tp = fold_enter_max(d.rho_run, e, scan_S<1>(r.p_tiles, blockIdx.x)[0], &behind);
    __syncthreads();
    e[l] = cmp_run_s(d, run, c, tp, 0.0);
    __syncthreads();
    const double ts = fold_enter_sum(d.alpha_run, e, scan_S<1>(r.s_tiles, blockIdx.x)[0], &behind);
    cmp_run_y(d, run, c, tp, ts, run);
    __syncthreads();
    tile_store(r.x + base, cnt, tile);
}

}  // namespace

void launch_compressor(const CmpRow* rows_dev, int n, int max_tiles, const CmpScan* designs_dev, hipStream_t stream, bool any_open) {
    if (n <= 0 || max_tiles <= 0) return;
    const int hands = any_open ? max_tiles : max_tiles - 1;   // (an open window's last tile hands on as well)
    const dim3 tiles((unsigned)max_tiles, (unsigned)n), handing((unsigned)hands, (unsigned)n), lanes(kDspLanes);
    if (hands > 0) {
        note_launch("k_cmp_summary_p");
        hipLaunchKernelGGL(k_cmp_summary_p, handing, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_cmp_carry_p");
    hipLaunchKernelGGL(k_cmp_carry_p, dim3((unsigned)n), lanes, 0, stream, rows_dev, designs_dev);
    if (hands > 0) {
        note_launch("k_cmp_summary_s");
        hipLaunchKernelGGL(k_cmp_summary_s, handing, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_cmp_carry_s");
    hipLaunchKernelGGL(k_cmp_carry_s, dim3((unsigned)n), lanes, 0, stream, rows_dev, designs_dev);
    note_launch("k_cmp_apply");
    hipLaunchKernelGGL(k_cmp_apply, tiles, lanes, 0, stream, rows_dev, designs_dev);
}

}  // namespace ptts
