// compressor.hip -- a request's dynamic range compressor on ragged rows of decoded 24 kHz audio, in place, in front of the DSP kernels (kernels.h
// CmpRow; compressor.h).  Five launches: one wave per workgroup, lane l owns run l of its tile, the tile sits in LDS
// (7.5 KB, plus 0.5 KB of run states).  The detector on a tile -- its folds, their barriers, the smoothing as the linear scan with N = 1 -- is
// dsp_tile.h's (det_*, carry_max, scan_carry); here it is given the tile's own samples.
//
//   k_cmp_summary_p   one workgroup per full tile that another tile follows: the detector's E_f (det_summary_p).
//   k_cmp_carry_p     one workgroup per row: the detector's S_f in tile order (carry_max).
//   k_cmp_summary_s   the same tiles: the smoothing's E_f, the detector recomputed from the state entering every run (det_summary_s).
//   k_cmp_carry_s     one workgroup per row: the smoothing's S_f in tile order (scan_carry).
//   k_cmp_apply       every tile: the states entering the lane's run (det_enter_p, det_enter_s), then the run itself -- detector, smoothing, the
//                     gain curve, the product rounded once to f32 -- and one store.
// The order of every fold is the host's (compressor.cpp cmp_tile_states), and so are the bits.  The stride-30 run access is the 2-way
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
    det_summary_p(d, tile, r.p_tiles, e);
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_carry_p(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const CmpRow& r = rows[blockIdx.x];
    if (win_tiles(r.t0, r.n) <= 0) return;
    carry_max(designs[r.design].rho_tile, win_tiles(r.t0, r.n), r.p_tiles, ein, r.carry ? r.carry + kCarryCmpP : nullptr, r.open);
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
    det_summary_s(d, tile, r.p_tiles, r.s_tiles, e);
}

__global__ __launch_bounds__(kDspLanes) void k_cmp_carry_s(const CmpRow* __restrict__ rows, const CmpScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const CmpRow& r = rows[blockIdx.x];
    if (win_tiles(r.t0, r.n) <= 0) return;
    scan_carry(CmpSmooth(designs[r.design], 0.0), win_tiles(r.t0, r.n), r.s_tiles, ein, r.carry ? r.carry + kCarryCmpS : nullptr, r.open);
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
    const int c = run_count(cnt);
    float* run = tile + threadIdx.x * kDspRun;
    const double tp = det_enter_p(d, tile, c, r.p_tiles, e);
    const double ts = det_enter_s(d, tile, c, tp, r.s_tiles, e);
    cmp_run_y(d, run, c, tp, ts, run);
    __syncthreads();
    tile_store(r.x + base, cnt, tile);
}

}  // namespace

void launch_compressor(const CmpRow* rows_dev, int n, int max_tiles, const CmpScan* designs_dev, hipStream_t stream, bool any_open) {
    if (n <= 0 || max_tiles <= 0) return;
    const int hands = any_open ? max_tiles : max_tiles - 1;   // (an open window's last tile hands on as well)
    launch_scan_pair("k_cmp_summary_p", k_cmp_summary_p, "k_cmp_carry_p", k_cmp_carry_p, hands, n, stream, rows_dev, designs_dev);
    launch_scan_pair("k_cmp_summary_s", k_cmp_summary_s, "k_cmp_carry_s", k_cmp_carry_s, hands, n, stream, rows_dev, designs_dev);
    note_launch("k_cmp_apply");
    hipLaunchKernelGGL(k_cmp_apply, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, designs_dev);
}

}  // namespace ptts
