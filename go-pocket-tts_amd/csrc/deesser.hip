// deesser.hip -- a request's de-esser on ragged rows of decoded 24 kHz audio, in place, behind the compressor's tables and in front of the DSP
// kernels (kernels.h DeRow; deesser.h).  Seven launches: one wave per workgroup, lane l owns run l of its tile; the
// tile's samples are read into LDS once per kernel (7.5 KB), its band is made beside them (7.5 KB, plus 1.5 KB of run states) and never leaves
// the workgroup.  The scan has three levels, each of which needs the one in front at the start of every tile; the section's is dsp_tile.h's linear
// scan for EqSys<1> (scan_summary, scan_carry, scan_enter), the other two are its detector (det_*, carry_max), here given the band:
//
//   k_de_summary_b    one workgroup per full tile that another tile follows: the section's E_f.
//   k_de_carry_b      one workgroup per row: the section's S_f in tile order.
//   k_de_summary_p    the same tiles: the band of the tile from the section's entering state S_f (de_band_run: the states entering the runs, every
//                     run with its outputs rounded to f32 into LDS), then the detector's E_f on the band.
//   k_de_carry_p      one workgroup per row: the detector's S_f.
//   k_de_summary_s    the same tiles: the band again, then the smoothing's E_f on it.
//   k_de_carry_s      one workgroup per row: the smoothing's S_f.
//   k_de_apply        every tile: the band, the detector and the smoothing state entering the lane's run, then the run itself -- detector,
//                     smoothing, the curve held at the floor, x + (g - 1) b rounded once to f32 where the gain is not 0 dB -- and one store.
// The band's summaries cannot share a launch with the detector's: a tile's band needs S_f of the section, which is the carry's to make.  The
// order of every fold is the host's (deesser.cpp de_apply_blocked: scan_tile, cmp_tile_states), and so are the bits; the functions that walk
// samples are scan_block.h's EqSys<1>::run, compressor.h's cmp_run_p
// and cmp_run_s and deesser.h's de_run_y, the host's own.  The stride-30 run access is the 2-way bank pattern k_eq_apply and k_cmp_apply live with.
// No atomics.  No workgroup reads what another workgroup of the same launch writes: the summaries read the raw samples and the states the
// carries in front stored, and write their own tile's E_f; a carry's one workgroup reads and writes its own row's states; k_de_apply reads
// states and its own tile's samples and writes that tile alone, and it is the only kernel that writes samples.  Stream order has each launch
// complete before the next reads what it wrote.  Nothing at or beyond n is read or written.
#include "device_util.h"
#include "dsp_tile.h"

namespace ptts {

namespace {

// the band of the lane's run (c samples at `run`, LDS) into brun (LDS) from the section's state S_f entering tile blockIdx.x (dsp_tile.h
// scan_enter; eb: LDS, [kDspLanes * 2]).  Ends behind a barrier: the tile's band is complete
__device__ __forceinline__ void de_band_run(const EqSys<1>& sys, const DeRow& r, const float* run, int c, double* eb, float* brun) {
    double z[2];
    scan_enter(sys, run, c, scan_S<2>(r.b_tiles, blockIdx.x), eb, z);
    sys.run(run, c, z, brun);
    __syncthreads();
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_b(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2];
    const DeRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    tile_load(r.x + (int64_t)blockIdx.x * kDspTile, kDspTile, tile);
    __syncthreads();
    scan_summary(de_band(designs[r.design]), tile, eb, scan_E<2>(r.b_tiles, blockIdx.x));
}

__global__ __launch_bounds__(kDspLanes) void k_de_carry_b(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes * 2];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    scan_carry(de_band(designs[r.design]), scan_tiles(r.n), r.b_tiles, ein, nullptr, false);
}

// P: the detector's summary (E_f into p_tiles), else the smoothing's (into s_tiles), on the band of a handing tile
template <bool P>
__device__ __forceinline__ void de_summary(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4], band4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2], e[kDspLanes];
    const DeRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    float* band = reinterpret_cast<float*>(band4);
    tile_load(r.x + (int64_t)blockIdx.x * kDspTile, kDspTile, tile);
    __syncthreads();
    const DeScan& d = designs[r.design];
    de_band_run(de_band(d), r, tile + threadIdx.x * kDspRun, kDspRun, eb, band + threadIdx.x * kDspRun);
    if (P) det_summary_p(d.det, band, r.p_tiles, e);
    else det_summary_s(d.det, band, r.p_tiles, r.s_tiles, e);
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_p(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) { de_summary<true>(rows, designs); }

__global__ __launch_bounds__(kDspLanes) void k_de_carry_p(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    carry_max(designs[r.design].det.rho_tile, scan_tiles(r.n), r.p_tiles, ein, nullptr, false);
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_s(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) { de_summary<false>(rows, designs); }

__global__ __launch_bounds__(kDspLanes) void k_de_carry_s(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    scan_carry(CmpSmooth(designs[r.design].det, 0.0), scan_tiles(r.n), r.s_tiles, ein, nullptr, false);
}

__global__ __launch_bounds__(kDspLanes) void k_de_apply(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4], band4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2], e[kDspLanes];
    const DeRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    float* tile = reinterpret_cast<float*>(tile4);
    float* band = reinterpret_cast<float*>(band4);
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    tile_load(r.x + base, cnt, tile);
    __syncthreads();
    const DeScan& d = designs[r.design];
    const int l = threadIdx.x, c = run_count(cnt);
    float* run = tile + l * kDspRun;
    de_band_run(de_band(d), r, run, c, eb, band + l * kDspRun);
    const double tp = det_enter_p(d.det, band, c, r.p_tiles, e);
    const double ts = det_enter_s(d.det, band, c, tp, r.s_tiles, e);
    de_run_y(d, run, band + l * kDspRun, c, tp, ts);
    __syncthreads();
    tile_store(r.x + base, cnt, tile);
}

}  // namespace

void launch_deesser(const DeRow* rows_dev, int n, int max_tiles, const DeScan* designs_dev, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    const int hands = max_tiles - 1;
    launch_scan_pair("k_de_summary_b", k_de_summary_b, "k_de_carry_b", k_de_carry_b, hands, n, stream, rows_dev, designs_dev);
    launch_scan_pair("k_de_summary_p", k_de_summary_p, "k_de_carry_p", k_de_carry_p, hands, n, stream, rows_dev, designs_dev);
    launch_scan_pair("k_de_summary_s", k_de_summary_s, "k_de_carry_s", k_de_carry_s, hands, n, stream, rows_dev, designs_dev);
    note_launch("k_de_apply");
    hipLaunchKernelGGL(k_de_apply, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, designs_dev);
}

}  // namespace ptts
