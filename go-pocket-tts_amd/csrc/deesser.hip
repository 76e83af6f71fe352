// deesser.hip -- a request's de-esser on ragged rows of decoded 24 kHz audio, in place, behind the compressor's tables and in front of the DSP
// kernels (kernels.h DeRow; deesser.h).  Seven launches, shaped like compressor.hip's: one wave per workgroup, lane l
// owns run l of its tile; the tile's samples are read into LDS once per kernel (7.5 KB), its band is made beside them (7.5 KB, plus 1.5 KB of
// run states) and never leaves the workgroup.  The scan has three levels, each of which needs the one in front at the start of every tile:
//
//   k_de_summary_b    one workgroup per full tile that another tile follows: every run's end state of the side chain's biquad from zero state,
//                     folded in run order (scan_advance<2>) into E_f.
//   k_de_carry_b      one workgroup per row: S_0 = 0, S_(f+1) = A^1920 S_f + E_f in tile order.
//   k_de_summary_p    the same tiles: the band of the tile from the section's entering state S_f (every run from zero, the fold, every run again
//                     with its outputs rounded to f32 into LDS), then every run's detector end state on the band from p = 0, folded with max.
//   k_de_carry_p      one workgroup per row: S_0 = 0, S_(f+1) = max(rho^1920 S_f, E_f).
//   k_de_summary_s    the same tiles: the band again, the detector state entering every run (the fold from S_f), every run's smoothing end state
//                     from s = 0 with the detector recomputed, folded in run order (scan_advance<1>).
//   k_de_carry_s      one workgroup per row: S_0 = 0, S_(f+1) = alpha^1920 S_f + E_f.
//   k_de_apply        every tile: band, detector fold and smoothing fold again from the tile's three entering states, then the run itself --
//                     detector, smoothing, the curve held at the floor, x + (g - 1) b rounded once to f32 where the gain is not 0 dB -- and one
//                     store.
// The band's summaries cannot share a launch with the detector's: a tile's band needs S_f of the section, which is the carry's to make.  Every
// fold is evaluated by all 64 lanes alike from LDS (a broadcast read), lane l keeping the value it meets at step l: the order is the host's
// (deesser.cpp de_apply_blocked), and so are the bits; the functions that walk samples are scan_block.h's EqSys<1>::run, compressor.h's cmp_run_p
// and cmp_run_s and deesser.h's de_run_y, the host's own.  The stride-30 run access is the 2-way bank pattern k_eq_apply and k_cmp_apply live with.
// No atomics.  No workgroup reads what another workgroup of the same launch writes: the summaries read the raw samples and the states the
// carries in front stored, and write their own tile's E_f; a carry's one workgroup reads and writes its own row's states; k_de_apply reads
// states and its own tile's samples and writes that tile alone, and it is the only kernel that writes samples.  Stream order has each launch
// complete before the next reads what it wrote.  Nothing at or beyond n is read or written.
#include "device_util.h"
#include "dsp_tile.h"

namespace ptts {

namespace {

// the section's fold over a tile's runs from state S: scan_advance<2>, t <- A^30 t + e_l (e: LDS, [kDspLanes][2], complete).  Every lane
// evaluates it alike; mine receives the state entering the lane's own run, behind the state behind the last run
__device__ __forceinline__ void de_enter_b(const EqSys<1>& sys, const double* e, const double* S, double* mine, double* behind) {
    const int l = threadIdx.x;
    double t[2] = {S[0], S[1]};
    mine[0] = t[0]; mine[1] = t[1];
    for (int j = 0; j < kDspLanes; j++) {
        if (j == l) { mine[0] = t[0]; mine[1] = t[1]; }
        scan_advance<2>(sys.a_run, t, e + 2 * j);
    }
    behind[0] = t[0]; behind[1] = t[1];
}

// every run's end state of the section from zero state into eb (LDS, [kDspLanes][2]); run: the lane's c samples (LDS).  Ends behind a barrier
__device__ __forceinline__ void de_ends_b(const EqSys<1>& sys, const float* run, int c, double* eb) {
    const int l = threadIdx.x;
    double z[2] = {0.0, 0.0};
    sys.run(run, c, z);
    eb[2 * l] = z[0]; eb[2 * l + 1] = z[1];
    __syncthreads();
}

// the band of the lane's run into brun (LDS) from the state S_f entering tile blockIdx.x.  Ends behind a barrier: the tile's band is complete
__device__ __forceinline__ void de_band_run(const EqSys<1>& sys, const DeRow& r, const float* run, int c, double* eb, float* brun) {
    de_ends_b(sys, run, c, eb);
    double z[2], behind[2];
    de_enter_b(sys, eb, scan_S<2>(r.b_tiles, blockIdx.x), z, behind);
    sys.run(run, c, z, brun);
    __syncthreads();
}

// a row of F >= 1 tiles: the section's S_f of every tile from the E_f (scan_E<2>, scan_S<2>), 64 tiles at a time, by every lane alike (lane 0
// stores); the state is carried from one group of 64 to the next.  ein: LDS, [kDspLanes][2]
__device__ __forceinline__ void de_carry_b(const double* a_tile, int64_t F, double* states, double* ein) {
    const int l = threadIdx.x;
    const int64_t hands = F - 1;
    double s[2] = {0.0, 0.0};   // the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) { ein[2 * l] = scan_E<2>(states, f)[0]; ein[2 * l + 1] = scan_E<2>(states, f)[1]; }
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            if (l == 0) { scan_S<2>(states, c0 + j)[0] = s[0]; scan_S<2>(states, c0 + j)[1] = s[1]; }
            if (c0 + j < hands) scan_advance<2>(a_tile, s, ein + 2 * j);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_b(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2];
    const DeRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    tile_load(r.x + (int64_t)blockIdx.x * kDspTile, kDspTile, tile);
    __syncthreads();
    const DeScan& d = designs[r.design];
    const EqSys<1> sys = de_band(d);
    de_ends_b(sys, tile + threadIdx.x * kDspRun, kDspRun, eb);
    const double zero[2] = {0.0, 0.0};
    double mine[2], E[2];
    de_enter_b(sys, eb, zero, mine, E);
    if (threadIdx.x == 0) { scan_E<2>(r.b_tiles, blockIdx.x)[0] = E[0]; scan_E<2>(r.b_tiles, blockIdx.x)[1] = E[1]; }
}

__global__ __launch_bounds__(kDspLanes) void k_de_carry_b(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes * 2];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    de_carry_b(designs[r.design].a_tile, scan_tiles(r.n), r.b_tiles, ein);
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_p(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4], band4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2], e[kDspLanes];
    const DeRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    float* band = reinterpret_cast<float*>(band4);
    tile_load(r.x + (int64_t)blockIdx.x * kDspTile, kDspTile, tile);
    __syncthreads();
    const DeScan& d = designs[r.design];
    const int l = threadIdx.x;
    const float* brun = band + l * kDspRun;
    de_band_run(de_band(d), r, tile + l * kDspRun, kDspRun, eb, band + l * kDspRun);
    e[l] = cmp_run_p(d.det, brun, kDspRun, 0.0);
    __syncthreads();
    double E;
    fold_enter_max(d.det.rho_run, e, 0.0, &E);
    if (l == 0) scan_E<1>(r.p_tiles, blockIdx.x)[0] = E;
}

__global__ __launch_bounds__(kDspLanes) void k_de_carry_p(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    carry_one<true>(designs[r.design].det.rho_tile, scan_tiles(r.n), r.p_tiles, ein, nullptr, false);
}

__global__ __launch_bounds__(kDspLanes) void k_de_summary_s(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ float4 tile4[kDspTile / 4], band4[kDspTile / 4];
    __shared__ double eb[kDspLanes * 2], e[kDspLanes];
    const DeRow& r = rows[blockIdx.y];
    if (!tile_hands_on(0, r.n, false)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    float* band = reinterpret_cast<float*>(band4);
    tile_load(r.x + (int64_t)blockIdx.x * kDspTile, kDspTile, tile);
    __syncthreads();
    const DeScan& d = designs[r.design];
    const int l = threadIdx.x;
    const float* brun = band + l * kDspRun;
    de_band_run(de_band(d), r, tile + l * kDspRun, kDspRun, eb, band + l * kDspRun);
    e[l] = cmp_run_p(d.det, brun, kDspRun, 0.0);
    __syncthreads();
    double behind;
    const double tp = fold_enter_max(d.det.rho_run, e, scan_S<1>(r.p_tiles, blockIdx.x)[0], &behind);
    __syncthreads();
    e[l] = cmp_run_s(d.det, brun, kDspRun, tp, 0.0);
    __syncthreads();
    double E;
    fold_enter_sum(d.det.alpha_run, e, 0.0, &E);
    if (l == 0) scan_E<1>(r.s_tiles, blockIdx.x)[0] = E;
}

__global__ __launch_bounds__(kDspLanes) void k_de_carry_s(const DeRow* __restrict__ rows, const DeScan* __restrict__ designs) {
    __shared__ double ein[kDspLanes];
    const DeRow& r = rows[blockIdx.x];
    if (scan_tiles(r.n) <= 0) return;
    carry_one<false>(designs[r.design].det.alpha_tile, scan_tiles(r.n), r.s_tiles, ein, nullptr, false);
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
    const float* brun = band + l * kDspRun;
    de_band_run(de_band(d), r, run, c, eb, band + l * kDspRun);
    e[l] = cmp_run_p(d.det, brun, c, 0.0);
    __syncthreads();
    double behind;
    const double tp = fold_enter_max(d.det.rho_run, e, scan_S<1>(r.p_tiles, blockIdx.x)[0], &behind);
    __syncthreads();
    e[l] = cmp_run_s(d.det, brun, c, tp, 0.0);
    __syncthreads();
    const double ts = fold_enter_sum(d.det.alpha_run, e, scan_S<1>(r.s_tiles, blockIdx.x)[0], &behind);
    de_run_y(d, run, brun, c, tp, ts);
    __syncthreads();
    tile_store(r.x + base, cnt, tile);
}

}  // namespace

void launch_deesser(const DeRow* rows_dev, int n, int max_tiles, const DeScan* designs_dev, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    const int hands = max_tiles - 1;
    const dim3 tiles((unsigned)max_tiles, (unsigned)n), handing((unsigned)hands, (unsigned)n), rows((unsigned)n), lanes(kDspLanes);
    if (hands > 0) {
        note_launch("k_de_summary_b");
        hipLaunchKernelGGL(k_de_summary_b, handing, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_de_carry_b");
    hipLaunchKernelGGL(k_de_carry_b, rows, lanes, 0, stream, rows_dev, designs_dev);
    if (hands > 0) {
        note_launch("k_de_summary_p");
        hipLaunchKernelGGL(k_de_summary_p, handing, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_de_carry_p");
    hipLaunchKernelGGL(k_de_carry_p, rows, lanes, 0, stream, rows_dev, designs_dev);
    if (hands > 0) {
        note_launch("k_de_summary_s");
        hipLaunchKernelGGL(k_de_summary_s, handing, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_de_carry_s");
    hipLaunchKernelGGL(k_de_carry_s, rows, lanes, 0, stream, rows_dev, designs_dev);
    note_launch("k_de_apply");
    hipLaunchKernelGGL(k_de_apply, tiles, lanes, 0, stream, rows_dev, designs_dev);
}

}  // namespace ptts
