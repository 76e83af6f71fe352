// dsp.hip -- post-processing of ragged rows of decoded 24 kHz audio on the device, in front of k_resample (kernels.h DspRow; scan_block.h;
// DESIGN.md section 8, N3): ptts_dsp_apply's chain -- peak normalise, DC block, fade in, fade out -- in place, and integrated loudness
// (ITU-R BS.1770-4, mono) with the gain that takes a row to its target.
//
//   k_dsp_peak      normalise and loudness rows: max |x| of the row.  A max is order-independent and non-negative floats order like their bit
//                   patterns, so the workgroups' atomicMax on the uint32 image gives the host's peak whatever the schedule.  NaNs never win.
//   k_*_summary     one workgroup per full tile that another tile follows: the tile into LDS, E_f from it (dsp_tile.h scan_summary; the DC block's
//                   fold is lane 0's, dc_summary below).
//   k_*_carry       one workgroup per row: S_f of every tile in tile order (dsp_tile.h scan_carry).
//   k_dsp_apply     every tile: gain (an IEEE f32 division, one f32 product per sample), the runs' recurrence from their entering states
//                   (dc_enter below: dsp_tile.h's scan_enter with lane 0's fold), the rounding to f32, the two fade gains as two f32 products,
//                   one store.
//   k_loud_energy   every tile: the runs' entering states, each run's sum of squared outputs in sample order, and the tile's four sub-block
//                   energies (16 run sums each, in run order) as doubles.
//   k_loud_gate     one workgroup per row: block energies (20 sub-blocks in order, over 9600; lanes take a block each), the absolute and the
//                   relative gate and the means in block order by lane 0, M and the f32 gain min((float)sqrt(T / M), 1 / peak).
//   k_eq_summary, k_eq_carry, k_eq_apply   equaliser rows (DSP_EQ), behind k_dsp_apply on what it stored: the same three steps for the row's own
//                   cascade (EqSys<S>, N = 2 S states, the coefficients read from the table's equalisers behind its rows; eq_dispatch picks
//                   the instantiation), then the two fade gains, which k_dsp_apply leaves to k_eq_apply for such a row.
// The scan itself -- the runs from zero state, the fold in run order, the carry in tile order -- is dsp_tile.h's for the three systems (but for
// dc_summary and dc_enter, which say why); the kernels here load and store tiles, own the LDS and apply gains, fades and energies.
// The limiter's kernels (limiter.hip) and the true-peak pair (true_peak.hip) follow these on the same rows; dsp_launch (dsp_device.cpp) has the order.
// k_dsp_* are the DC block's (DspScan, DSP_DC rows, on the f32 product x * gain wherever it is read), k_loud_* the K-weighting's (LoudScan,
// DSP_LOUD rows, on the RAW samples: nothing is written to them, k_dsp_apply applies the gain).  Stream order has the peak complete before
// k_loud_gate and k_dsp_summary start, and the loudness gain before k_dsp_summary.  One wave per workgroup and at most 12.5 KB of LDS: a CU
// holds a dozen workgroups, the passes are reads of the rows at HBM rate.  Tiles lie on the row's own grid and every sum has one order: a
// row's bits are a function of the row alone, and they are the bits of the host instantiations (dsp.cpp, loudness.cpp).  Nothing at or beyond
// n is read or written.
// Windows (kernels.h DSP_OPEN, DspRow::t0, ::carry; dsp_tile.h): k_dsp_summary / _carry / _apply and k_eq_summary / _carry / _apply may cover tiles
// [t0, ceil(n / 1920)) of a row only, with the window's own per-tile states; the carries start from the state the window in front left and an open
// window leaves the state behind its last tile, whose E_f the summaries then make as well; the fade in counts in the whole row, the fade out is the
// closing window's.  The fold runs in tile order from whatever state it starts with, so the windows of a row give the one-shot bits, and the
// one-shot chain is the window t0 = 0, carry null, of a closed row: the same code, launches and LDS.
// k_dsp_summary and k_dsp_apply are templates on whether the table has a loudness row (k_dsp_apply: and an equaliser row), so a table without
// one launches the instantiation that does not know the flag: the code it ran before the flag existed.
#include "device_util.h"
#include "dsp_tile.h"

namespace ptts {

namespace {

constexpr int kPeakThreads = 256, kPeakChunk = 4 * kDspTile;

struct Gain { bool on; float g; };
constexpr Gain kNoGain{false, 1.0f};
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

// samples [base, base + cnt) of the row into tile[0, cnt), times the gain if it is on; 16-byte loads where the row's alignment allows
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

// The DC block's own summary and enter: dsp_tile.h's scan_summary and scan_enter with the fold left to lane 0, its t_l scattered through a second
// LDS array, and the LDS their own.  Both shared forms measured slower in k_dsp_summary and k_dsp_apply (profiles/dsp_scan_refactor.json: 4 % split,
// 8 % whole), and so did this form on LDS passed in by pointer (3 %: the fold is then not unrolled), so these two kernels keep the code they had;
// the carry is the shared one.  The bits are scan_advance's either way.
// tile blockIdx.x of the row's window, which hands a state on: E_f into the window's per-tile states
__device__ __forceinline__ void dc_summary(const DspScan& sc, const DspRow& r, double* states, const Gain g) {
    constexpr int N = DspScan::N;
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes][N];
    float* tile = reinterpret_cast<float*>(tile4);
    load_tile(r, (r.t0 + blockIdx.x) * kDspTile, kDspTile, tile, g);
    __syncthreads();
    const int l = threadIdx.x;
    double z[N] = {};
    sc.run(tile + l * kDspRun, kDspRun, z);
    for (int i = 0; i < N; i++) e[l][i] = z[i];
    __syncthreads();
    if (l == 0) {
        double s[N] = {};
        for (int j = 0; j < kDspLanes; j++) scan_advance<N>(sc.a_run, s, e[j]);
        double* E = scan_E<N>(states, blockIdx.x);
        for (int i = 0; i < N; i++) E[i] = s[i];
    }
}
// z <- the state entering the lane's run (c samples at `run`, in LDS) of tile blockIdx.x
__device__ __forceinline__ void dc_enter(const DspScan& sc, const float* run, int c, double* states, double* z) {
    constexpr int N = DspScan::N;
    __shared__ double e[kDspLanes][N], t[kDspLanes][N];
    const int l = threadIdx.x;
    for (int i = 0; i < N; i++) z[i] = 0.0;
    sc.run(run, c, z);
    for (int i = 0; i < N; i++) e[l][i] = z[i];
    __syncthreads();
    if (l == 0) {
        const double* S = scan_S<N>(states, blockIdx.x);
        double s[N];
        for (int i = 0; i < N; i++) s[i] = S[i];
        for (int j = 0; j < kDspLanes; j++) {
            for (int i = 0; i < N; i++) t[j][i] = s[i];
            scan_advance<N>(sc.a_run, s, e[j]);
        }
    }
    __syncthreads();
    for (int i = 0; i < N; i++) z[i] = t[l][i];
}

// the same for the K-weighting, on the shared scan
__device__ __forceinline__ void loud_summary(const LoudScan& sc, const DspRow& r, double* states) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes * LoudScan::N];
    float* tile = reinterpret_cast<float*>(tile4);
    load_tile(r, blockIdx.x * (int64_t)kDspTile, kDspTile, tile, kNoGain);
    __syncthreads();
    scan_summary(sc, tile, e, scan_E<LoudScan::N>(states, blockIdx.x));
}

template <bool LOUD>
__global__ __launch_bounds__(kDspLanes) void k_dsp_summary(const DspRow* __restrict__ rows, const DspScan sc) {
    const DspRow& r = rows[blockIdx.y];
    if ((r.flags & DSP_DC) && tile_hands_on(r.t0, r.n, r.flags & DSP_OPEN)) dc_summary(sc, r, r.tiles, row_gain<LOUD>(r));
}

__global__ __launch_bounds__(kDspLanes) void k_loud_summary(const DspRow* __restrict__ rows, const LoudScan sc) {
    const DspRow& r = rows[blockIdx.y];
    if ((r.flags & DSP_LOUD) && tile_hands_on(0, r.n, false)) loud_summary(sc, r, loud_states(r.loud));
}

__global__ __launch_bounds__(kDspLanes) void k_dsp_carry(const DspRow* __restrict__ rows, const DspScan sc) {
    __shared__ double ein[kDspLanes * DspScan::N];
    const DspRow& r = rows[blockIdx.x];
    if ((r.flags & DSP_DC) && win_tiles(r.t0, r.n) > 0) scan_carry(sc, win_tiles(r.t0, r.n), r.tiles, ein, r.carry ? r.carry + kCarryDc : nullptr, r.flags & DSP_OPEN);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_carry(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ double ein[kDspLanes * LoudScan::N];
    const DspRow& r = rows[blockIdx.x];
    if ((r.flags & DSP_LOUD) && r.n > 0) scan_carry(sc, scan_tiles(r.n), loud_states(r.loud), ein, nullptr, false);
}

// tile[0, cnt) -- samples [base, base + cnt) of the row -- times the two fade gains, into the row.  base counts in the whole row, and so do the
// fades: an open window's row has no fade out yet (fade_out 0), the window that closes the row applies it with the row's final n
__device__ __forceinline__ void store_tile(const DspRow& r, int64_t base, int cnt, const float* tile, int64_t fin, int64_t fade_out) {
    const int64_t n = r.n, fout0 = n - fade_out;
    float* dst = r.x + base;
    const bool vec = ((uintptr_t)dst & 15) == 0;
    const float fin_f = (float)fin, fout_f = (float)fade_out;
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

// EQ: the table has an equaliser row; such a row's fades are k_eq_apply's, behind its filter
template <bool LOUD, bool EQ>
__global__ __launch_bounds__(kDspLanes) void k_dsp_apply(const DspRow* __restrict__ rows, const DspScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (r.t0 + blockIdx.x) * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const Gain g = row_gain<LOUD>(r);
    const bool dc = (r.flags & DSP_DC) != 0;
    const bool fades = !(EQ && (r.flags & DSP_EQ));
    const int64_t fin = fades ? r.fade_in : 0, fade_out = fades ? r.fade_out : 0, fout0 = n - fade_out;   // fade in below fin, fade out from fout0 on
    if (!g.on && !dc && base >= fin && base + cnt <= fout0) return;   // a tile that no step changes
    load_tile(r, base, cnt, tile, g);
    __syncthreads();
    if (dc) {
        float* run = tile + threadIdx.x * kDspRun;
        const int c = run_count(cnt);
        double z[DspScan::N];
        dc_enter(sc, run, c, r.tiles, z);
        sc.run(run, c, z, run);
        __syncthreads();
    }
    store_tile(r, base, cnt, tile, fin, fade_out);
}

// ---- equaliser rows ----

constexpr int kEqStates = 2 * kEqMaxSections;   // the kernels' LDS is sized for the longest cascade; a row's own N = 2 S packs at its front

__global__ __launch_bounds__(kDspLanes) void k_eq_summary(const DspRow* __restrict__ rows, const EqScan* __restrict__ eqs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes * kEqStates];
    const DspRow& r = rows[blockIdx.y];
    if (!(r.flags & DSP_EQ) || !tile_hands_on(r.t0, r.n, r.flags & DSP_OPEN)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    load_tile(r, (r.t0 + blockIdx.x) * kDspTile, kDspTile, tile, kNoGain);
    __syncthreads();
    eq_dispatch(eqs[r.eq], [&](auto sys) { scan_summary(sys, tile, e, scan_E<decltype(sys)::N>(r.eq_tiles, blockIdx.x)); });
}

__global__ __launch_bounds__(kDspLanes) void k_eq_carry(const DspRow* __restrict__ rows, const EqScan* __restrict__ eqs) {
    __shared__ double ein[kDspLanes * kEqStates];
    const DspRow& r = rows[blockIdx.x];
    const int64_t F = win_tiles(r.t0, r.n);
    if (!(r.flags & DSP_EQ) || F <= 0) return;
    double* const carry = r.carry ? r.carry + kCarryEq : nullptr;
    eq_dispatch(eqs[r.eq], [&](auto sys) { scan_carry(sys, F, r.eq_tiles, ein, carry, (r.flags & DSP_OPEN) != 0); });
}

__global__ __launch_bounds__(kDspLanes) void k_eq_apply(const DspRow* __restrict__ rows, const EqScan* __restrict__ eqs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double et[kDspLanes * kEqStates];
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (r.t0 + blockIdx.x) * kDspTile;
    if (!(r.flags & DSP_EQ) || base >= n) return;
    float* tile = reinterpret_cast<float*>(tile4);
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    load_tile(r, base, cnt, tile, kNoGain);
    __syncthreads();
    float* run = tile + threadIdx.x * kDspRun;
    const int c = run_count(cnt);
    eq_dispatch(eqs[r.eq], [&](auto sys) {   // the lane's run, filtered in place from its entering state
        double z[decltype(sys)::N];
        scan_enter(sys, run, c, scan_S<decltype(sys)::N>(r.eq_tiles, blockIdx.x), et, z);
        sys.run(run, c, z, run);
    });
    __syncthreads();
    store_tile(r, base, cnt, tile, r.fade_in, r.fade_out);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_energy(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double q[kDspLanes], et[kDspLanes * LoudScan::N];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_LOUD) || base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    load_tile(r, base, cnt, tile, kNoGain);
    __syncthreads();
    const int l = threadIdx.x, c = run_count(cnt);
    double z[LoudScan::N];
    scan_enter(sc, tile + l * kDspRun, c, scan_S<LoudScan::N>(loud_states(r.loud), blockIdx.x), et, z);
    q[l] = sc.run(tile + l * kDspRun, c, z);
    __syncthreads();
    // (a sub-block the row ends in holds the sum over the samples that are there; no whole 400 ms block contains it, so the gate never reads it)
    if (l < kLoudSubsPerTile) loud_subs(r.loud, scan_tiles(n))[(int64_t)blockIdx.x * kLoudSubsPerTile + l] = loud_sub_energy(q + l * kLoudRunsPerSub);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_gate(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ double z[kDspLanes];
    __shared__ double rel_s;
    const DspRow& r = rows[blockIdx.x];
    if (!(r.flags & DSP_LOUD)) return;
    const int64_t nb = loud_blocks(r.n);
    const double* sub = loud_subs(r.loud, scan_tiles(r.n));
    const int l = threadIdx.x;
    LoudAcc first{0.0, 0}, second{0.0, 0};   // lane 0's
    for (int pass = 0; pass < 2; pass++) {
        const double rel = pass ? rel_s : sc.abs_gate;
        for (int64_t c0 = 0; c0 < nb; c0 += kDspLanes) {
            if (c0 + l < nb) z[l] = loud_block_energy(sub, c0 + l);
            __syncthreads();
            if (l == 0) {
                const int m = (int)min((int64_t)kDspLanes, nb - c0);
                for (int j = 0; j < m; j++) loud_gate_add(pass ? second : first, z[j], sc.abs_gate, rel);
            }
            __syncthreads();
        }
        if (pass == 0) {
            if (l == 0) rel_s = first.cnt ? loud_rel_gate(first) : 0.0;
            __syncthreads();
        }
    }
    if (l == 0) {
        const double M = (first.cnt && second.cnt) ? loud_div(second.sum, (double)second.cnt) : 0.0;
        r.loud[0] = M;
        *reinterpret_cast<float*>(r.loud + 1) = loud_gain(M, r.target, __uint_as_float(*r.peak));
    }
}

}  // namespace

void launch_dsp(const DspRow* rows_dev, int n, int max_tiles, const DspLaunch& p, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    const int hands = p.any_open ? max_tiles : max_tiles - 1;   // (an open window's last tile hands on as well)
    const dim3 tiles((unsigned)max_tiles, (unsigned)n), handing((unsigned)hands, (unsigned)n), lanes(kDspLanes);
    if (p.any_norm || (p.any_loud && (p.apply || p.gain_only))) {   // (a measurement alone has no ceiling to keep)
        note_launch("k_dsp_peak");
        hipLaunchKernelGGL(k_dsp_peak, dim3((unsigned)((max_tiles + 3) / 4), (unsigned)n), dim3(kPeakThreads), 0, stream, rows_dev);
    }
    if (p.any_loud) {   // behind k_dsp_peak, in front of every kernel that reads a gain
        if (max_tiles > 1) {
            note_launch("k_loud_summary");
            hipLaunchKernelGGL(k_loud_summary, handing, lanes, 0, stream, rows_dev, *p.loud);
        }
        note_launch("k_loud_carry");
        hipLaunchKernelGGL(k_loud_carry, dim3((unsigned)n), lanes, 0, stream, rows_dev, *p.loud);
        note_launch("k_loud_energy");
        hipLaunchKernelGGL(k_loud_energy, tiles, lanes, 0, stream, rows_dev, *p.loud);
        note_launch("k_loud_gate");
        hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)n), lanes, 0, stream, rows_dev, *p.loud);
    }
    if (!p.apply || p.gain_only) return;   // a measurement alone, or the gain left in its word for another kernel to apply
    if (p.any_dc) launch_scan_pair("k_dsp_summary", p.any_loud ? k_dsp_summary<true> : k_dsp_summary<false>, "k_dsp_carry", k_dsp_carry, hands, n, stream, rows_dev, *p.scan);
    note_launch("k_dsp_apply");
    if (!p.any_eq) {
        hipLaunchKernelGGL((p.any_loud ? k_dsp_apply<true, false> : k_dsp_apply<false, false>), tiles, lanes, 0, stream, rows_dev, *p.scan);
    } else {
        hipLaunchKernelGGL((p.any_loud ? k_dsp_apply<true, true> : k_dsp_apply<false, true>), tiles, lanes, 0, stream, rows_dev, *p.scan);
        launch_scan_pair("k_eq_summary", k_eq_summary, "k_eq_carry", k_eq_carry, hands, n, stream, rows_dev, p.eqs);   // behind k_dsp_apply: the equaliser reads what it stored
        note_launch("k_eq_apply");
        hipLaunchKernelGGL(k_eq_apply, tiles, lanes, 0, stream, rows_dev, p.eqs);
    }
}

}  // namespace ptts
