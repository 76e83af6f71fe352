// dsp.hip -- post-processing of ragged rows of decoded 24 kHz audio on the device, in front of k_resample (kernels.h DspRow; scan_block.h;
// DESIGN.md section 8, N3): ptts_dsp_apply's chain -- peak normalise, DC block, fade in, fade out -- in place, and integrated loudness
// (ITU-R BS.1770-4, mono) with the gain that takes a row to its target.
//
//   k_dsp_peak      normalise and loudness rows: max |x| of the row.  A max is order-independent and non-negative floats order like their bit
//                   patterns, so the workgroups' atomicMax on the uint32 image gives the host's peak whatever the schedule.  NaNs never win.
//   k_*_summary     one workgroup per full tile that another tile follows; lane l runs run l from zero state, lane 0 folds the 64 end states
//                   in run order into E_f (scan_summary).
//   k_*_carry       one workgroup per row; S_0 = 0, S_(f+1) = A^1920 S_f + E_f in tile order (scan_carry).
//   k_dsp_apply     every tile: gain (an IEEE f32 division, one f32 product per sample), the runs' recurrence from their entering states
//                   (scan_enter: t_0 = S_f, t_(l+1) = A^30 t_l + e_l in run order), the rounding to f32, the two fade gains as two f32
//                   products, one store.
//   k_loud_energy   every tile: the runs' entering states, each run's sum of squared outputs in sample order, and the tile's four sub-block
//                   energies (16 run sums each, in run order) as doubles.
//   k_loud_gate     one workgroup per row: block energies (20 sub-blocks in order, over 9600; lanes take a block each), the absolute and the
//                   relative gate and the means in block order by lane 0, M and the f32 gain min((float)sqrt(T / M), 1 / peak).
//   k_eq_summary, k_eq_carry, k_eq_apply   equaliser rows (DSP_EQ), behind k_dsp_apply on what it stored: the same three steps for the row's own
//                   cascade (EqSys<S>, N = 2 S states, the coefficients read from the table's equalisers behind its rows), then the two fade
//                   gains, which k_dsp_apply leaves to k_eq_apply for such a row.  The fold s <- A^30 s + e_l is N independent sums, each in its
//                   fixed order: lane i < N computes component i (lanes_advance), the other components reach it by v_readlane.  The bits are
//                   scan_advance's; the serial chain is one sum long, not N.
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
// closing window's.  The fold is lane 0's (the lanes' for the equaliser) in tile order from whatever state it starts with, so the windows of a row
// give the one-shot bits, and the one-shot chain is the window t0 = 0, carry null, of a closed row: the same code, launches and LDS.
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

// tile blockIdx.x of the row's window, which hands a state on: E_f into the window's per-tile states
template <class Sys>
__device__ __forceinline__ void scan_summary(const Sys& sc, const DspRow& r, double* states, const Gain g) {
    constexpr int N = Sys::N;
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

// a window of F >= 1 tiles: S_f of every tile from the E_f, 64 tiles at a time.  carry (null: the row starts here, from zero state, and ends
// here): the state the window in front left, and, behind an open window's last tile, the state it leaves (win_hands: the tiles that hand on)
template <class Sys>
__device__ __forceinline__ void scan_carry(const Sys& sc, int64_t F, double* states, double* carry, bool open) {
    constexpr int N = Sys::N;
    __shared__ double ein[kDspLanes][N], sout[kDspLanes][N];
    const int l = threadIdx.x;
    const int64_t hands = win_hands(F, open);
    double s[N] = {};   // lane 0's: the state entering tile c0 + j
    if (carry) for (int i = 0; i < N; i++) s[i] = carry[i];
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) for (int i = 0; i < N; i++) ein[l][i] = scan_E<N>(states, f)[i];
        __syncthreads();
        if (l == 0) {
            const int m = (int)min((int64_t)kDspLanes, F - c0);
            for (int j = 0; j < m; j++) {
                for (int i = 0; i < N; i++) sout[j][i] = s[i];
                if (c0 + j < hands) scan_advance<N>(sc.a_tile, s, ein[j]);
            }
        }
        __syncthreads();
        if (f < F) for (int i = 0; i < N; i++) scan_S<N>(states, f)[i] = sout[l][i];
        __syncthreads();
    }
    if (open && l == 0) for (int i = 0; i < N; i++) carry[i] = s[i];
}

// z <- the state entering the lane's run (c samples at `run`, in LDS) of tile blockIdx.x: every run from zero state, then lane 0's fold in run
// order from S_f.  (Behind a run that is not full no run follows: its t is not read.)
template <class Sys>
__device__ __forceinline__ void scan_enter(const Sys& sc, const float* run, int c, double* states, double* z) {
    constexpr int N = Sys::N;
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

template <bool LOUD>
__global__ __launch_bounds__(kDspLanes) void k_dsp_summary(const DspRow* __restrict__ rows, const DspScan sc) {
    const DspRow& r = rows[blockIdx.y];
    if ((r.flags & DSP_DC) && tile_hands_on(r.t0, r.n, r.flags & DSP_OPEN)) scan_summary(sc, r, r.tiles, row_gain<LOUD>(r));
}

__global__ __launch_bounds__(kDspLanes) void k_loud_summary(const DspRow* __restrict__ rows, const LoudScan sc) {
    const DspRow& r = rows[blockIdx.y];
    if ((r.flags & DSP_LOUD) && tile_hands_on(0, r.n, false)) scan_summary(sc, r, loud_states(r.loud), kNoGain);
}

__global__ __launch_bounds__(kDspLanes) void k_dsp_carry(const DspRow* __restrict__ rows, const DspScan sc) {
    const DspRow& r = rows[blockIdx.x];
    if ((r.flags & DSP_DC) && win_tiles(r.t0, r.n) > 0) scan_carry(sc, win_tiles(r.t0, r.n), r.tiles, r.carry ? r.carry + kCarryDc : nullptr, r.flags & DSP_OPEN);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_carry(const DspRow* __restrict__ rows, const LoudScan sc) {
    const DspRow& r = rows[blockIdx.x];
    if ((r.flags & DSP_LOUD) && r.n > 0) scan_carry(sc, scan_tiles(r.n), loud_states(r.loud), nullptr, false);
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
        scan_enter(sc, run, c, r.tiles, z);
        sc.run(run, c, z, run);
        __syncthreads();
    }
    store_tile(r, base, cnt, tile, fin, fade_out);
}

// ---- equaliser rows ----

__device__ __forceinline__ double lane_bcast(double v, int lane) {   // lane's v in every lane (lane: the same in all of them)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// scan_advance, a component per lane: s <- P s + e with s_i, e_i and row i of P in lane i (i < N; the lanes behind repeat lane N - 1).  Sum i is
// scan_advance's sum i, product by product.  All 64 lanes call it together.
template <int N>
__device__ __forceinline__ double lanes_advance(const double (&prow)[N], double si, double ei) {
#pragma clang fp contract(off)
    double v = prow[0] * lane_bcast(si, 0);
#pragma unroll
    for (int m = 1; m < N; m++) v = v + prow[m] * lane_bcast(si, m);
    return v + ei;
}

// tile blockIdx.x of an equaliser row, which hands a state on (the tile is in LDS): E_f into the row's per-tile states.  e: [kDspLanes][N]
template <class Sys>
__device__ __forceinline__ void eq_summary(const Sys sc, const DspRow& r, const float* tile, double* e) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x, i = min(l, N - 1);
    double z[N] = {};
    sc.run(tile + l * kDspRun, kDspRun, z);
#pragma unroll
    for (int k = 0; k < N; k++) e[l * N + k] = z[k];
    __syncthreads();
    double prow[N];
#pragma unroll
    for (int m = 0; m < N; m++) prow[m] = sc.a_run[N * i + m];
    double s = 0.0;
    for (int j = 0; j < kDspLanes; j++) s = lanes_advance<N>(prow, s, e[j * N + i]);
    if (l < N) scan_E<N>(r.eq_tiles, blockIdx.x)[l] = s;
}

// a window of F >= 1 tiles of an equaliser row: S_f of every tile from the E_f, 64 tiles at a time.  ein: [kDspLanes][N]; carry, open: as
// scan_carry's
template <class Sys>
__device__ __forceinline__ void eq_carry(const Sys sc, int64_t F, double* states, double* ein, double* carry, bool open) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x, i = min(l, N - 1);
    const int64_t hands = win_hands(F, open);
    double prow[N];
#pragma unroll
    for (int m = 0; m < N; m++) prow[m] = sc.a_tile[N * i + m];
    double s = carry ? carry[i] : 0.0;   // component i of the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) {
#pragma unroll
            for (int k = 0; k < N; k++) ein[l * N + k] = scan_E<N>(states, f)[k];
        }
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            if (l < N) scan_S<N>(states, c0 + j)[l] = s;
            if (c0 + j < hands) s = lanes_advance<N>(prow, s, ein[j * N + i]);
        }
        __syncthreads();
    }
    if (open && l < N) carry[l] = s;
}

// the lane's run (c samples at `run`, in LDS) of tile blockIdx.x of an equaliser row, filtered in place from its entering state: every run from
// zero state, the fold in run order from S_f (t_l takes e_l's place in et: [kDspLanes][N]), the run again
template <class Sys>
__device__ __forceinline__ void eq_filter(const Sys sc, const DspRow& r, float* run, int c, double* et) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x, i = min(l, N - 1);
    double z[N] = {};
    sc.run(run, c, z);
#pragma unroll
    for (int k = 0; k < N; k++) et[l * N + k] = z[k];
    __syncthreads();
    double prow[N];
#pragma unroll
    for (int m = 0; m < N; m++) prow[m] = sc.a_run[N * i + m];
    double s = scan_S<N>(r.eq_tiles, blockIdx.x)[i];
    for (int j = 0; j < kDspLanes; j++) {
        double ej = 0.0;
        if (l < N) { ej = et[j * N + l]; et[j * N + l] = s; }
        s = lanes_advance<N>(prow, s, ej);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) z[k] = et[l * N + k];
    sc.run(run, c, z, run);
    __syncthreads();
}

constexpr int kEqStates = 2 * kEqMaxSections;

__global__ __launch_bounds__(kDspLanes) void k_eq_summary(const DspRow* __restrict__ rows, const EqScan* __restrict__ eqs) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes * kEqStates];
    const DspRow& r = rows[blockIdx.y];
    if (!(r.flags & DSP_EQ) || !tile_hands_on(r.t0, r.n, r.flags & DSP_OPEN)) return;
    float* tile = reinterpret_cast<float*>(tile4);
    load_tile(r, (r.t0 + blockIdx.x) * kDspTile, kDspTile, tile, kNoGain);
    __syncthreads();
    const EqScan& q = eqs[r.eq];
    switch (q.S) {
        case 1: eq_summary(EqSys<1>(q), r, tile, e); break;
        case 2: eq_summary(EqSys<2>(q), r, tile, e); break;
        case 3: eq_summary(EqSys<3>(q), r, tile, e); break;
        case 4: eq_summary(EqSys<4>(q), r, tile, e); break;
        default: break;
    }
}

__global__ __launch_bounds__(kDspLanes) void k_eq_carry(const DspRow* __restrict__ rows, const EqScan* __restrict__ eqs) {
    __shared__ double ein[kDspLanes * kEqStates];
    const DspRow& r = rows[blockIdx.x];
    const int64_t F = win_tiles(r.t0, r.n);
    if (!(r.flags & DSP_EQ) || F <= 0) return;
    const EqScan& q = eqs[r.eq];
    double* const carry = r.carry ? r.carry + kCarryEq : nullptr;
    const bool open = (r.flags & DSP_OPEN) != 0;
    switch (q.S) {
        case 1: eq_carry(EqSys<1>(q), F, r.eq_tiles, ein, carry, open); break;
        case 2: eq_carry(EqSys<2>(q), F, r.eq_tiles, ein, carry, open); break;
        case 3: eq_carry(EqSys<3>(q), F, r.eq_tiles, ein, carry, open); break;
        case 4: eq_carry(EqSys<4>(q), F, r.eq_tiles, ein, carry, open); break;
        default: break;
    }
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
    const EqScan& q = eqs[r.eq];
    switch (q.S) {
        case 1: eq_filter(EqSys<1>(q), r, run, c, et); break;
        case 2: eq_filter(EqSys<2>(q), r, run, c, et); break;
        case 3: eq_filter(EqSys<3>(q), r, run, c, et); break;
        case 4: eq_filter(EqSys<4>(q), r, run, c, et); break;
        default: break;
    }
    store_tile(r, base, cnt, tile, r.fade_in, r.fade_out);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_energy(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double q[kDspLanes];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_LOUD) || base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    load_tile(r, base, cnt, tile, kNoGain);
    __syncthreads();
    const int l = threadIdx.x, c = run_count(cnt);
    double z[LoudScan::N];
    scan_enter(sc, tile + l * kDspRun, c, loud_states(r.loud), z);
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
    if (p.any_norm || (p.any_loud && p.apply)) {   // (a measurement alone has no ceiling to keep)
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
    if (!p.apply) return;   // a measurement alone
    if (p.any_dc) {
        if (hands > 0) {
            note_launch("k_dsp_summary");
            hipLaunchKernelGGL(p.any_loud ? k_dsp_summary<true> : k_dsp_summary<false>, handing, lanes, 0, stream, rows_dev, *p.scan);
        }
        note_launch("k_dsp_carry");
        hipLaunchKernelGGL(k_dsp_carry, dim3((unsigned)n), lanes, 0, stream, rows_dev, *p.scan);
    }
    note_launch("k_dsp_apply");
    if (!p.any_eq) {
        hipLaunchKernelGGL((p.any_loud ? k_dsp_apply<true, false> : k_dsp_apply<false, false>), tiles, lanes, 0, stream, rows_dev, *p.scan);
    } else {
        hipLaunchKernelGGL((p.any_loud ? k_dsp_apply<true, true> : k_dsp_apply<false, true>), tiles, lanes, 0, stream, rows_dev, *p.scan);
        if (hands > 0) {   // behind k_dsp_apply: the equaliser reads what it stored
            note_launch("k_eq_summary");
            hipLaunchKernelGGL(k_eq_summary, handing, lanes, 0, stream, rows_dev, p.eqs);
        }
        note_launch("k_eq_carry");
        hipLaunchKernelGGL(k_eq_carry, dim3((unsigned)n), lanes, 0, stream, rows_dev, p.eqs);
        note_launch("k_eq_apply");
        hipLaunchKernelGGL(k_eq_apply, tiles, lanes, 0, stream, rows_dev, p.eqs);
    }
}

}  // namespace ptts
