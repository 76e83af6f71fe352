// dsp_tile.h -- what the post-processing kernels share on the device (dsp.hip, compressor.hip, deesser.hip, limiter.hip; scan_block.h has the grid and the
// host-and-device arithmetic): one wave per workgroup, workgroup blockIdx.x on tile blockIdx.x of its row, lane l on
// run l of the tile; the one linear tile scan (scan_summary, scan_carry, scan_enter) for every system of scan_block.h, the compressor's detector on a
// tile or on a band (det_*), and, the one piece of host code here, the summary-then-carry pair of launches every scan level makes (launch_scan_pair).  For .hip files only.
#pragma once
#include "compressor.h"
#include "scan_block.h"

namespace ptts {

// A launch covers a window of a row: tiles [t0, ceil(n / kDspTile)) of the row's own grid, n the samples up to the window's end; workgroup
// blockIdx.x is on tile t0 + blockIdx.x and on entry blockIdx.x of the window's per-tile states.  The row is open when more samples will follow
// behind n (n is then a multiple of kDspTile).  The one-shot chain is the window t0 = 0 of a closed row.
// only a full tile that another one follows hands a state on: in a closed row every tile but the last, in an open one the last as well
__device__ __forceinline__ bool tile_hands_on(int64_t t0, int64_t n, bool open) { return (t0 + blockIdx.x + 1) * kDspTile < n + (open ? 1 : 0); }
// of a window's F tiles, those that hand a state on (the first ones)
__device__ __forceinline__ int64_t win_hands(int64_t F, bool open) { return open ? F : F - 1; }
// samples of the lane's run in a tile of cnt
__device__ __forceinline__ int run_count(int cnt) { return scan_run_count(cnt, threadIdx.x); }

// src[0, cnt) -- a tile's samples in the row -- into tile[0, cnt) (LDS) and back; 16-byte accesses where the row's alignment allows
__device__ __forceinline__ void tile_load(const float* src, int cnt, float* tile) {
    const bool vec = ((uintptr_t)src & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(tile + q) = *reinterpret_cast<const float4*>(src + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) tile[q + u] = src[q + u];
    }
}
__device__ __forceinline__ void tile_store(float* dst, int cnt, const float* tile) {
    const bool vec = ((uintptr_t)dst & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(dst + q) = *reinterpret_cast<const float4*>(tile + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) dst[q + u] = tile[q + u];
    }
}

// ---- the linear scan (scan_block.h: e_l, the fold in run order, the carry in tile order, the run again), for a system Sys: N, a_run, a_tile, run() ----
// Summary, carry and enter are written once, on a fold state (LaneFold) that has two forms; both evaluate scan_advance's sums product by product,
// so the bits are the same whichever is used.  Measured on an MI355X (profiles/dsp_scan_refactor.json): with N = 4 the split form wins (k_loud_summary
// 35 us against 56 us), with N = 2 a v_readlane in the serial chain costs more than the products it saves (the k_de_* kernels 0.8 % slower, k_dsp_apply
// 7 %), so N = 2 keeps the state whole in every lane.  With N = 1 the split form has nothing to broadcast and differs from the whole one only in
// how scan_enter hands t_l to lane l: through LDS, which measured faster than the select (k_cmp_apply 91.6 us against 95 us).  The LDS every function
// needs is the caller's, [kDspLanes * N] doubles.

__device__ __forceinline__ double lane_bcast(double v, int lane) {   // lane's v in every lane (lane: the same in all of them)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The state of a fold s <- P s + e_j (P row-major N x N, in memory; e_j: LDS, [N]) as the wave holds it.  All 64 lanes call every member together.
template <int N, bool Split = (N != 2)>
struct LaneFold;
// ... whole in every lane: scan_advance itself, N^2 products a step, nothing crosses lanes; lane 0 stores
template <int N>
struct LaneFold<N, false> {
    const double* P;
    double s[N];
    __device__ LaneFold(const double* P_, const double* from) : P(P_) {   // from: the state to start with (null: zero)
#pragma unroll
        for (int k = 0; k < N; k++) s[k] = from ? from[k] : 0.0;
    }
    __device__ void advance(const double* e) { scan_advance<N>(P, s, e); }
    __device__ void enter_step(double* e, int j, double* mine) {   // step j of scan_enter: lane j keeps the state it meets (a select: e is only read)
        if (j == (int)threadIdx.x) {
#pragma unroll
            for (int k = 0; k < N; k++) mine[k] = s[k];
        }
        advance(e);
    }
    __device__ void entered(const double*, double*) const {}
    __device__ void store(double* dst) const {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < N; k++) dst[k] = s[k];
        }
    }
};
// ... split: lane i < N holds component i and row i of P and reads the other components by v_readlane (the lanes behind repeat lane N - 1): N
// independent sums, each scan_advance's sum i in its order; the serial chain is one sum long, a lane evaluates N products a step; lanes < N store
template <int N>
struct LaneFold<N, true> {
    const int i = min((int)threadIdx.x, N - 1);
    double prow[N], s;
    __device__ LaneFold(const double* P, const double* from) : s(from ? from[i] : 0.0) {
#pragma unroll
        for (int m = 0; m < N; m++) prow[m] = P[N * i + m];
    }
    __device__ void step(double ei) {
#pragma clang fp contract(off)
        double v = prow[0] * (N == 1 ? s : lane_bcast(s, 0));   // (N = 1: every lane repeats lane 0 and holds s itself)
#pragma unroll
        for (int m = 1; m < N; m++) v = v + prow[m] * lane_bcast(s, m);
        s = v + ei;
    }
    __device__ void advance(const double* e) { step(e[i]); }
    __device__ void enter_step(double* e, int, double*) {   // ... the state takes e_j's place in LDS
        const double ei = e[i];
        store(e);
        step(ei);
    }
    __device__ void entered(const double* et, double* mine) const {   // ... and every lane reads its own back
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; k++) mine[k] = et[threadIdx.x * N + k];
    }
    __device__ void store(double* dst) const { if (threadIdx.x < N) dst[threadIdx.x] = s; }
};

// Summary: E_f of a full tile that hands a state on (the tile or what stands for it is in LDS, complete) into E[0, N): every run from zero state,
// the fold from zero in run order.  e: LDS, [kDspLanes * N]
template <class Sys>
__device__ __forceinline__ void scan_summary(const Sys& sc, const float* tile, double* e, double* E) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x;
    double z[N] = {};
    sc.run(tile + l * kDspRun, kDspRun, z);
#pragma unroll
    for (int k = 0; k < N; k++) e[l * N + k] = z[k];
    __syncthreads();
    LaneFold<N> t(sc.a_run, nullptr);
    for (int j = 0; j < kDspLanes; j++) t.advance(e + j * N);
    t.store(E);
}

// Carry: a window of F >= 1 tiles, S_f of every tile from the E_f (scan_E<N>, scan_S<N> of states), 64 tiles at a time; the state is carried from
// one group of 64 to the next.  ein: LDS, [kDspLanes * N].  carry (null: the row starts here, from zero state, and ends here): the state the window
// in front left, and, behind an open window's last tile, the state it leaves (win_hands: the tiles that hand on)
template <class Sys>
__device__ __forceinline__ void scan_carry(const Sys& sc, int64_t F, double* states, double* ein, double* carry, bool open) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x;
    const int64_t hands = win_hands(F, open);
    LaneFold<N> S(sc.a_tile, carry);   // the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) {
#pragma unroll
            for (int k = 0; k < N; k++) ein[l * N + k] = scan_E<N>(states, f)[k];
        }
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            S.store(scan_S<N>(states, c0 + j));
            if (c0 + j < hands) S.advance(ein + j * N);
        }
        __syncthreads();
    }
    if (open) S.store(carry);
}

// Enter: z <- the state entering the lane's run (c samples at `run`, in LDS) of a tile entered in state S[0, N): every run from zero state, the
// fold in run order from S, of which lane l keeps t_l (et: LDS, [kDspLanes * N]).  (Behind a run that is not full no run follows: its t is not read.)
template <class Sys>
__device__ __forceinline__ void scan_enter(const Sys& sc, const float* run, int c, const double* S, double* et, double* z) {
    constexpr int N = Sys::N;
    const int l = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; k++) z[k] = 0.0;
    sc.run(run, c, z);
#pragma unroll
    for (int k = 0; k < N; k++) et[l * N + k] = z[k];
    __syncthreads();
    LaneFold<N> t(sc.a_run, S);
    for (int j = 0; j < kDspLanes; j++) t.enter_step(et + j * N, j, z);
    t.entered(et, z);
}

// ---- the compressor's detector (compressor.h) on a tile's samples or on a band of them: src, in LDS, lane l on src + l * kDspRun ----

// The (max, times) fold (compressor.h cmp_fold_p) over a tile's runs from state S: e[l] is run l's end state from zero (LDS, [kDspLanes],
// complete), rho_run the release's power kDspRun.  Every lane evaluates it alike (a broadcast read) and returns the state entering its own run;
// *behind receives the state behind the last run
__device__ __forceinline__ double fold_enter_max(double rho_run, const double* e, double S, double* behind) {
    const int l = threadIdx.x;
    double t = S, mine = S;
    for (int j = 0; j < kDspLanes; j++) {
        if (j == l) mine = t;
        t = cmp_fold_p(rho_run, t, e[j]);
    }
    *behind = t;
    return mine;
}
// The attack smoothing as a system of one state (compressor.h: the linear scan with N = 1): a run recomputes the detector from p, the detector
// state entering it
struct CmpSmooth {
    static constexpr int N = 1;
    const CmpScan& d;
    double p, a_run[1], a_tile[1];
    __device__ CmpSmooth(const CmpScan& d_, double p_) : d(d_), p(p_), a_run{d_.alpha_run}, a_tile{d_.alpha_tile} {}
    __device__ void run(const float* x, int count, double* z) const { z[0] = cmp_run_s(d, x, count, p, z[0]); }
};

// tp, the detector state entering the lane's run of c samples, from S_f of tile blockIdx.x in p_tiles; e: LDS, [kDspLanes], for all four
__device__ __forceinline__ double det_enter_p(const CmpScan& d, const float* src, int c, double* p_tiles, double* e) {
    e[threadIdx.x] = cmp_run_p(d, src + threadIdx.x * kDspRun, c, 0.0);
    __syncthreads();
    double behind;
    const double tp = fold_enter_max(d.rho_run, e, scan_S<1>(p_tiles, blockIdx.x)[0], &behind);
    __syncthreads();   // e may be written again
    return tp;
}
// ts, the smoothing state entering it, from tp and S_f in s_tiles
__device__ __forceinline__ double det_enter_s(const CmpScan& d, const float* src, int c, double tp, double* s_tiles, double* e) {
    double ts;
    scan_enter(CmpSmooth(d, tp), src + threadIdx.x * kDspRun, c, scan_S<1>(s_tiles, blockIdx.x), e, &ts);
    return ts;
}
// E_f of a handing tile: the detector's into p_tiles, the smoothing's (behind the detector's carry) into s_tiles
__device__ __forceinline__ void det_summary_p(const CmpScan& d, const float* src, double* p_tiles, double* e) {
    e[threadIdx.x] = cmp_run_p(d, src + threadIdx.x * kDspRun, kDspRun, 0.0);
    __syncthreads();
    double E;
    fold_enter_max(d.rho_run, e, 0.0, &E);
    if (threadIdx.x == 0) scan_E<1>(p_tiles, blockIdx.x)[0] = E;
}
__device__ __forceinline__ void det_summary_s(const CmpScan& d, const float* src, double* p_tiles, double* s_tiles, double* e) {
    const double tp = det_enter_p(d, src, kDspRun, p_tiles, e);
    scan_summary(CmpSmooth(d, tp), src, e, scan_E<1>(s_tiles, blockIdx.x));
}

// The detector's carry: scan_carry with S_(f+1) = max(rho_tile S_f, E_f) (cmp_fold_p) in the place of the sum, by every lane alike (lane 0 stores)
__device__ __forceinline__ void carry_max(double rho_tile, int64_t F, double* states, double* ein, double* carry, bool open) {
    const int l = threadIdx.x;
    const int64_t hands = win_hands(F, open);
    double s = carry ? *carry : 0.0;   // the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) ein[l] = scan_E<1>(states, f)[0];
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            if (l == 0) scan_S<1>(states, c0 + j)[0] = s;
            if (c0 + j < hands) s = cmp_fold_p(rho_tile, s, ein[j]);
        }
        __syncthreads();
    }
    if (open && l == 0) *carry = s;
}

// ---- launches ----
// The pair every level of a scan launches: the summary over the handing tiles (hands of them in the longest row: none, no launch), then the carry,
// one workgroup per row
template <class KS, class KC, class... Args>
inline void launch_scan_pair(const char* summary_name, KS summary, const char* carry_name, KC carry, int hands, int n, hipStream_t stream, Args... args) {
    if (hands > 0) {
        note_launch(summary_name);
        hipLaunchKernelGGL(summary, dim3((unsigned)hands, (unsigned)n), dim3(kDspLanes), 0, stream, args...);
    }
    note_launch(carry_name);
    hipLaunchKernelGGL(carry, dim3((unsigned)n), dim3(kDspLanes), 0, stream, args...);
}

}  // namespace ptts
