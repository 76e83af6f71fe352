// scan_block.h -- the post-processing recurrences in blocked form, written once for the host and the device (dsp.hip's kernels; dsp.cpp's
// dsp_dc_block_blocked, which a CPU test drives through libptts_hooks.so; loudness.cpp's loud_measure, which IS ptts_loudness).  DESIGN.md
// section 8 (N3).
//
// A cascade of biquads (direct form II transposed, float64 state) is a linear system with N states
//     z' = A z + B x
// so a run of samples started from state z gives what the same run gives from state 0 plus the free response of z, and the state behind
// the run is A^len z + e with e the end state of the zero-state run.  A row is cut on a grid that depends on nothing but the sample index:
// tiles of kDspTile samples (one decoder frame), each of kDspLanes runs of kDspRun samples.
//     e_l          end state of run l from zero state                              (Sys::run, parallel over runs)
//     t_0 = S_f,   t_(l+1) = A^kDspRun t_l + e_l                                   (scan_advance, in run order)
//     E_f = the same fold from t_0 = 0;   S_(f+1) = A^kDspTile S_f + E_f           (in tile order)
//     run l again  the recurrence itself, started from t_l                         (Sys::run: its outputs, or the sum of their squares)
// Two systems: the DC block (DspScan, N = 2: one section, y = b0 x + z1, A = [[-a1, 1], [-a2, 0]]) and the K-weighting of BS.1770-4 at
// 24 kHz (LoudScan, N = 4: a high shelf, then a high-pass, z = (shelf z1, shelf z2, high-pass z1, high-pass z2)).  A third, per request: the
// equaliser (EqScan seen as EqSys<S>, N = 2 S for S = 1 .. 4 sections of the caller's choice; eq.cpp's eq_apply_blocked IS ptts_eq_apply).
// Loudness energies: a sub-block is kLoudSub = 480 samples = 16 runs (a tile has 4, the 100 ms hop 5, the 400 ms block 20); its energy is the
// sum of its runs' sums of squares in run order; block j (samples [2400 j, 2400 j + 9600), whole blocks only) is the sum of its 20 sub-blocks
// in order, over 9600.  Gating is linear: the absolute gate z > abs_gate, the relative gate z > 0.1 * mean of the absolutely gated z, M the
// mean of the doubly gated z, all sums in block order.  No logarithm here: LUFS = -0.691 + 10 log10(M) is the host's.
// Every product and sum below is a separate float64 operation (no contraction); the division and the square root are the correctly rounded
// IEEE operations on both sides, so the host and the device instantiation agree bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTTS_HD __host__ __device__
#else
#define PTTS_HD
#endif

namespace ptts {

constexpr int kDspRun = 30, kDspLanes = 64, kDspTile = kDspRun * kDspLanes;   // 1920 = samples per frame at 24 kHz

struct DspBiquad { double b0, b1, b2, a1, a2; };

// s <- P s + e (P row-major N x N): each row's products summed left to right, then e[i]
template <int N>
PTTS_HD inline void scan_advance(const double* P, double* s, const double* e) {
#pragma clang fp contract(off)
    double n[N];
    for (int i = 0; i < N; i++) {
        double v = P[N * i] * s[0];
        for (int m = 1; m < N; m++) v = v + P[N * i + m] * s[m];
        n[i] = v + e[i];
    }
    for (int i = 0; i < N; i++) s[i] = n[i];
}

// a_run = A^kDspRun and a_tile = A^kDspTile of a state matrix A (row-major N x N), by repeated multiplication Q = A P on the host.  A sum
// starts from its first product, not from 0.0: a 0.0 in front could turn an exact -0 into +0.
template <int N>
inline void scan_powers(const double* A, double* a_run, double* a_tile) {
#pragma clang fp contract(off)
    double P[N * N], Q[N * N];
    for (int i = 0; i < N * N; i++) P[i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
    for (int k = 1; k <= kDspTile; k++) {
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                double v = A[N * i] * P[j];
                for (int m = 1; m < N; m++) v = v + A[N * i + m] * P[N * m + j];
                Q[N * i + j] = v;
            }
        for (int j = 0; j < N * N; j++) P[j] = Q[j];
        if (k == kDspRun) for (int j = 0; j < N * N; j++) a_run[j] = P[j];
    }
    for (int j = 0; j < N * N; j++) a_tile[j] = P[j];
}

// A system: its sections, the two powers of A the blocked form needs (made on the host, passed by value) and run(): `count` samples from
// state z, which is left at the state behind them.

// the DC block (dsp_scan_coeffs): y (optional, may be x) receives the outputs rounded to f32
struct DspScan {
    static constexpr int N = 2;
    DspBiquad c;
    double a_run[N * N], a_tile[N * N];
    PTTS_HD void run(const float* x, int count, double* z, float* y = nullptr) const {
#pragma clang fp contract(off)
        double z1 = z[0], z2 = z[1];
        for (int i = 0; i < count; i++) {
            const double xi = (double)x[i];
            const double yi = c.b0 * xi + z1;
            z1 = c.b1 * xi - c.a1 * yi + z2;
            z2 = c.b2 * xi - c.a2 * yi;
            if (y) y[i] = (float)yi;
        }
        z[0] = z1; z[1] = z2;
    }
};

// the K-weighting cascade and the absolute gate 10^((-70 + 0.691) / 10) (loud_scan_coeffs): returns the sum of the squared outputs in
// sample order
struct LoudScan {
    static constexpr int N = 4;
    DspBiquad s1, s2;
    double a_run[N * N], a_tile[N * N];
    double abs_gate;
    PTTS_HD double run(const float* x, int count, double* z) const {
#pragma clang fp contract(off)
        double q = 0.0;
        double z1 = z[0], z2 = z[1], z3 = z[2], z4 = z[3];
        for (int i = 0; i < count; i++) {
            const double xi = (double)x[i];
            const double u = s1.b0 * xi + z1;
            z1 = s1.b1 * xi - s1.a1 * u + z2;
            z2 = s1.b2 * xi - s1.a2 * u;
            const double y = s2.b0 * u + z3;
            z3 = s2.b1 * u - s2.a1 * y + z4;
            z4 = s2.b2 * u - s2.a2 * y;
            q = q + y * y;
        }
        z[0] = z1; z[1] = z2; z[2] = z3; z[3] = z4;
        return q;
    }
};

// a request's equaliser (eq.cpp, ptts_eq): S = 1 .. 4 sections chosen by the caller, N = 2 S states z = (section 0 z1, z2, section 1 z1, ...);
// a_run and a_tile are N x N row-major, packed at the front.  It travels to the device as it is, behind a table's rows (dsp_device.cpp).
constexpr int kEqMaxSections = 4;
struct EqScan {
    int32_t S, pad;
    DspBiquad c[kEqMaxSections];
    double a_run[4 * kEqMaxSections * kEqMaxSections], a_tile[4 * kEqMaxSections * kEqMaxSections];
};
// ... seen as a system of S sections: only those are evaluated (an identity section in an unused place would turn -0 into +0).  y (optional,
// may be x) receives the outputs rounded to f32
template <int S_>
struct EqSys {
    static constexpr int S = S_, N = 2 * S_;
    const DspBiquad* c;
    const double *a_run, *a_tile;
    PTTS_HD explicit EqSys(const EqScan& e) : c(e.c), a_run(e.a_run), a_tile(e.a_tile) {}
    PTTS_HD EqSys(const DspBiquad* c_, const double* a_run_, const double* a_tile_) : c(c_), a_run(a_run_), a_tile(a_tile_) {}   // (deesser.h: a design that holds one section)
    PTTS_HD void run(const float* x, int count, double* z, float* y = nullptr) const {
#pragma clang fp contract(off)
        double w[N];
        for (int k = 0; k < N; k++) w[k] = z[k];
        for (int i = 0; i < count; i++) {
            double v = (double)x[i];
            for (int k = 0; k < S; k++) {
                const DspBiquad& q = c[k];
                const double u = q.b0 * v + w[2 * k];
                w[2 * k] = q.b1 * v - q.a1 * u + w[2 * k + 1];
                w[2 * k + 1] = q.b2 * v - q.a2 * u;
                v = u;
            }
            if (y) y[i] = (float)v;
        }
        for (int k = 0; k < N; k++) z[k] = w[k];
    }
};
// f(EqSys<S>) for the equaliser's section count (1 .. kEqMaxSections, checked where it was made)
template <class F>
PTTS_HD inline void eq_dispatch(const EqScan& e, F&& f) {
    switch (e.S) {
        case 1: f(EqSys<1>(e)); break;
        case 2: f(EqSys<2>(e)); break;
        case 3: f(EqSys<3>(e)); break;
        case 4: f(EqSys<4>(e)); break;
        default: break;
    }
}

// A row's per-tile states in scratch: [F = ceil(n / kDspTile)][2 N] doubles, E_f (N) then S_f (N)
PTTS_HD inline int64_t scan_tiles(int64_t n) { return (n + kDspTile - 1) / kDspTile; }
// ... and of a window of it: the tiles from t0 to the end of the first n samples (kernels.h has what a window is)
PTTS_HD inline int64_t win_tiles(int64_t t0, int64_t n) { return scan_tiles(n) - t0; }
template <int N> PTTS_HD inline size_t scan_state_doubles(int64_t F) { return (size_t)F * 2 * N; }
template <int N> PTTS_HD inline double* scan_E(double* states, int64_t f) { return states + f * 2 * N; }
template <int N> PTTS_HD inline double* scan_S(double* states, int64_t f) { return states + f * 2 * N + N; }

// samples of run l in a tile of cnt
PTTS_HD inline int scan_run_count(int cnt, int l) { const int c = cnt - l * kDspRun; return c < 0 ? 0 : (c < kDspRun ? c : kDspRun); }

// The host form, a tile of it: x[0, cnt) entered in state S, which is left at the state behind the tile -- the runs from zero state, the fold
// giving each run's entering state and E_f, and each_run(off, count, z) for every run -- samples [off, off + count) of the tile, z its entering
// state (the callback's own arithmetic wants its own pragma)
template <class Sys, class F>
inline void scan_tile(const Sys& sc, const float* x, int cnt, double* S, F&& each_run) {
    constexpr int N = Sys::N;
    double e[kDspLanes][N] = {};
    for (int l = 0; l < kDspLanes; l++) sc.run(x + l * kDspRun, scan_run_count(cnt, l), e[l]);
    double E[N] = {}, t[N];
    for (int i = 0; i < N; i++) t[i] = S[i];
    for (int l = 0; l < kDspLanes; l++) {
        double z[N];
        for (int i = 0; i < N; i++) z[i] = t[i];
        each_run(l * kDspRun, scan_run_count(cnt, l), z);
        scan_advance<N>(sc.a_run, t, e[l]);
        scan_advance<N>(sc.a_run, E, e[l]);
    }
    scan_advance<N>(sc.a_tile, S, E);
}
// ... and the tiles of x[0, n) in order from zero state: each_run(i0, count, z) with i0 counting in the row
template <class Sys, class F>
inline void scan_walk(const Sys& sc, const float* x, int64_t n, F&& each_run) {
    double S[Sys::N] = {};
    for (int64_t base = 0; base < n; base += kDspTile)
        scan_tile(sc, x + base, (int)std::min<int64_t>(kDspTile, n - base), S, [&](int off, int count, double* z) { each_run(base + off, count, z); });
}

// ---- loudness only: energies, gates and the gain ----

constexpr int kLoudSub = 480, kLoudRunsPerSub = kLoudSub / kDspRun, kLoudSubsPerTile = kDspTile / kLoudSub;   // 16 runs, 4 per tile
constexpr int kLoudHopSubs = 5, kLoudBlockSubs = 20;
constexpr int64_t kLoudBlock = (int64_t)kLoudBlockSubs * kLoudSub, kLoudHop = (int64_t)kLoudHopSubs * kLoudSub;   // 9600, 2400
static_assert(kLoudSub % kDspRun == 0 && kDspTile % kLoudSub == 0, "sub-blocks lie on the run grid and tiles on the sub-block grid");

// A loudness row's scratch (kernels.h DspRow::loud): [0] the gated mean square M, [1] the f32 gain in its first four bytes, then the
// K-weighting's per-tile states, then [4 F] sub-block energies
constexpr int kLoudHead = 2;
PTTS_HD inline double* loud_states(double* loud) { return loud + kLoudHead; }
PTTS_HD inline double* loud_subs(double* loud, int64_t F) { return loud_states(loud) + scan_state_doubles<LoudScan::N>(F); }
PTTS_HD inline size_t loud_doubles(int64_t F) { return kLoudHead + scan_state_doubles<LoudScan::N>(F) + (size_t)F * kLoudSubsPerTile; }

PTTS_HD inline int64_t loud_blocks(int64_t n) { return n >= kLoudBlock ? (n - kLoudBlock) / kLoudHop + 1 : 0; }

// sub-block k's energy from its 16 run sums, in run order
PTTS_HD inline double loud_sub_energy(const double* q) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int r = 0; r < kLoudRunsPerSub; r++) s = s + q[r];
    return s;
}

PTTS_HD inline double loud_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

// block j's mean square from the row's sub-block energies
PTTS_HD inline double loud_block_energy(const double* sub, int64_t j) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int k = 0; k < kLoudBlockSubs; k++) s = s + sub[j * kLoudHopSubs + k];
    return loud_div(s, (double)kLoudBlock);
}

// one gate pass over a stretch of block energies in block order: z counts when it is above the absolute gate and above `rel`
struct LoudAcc { double sum; int64_t cnt; };
PTTS_HD inline void loud_gate_add(LoudAcc& a, double z, double abs_gate, double rel) {
#pragma clang fp contract(off)
    if (z > abs_gate && z > rel) { a.sum = a.sum + z; a.cnt++; }
}
PTTS_HD inline double loud_rel_gate(const LoudAcc& a) {   // 0.1 * the mean of the absolutely gated blocks (-10 LU); a: at least one block
#pragma clang fp contract(off)
    return 0.1 * loud_div(a.sum, (double)a.cnt);
}

// The gain that takes mean square M to T = 10^((target + 0.691) / 10), never above 1 / peak (the row's sample peak, k_dsp_peak's: max |x| with
// NaNs ignored, the division of dsp_peak_normalize).  1 when nothing passed the gates (M == 0) or M is not finite.
PTTS_HD inline float loud_gain(double M, double T, float peak) {
    if (!(M > 0.0) || !(M <= 1.7976931348623157e308)) return 1.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    float g = (float)__dsqrt_rn(__ddiv_rn(T, M));
    if (peak > 0.0f) { const float c = __fdiv_rn(1.0f, peak); if (c < g) g = c; }
#else
    float g = (float)std::sqrt(T / M);
    if (peak > 0.0f) { const float c = 1.0f / peak; if (c < g) g = c; }
#endif
    return g;
}

}  // namespace ptts
