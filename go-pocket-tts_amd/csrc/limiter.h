// limiter.h -- a request's look-ahead peak limiter (include/ptts.h ptts_limiter_opts, ptts_limit_*), written once for the
// host (limiter.cpp) and the device (limiter.hip).  No HIP header: limiter.cpp builds with a plain C++ compiler.
//
// The stage behind the fades and in front of the true-peak ceiling, on the 24 kHz row x[0, n), float64 throughout.  With c the linear ceiling,
// d the linear drive, L the look-ahead in samples (6 .. 120), rho = exp(-1 / (release_ms * 24)) and inv = 1.0 / (L + 1):
//     a[i] = |(double)x[i]| d                                    the level; a NaN never wins and reads as 0, as in k_dsp_peak
//     m[i] = max a[j], j in [i, i + L]                            the look-ahead peak hold; samples at or beyond n read as 0
//     p[i] = (m[i] > rho p[i-1]) ? m[i] : rho p[i-1], p[-1] = 0   the release
//     r[i] = (p[i] > c) ? (float)(c / p[i]) : 1.0f                the required gain: one IEEE division, rounded once to f32; r[i] = r[0] for i < 0
//     g[i] = (r[i] + r[i-1] + ... + r[i-L]) inv                   the smoothed gain: a float64 sum in exactly that order, from its first term
//     y[i] = (float)((((double)x[i]) d) g[i])                     rounded once
// No step is a nonlinear recurrence:
//   m   is a sliding maximum.  A maximum has no order, and rounding is monotone, so max_j fl(|x[j]| d) = fl((max_j |x[j]|) d) for d > 0: the
//       hold is taken on the f32 magnitudes (lim_mag, lim_hold) and multiplied by d once per sample (lim_level).  Any algorithm gives the bits.
//   p   is compressor.h's detector, linear in the (max, times) semiring, in the same blocked form on the grid of scan_block.h, and the blocked
//       form IS the definition (lim_apply_blocked is ptts_limit_apply):  e_l the run's end state from p = 0 (lim_run_p);  t_0 = S_f,
//       t_(l+1) = max(rho^30 t_l, e_l) (cmp_fold_p, in run order);  E_f the same fold from 0;  S_(f+1) = max(rho^1920 S_f, E_f).  Inside a run p
//       is the recurrence itself from t_l.  It differs from the sample-by-sample release by a few float64 steps and by nothing in any f32
//       output seen so far (tests/test_limiter_cpu.py holds it to one f32 step at the row's peak).
//   g   is a box mean with ONE order of summation (lim_box).  A running sum or a difference of prefix sums would have another and is not
//       this function.
// What follows from it:
//   - Every one of the L + 1 terms of g[i] comes from a sample j in [i - L, i], whose hold window [j, j + L] contains sample i (for j < 0 the
//     term is r[0], and i <= L then).  So p[j] >= m[j] >= a[i], r[j] a[i] <= c (1 + 2^-24), and with the roundings of the sum, of the product
//     by inv, of the two products of y and of y itself: |y[i]| <= c (1 + 2^-22).
//   - Where every p[j], j in [i - L, i], is at or under c -- the signal times d has been under the ceiling for long enough -- the sum is
//     exactly L + 1 and g[i] = (L + 1) inv, which is 1 or the double just below 1 (L + 1 = 49, 98, 103, 107: one float64 division does not
//     always undo itself).  With drive_db = 0 the product (double)x g rounds back to x either way: the sample comes back bit for bit.
//   - y[i] depends on x[0, i + L] only.
//   - It limits SAMPLE peaks at 24 kHz.  The static true-peak ceiling may follow it and then has only the inter-sample remainder to take off.
// Non-finite samples are not treated specially.  A NaN sample never enters the hold and comes out as NaN; its neighbours are untouched.  An
// infinite sample makes m, and with it p, +inf from L samples in front of it to the end of the row (rho * inf = inf), so r is 0 there: the
// gain falls to 0 over the L + 1 samples in front, the infinite sample itself comes out as NaN (inf * 0), and every later finite sample as a
// zero.
#pragma once
#include <string>

#include "compressor.h"

struct ptts_limiter_opts;

namespace ptts {

// A designed limiter (limiter.cpp lim_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct LimScan {
    double c, d;                     // the linear ceiling 10^(ceiling_db / 20) and drive 10^(drive_db / 20)
    double rho, rho_run, rho_tile;   // the release, and its powers kDspRun and kDspTile by repeated multiplication (scan_powers<1>)
    double inv;                      // 1.0 / (L + 1)
    int32_t L, pad;                  // the look-ahead in samples, lrint(lookahead_ms * 24): 6 .. kLimMaxAhead
    double pad2;
};

constexpr int kLimMaxAhead = 120;   // 5 ms

// |x| as an f32, a NaN as 0: what the hold sees
PTTS_HD inline float lim_mag(float x) {
    const float a = __builtin_fabsf(x);
    return (a > 0.0f) ? a : 0.0f;
}

// the hold over one run: m[i] = max ax[i .. i + L] for i in [0, kDspRun).  ax[0, kDspRun + L) are magnitudes (lim_mag: no NaN, none negative),
// zero at and beyond the row's end.  The windows of a run share ax[kDspRun - 1 .. L] when L reaches that far; what lies in front of and
// behind the shared part is a suffix and a prefix maximum
PTTS_HD inline void lim_hold(const float* ax, int L, float (&m)[kDspRun]) {
    if (L >= kDspRun - 1) {
        float C = 0.0f;
        for (int j = kDspRun - 1; j <= L; j++) C = (ax[j] > C) ? ax[j] : C;
        float s = C;
        m[kDspRun - 1] = C;
#pragma unroll
        for (int i = kDspRun - 2; i >= 0; i--) { s = (ax[i] > s) ? ax[i] : s; m[i] = s; }
        float q = 0.0f;
#pragma unroll
        for (int i = 1; i < kDspRun; i++) { q = (ax[L + i] > q) ? ax[L + i] : q; m[i] = (q > m[i]) ? q : m[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < kDspRun; i++) {
            float v = ax[i];
            for (int j = 1; j <= L; j++) v = (ax[i + j] > v) ? ax[i + j] : v;
            m[i] = v;
        }
    }
}
// m[i] as the level: the one product by d
PTTS_HD inline double lim_level(const LimScan& d, float m) {
#pragma clang fp contract(off)
    return (double)m * d.d;
}

// the release over the first `count` samples of a run from state p: the state behind them
PTTS_HD inline double lim_run_p(const LimScan& d, const float (&m)[kDspRun], int count, double p) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < kDspRun; i++) {
        if (i < count) {
            const double a = lim_level(d, m[i]), r = d.rho * p;
            p = (a > r) ? a : r;
        }
    }
    return p;
}
// the run itself from its entering state: r[0, count) receives the required gains
PTTS_HD inline void lim_run_r(const LimScan& d, const float (&m)[kDspRun], int count, double p, float* r) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < kDspRun; i++) {
        if (i < count) {
            const double a = lim_level(d, m[i]), q = d.rho * p;
            p = (a > q) ? a : q;
            r[i] = (p > d.c) ? (float)loud_div(d.c, p) : 1.0f;
        }
    }
}
// g[i]: r points at r[i], and r[-L .. 0] are there (r[0] of the row in the places in front of it)
PTTS_HD inline double lim_box(const LimScan& d, const float* r) {
#pragma clang fp contract(off)
    double s = (double)r[0];
    for (int k = 1; k <= d.L; k++) s = s + (double)r[-k];
    return s * d.inv;
}
// g[i] where every one of its terms is 1.0f: the same sum, which is exactly L + 1
PTTS_HD inline double lim_box_ones(const LimScan& d) {
#pragma clang fp contract(off)
    return (double)(d.L + 1) * d.inv;
}
PTTS_HD inline float lim_out(const LimScan& d, float x, double g) {
#pragma clang fp contract(off)
    return (float)(((double)x * d.d) * g);
}

// A row's scratch: the release's per-tile states, [F][2] doubles (E_f then S_f; scan_E<1>, scan_S<1>), then r, one f32 a sample
PTTS_HD inline size_t lim_scratch_doubles(int64_t n) { return scan_state_doubles<1>(scan_tiles(n)) + (size_t)((n + 1) / 2); }

// ---- the host side (limiter.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, every field in its range); otherwise the message, naming the field
std::string lim_opts_error(const ptts_limiter_opts* l);
// the design of well-formed options
LimScan lim_design(const ptts_limiter_opts& l);
// the limiter over x[0, n) in place, in blocked form: what the k_lim_* kernels compute for one row
void lim_apply_blocked(const LimScan& d, float* x, int64_t n);

}  // namespace ptts
