// compressor.h -- a request's dynamic range compressor (include/ptts.h ptts_compressor_opts, ptts_compress_*), written
// once for the host (compressor.cpp) and the device (compressor.hip).  No HIP header: compressor.cpp builds with a plain C++ compiler.
//
// A feed-forward compressor on the 24 kHz row, float64 throughout.  Per sample, from p = s = 0:
//     a = |x|                                   (as a double)
//     p = (a > rho p) ? a : rho p               the peak detector with release; a NaN never wins, as in k_dsp_peak
//     s = alpha s + (1 - alpha) p               the attack smoothing
//     g = curve(s)                              the soft-knee curve of Giannoulis, Massberg and Reiss (JAES 60(6), 2012) plus the makeup gain
//     y = (float)((double)x * g)                rounded once
// with rho = exp(-1 / (release_ms * 24)) and alpha = exp(-1 / (attack_ms * 24)).  With L = 20 log10 s, T the threshold, W the knee, R the ratio:
//     2 (L - T) < -W : 0 dB        2 (L - T) > W : (1 / R - 1) (L - T)        between : (1 / R - 1) (L - T + W / 2)^2 / (2 W)
//
// Both recurrences are evaluated in blocked form on the grid of scan_block.h (runs of kDspRun samples, tiles of kDspTile), and the blocked form IS
// the definition (cmp_apply_blocked is ptts_compress_apply):
//   p   is linear in the (max, times) semiring.  Rounding is monotone, so max(fl(c a), fl(c b)) = fl(c max(a, b)) and the summary / carry / apply
//       decomposition of a linear scan holds with max in the place of +:  e_l the run's end state from p = 0 (cmp_run_p);
//       t_0 = S_f, t_(l+1) = max(rho^30 t_l, e_l) (cmp_fold_p, in run order);  E_f the same fold from 0;  S_(f+1) = max(rho^1920 S_f, E_f).
//       Inside a run p is the recurrence itself from t_l.  (rho^30 t in one product is not thirty products by rho: the blocked level differs
//       from the sample-by-sample one by a few float64 steps, and by nothing in any f32 output seen so far.)
//   s   is the linear scan of scan_block.h with N = 1 (scan_advance<1>): its runs recompute p from their entering p state t_l.
// log2 and exp2 are this header's own: the exponent taken from and put into the bits (exact), a fixed polynomial in separate float64 products and
// sums, one IEEE division.  No libm, no ocml: host and device give the same bits.  The linear gain agrees with the libm statement
// 10^(gain_db / 20) to far better than 2^-30 relative (tests/test_compressor_cpu.py), well under half an f32 step.
// A level at or under the knee's lower edge (s <= s_lo, a double made at design time) takes the constant makeup gain g_lo; neither function is
// evaluated there, so silence costs nothing and log2 never sees a zero.
// Non-finite samples are not treated specially.  A NaN sample never enters the detector and comes out as NaN; its neighbours are untouched.  An
// infinite sample makes p, and with it s, +inf for the rest of the row (rho * inf = inf); cmp_log2 reads +inf as 2^1024, so L is 6165.09 dB and
// the gain is the curve's value there: with a ratio above 1 it is so small that every later finite sample rounds to a zero, the infinite
// sample itself stays infinite (NaN where the gain underflows to 0: cmp_exp2 returns 0 under 2^-1020); with ratio 1 the row is unchanged.
#pragma once
#include <string>

#include "scan_block.h"

struct ptts_compressor_opts;

namespace ptts {

// A designed compressor (compressor.cpp cmp_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct CmpScan {
    double rho, alpha, beta;                             // beta = 1 - alpha
    double rho_run, rho_tile, alpha_run, alpha_tile;     // the powers kDspRun and kDspTile, by repeated multiplication (scan_powers<1>)
    double thr_db, knee_db, slope, knee_q, makeup_db;    // slope = 1 / R - 1; knee_q = slope / (2 W), 0 for a hard knee
    double s_lo, g_lo;                                   // the level of the knee's lower edge, 10^((T - W / 2) / 20); the gain at or under it
    double pad[2];
};

constexpr double kCmpDbPerLog2 = 6.020599913279624;      // 20 log10(2)
constexpr double kCmpLog2PerDb = 0.16609640474436813;    // log2(10) / 20

PTTS_HD inline uint64_t cmp_bits(double v) { uint64_t b; __builtin_memcpy(&b, &v, sizeof b); return b; }
PTTS_HD inline double cmp_double(uint64_t b) { double v; __builtin_memcpy(&v, &b, sizeof v); return v; }

// log2 of a positive normal double (+inf reads as 2^1024).  s = m 2^e with m in [sqrt(1/2), sqrt(2)); ln m = 2 atanh(t), t = (m - 1) / (m + 1),
// |t| < 0.1716, the series up to t^15 (the first term left out is under 4e-14 of the sum)
PTTS_HD inline double cmp_log2(double s) {
#pragma clang fp contract(off)
    const uint64_t b = cmp_bits(s);
    int e = (int)((b >> 52) & 0x7ff) - 1022;
    double m = cmp_double((b & 0x000fffffffffffffull) | 0x3fe0000000000000ull);   // [0.5, 1)
    if (m < 0.70710678118654757) { m = m * 2.0; e = e - 1; }
    const double t = loud_div(m - 1.0, m + 1.0);
    const double w = t * t;
    double q = 1.0 / 15.0;
    q = q * w + 1.0 / 13.0;
    q = q * w + 1.0 / 11.0;
    q = q * w + 1.0 / 9.0;
    q = q * w + 1.0 / 7.0;
    q = q * w + 1.0 / 5.0;
    q = q * w + 1.0 / 3.0;
    q = q * w + 1.0;
    return (double)e + (t * q) * 2.8853900817779268;   // 2 / ln 2
}

// 2^v for v under 1023 (not a NaN); 0 under 2^-1020.  v = k + f, |f| <= 1/2, 2^f = exp(f ln 2) as its series up to the 11th power (the first
// term left out is under 7e-15), the exponent put into the bits
PTTS_HD inline double cmp_exp2(double v) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)(v < 0.0 ? v - 0.5 : v + 0.5);
    if (k < -1020) return 0.0;
    const double z = (v - (double)k) * 0.69314718055994529;
    double q = 1.0 / 39916800.0;
    q = q * z + 1.0 / 3628800.0;
    q = q * z + 1.0 / 362880.0;
    q = q * z + 1.0 / 40320.0;
    q = q * z + 1.0 / 5040.0;
    q = q * z + 1.0 / 720.0;
    q = q * z + 1.0 / 120.0;
    q = q * z + 1.0 / 24.0;
    q = q * z + 1.0 / 6.0;
    q = q * z + 0.5;
    q = q * z + 1.0;
    q = q * z + 1.0;
    return q * cmp_double((uint64_t)(k + 1023) << 52);
}

// the static curve in dB at a level s above the knee's lower edge (s > s_lo, +inf included, never a NaN), without the makeup gain (deesser.h
// holds it against its floor)
PTTS_HD inline double cmp_curve_db(const CmpScan& d, double s) {
#pragma clang fp contract(off)
    const double over = kCmpDbPerLog2 * cmp_log2(s) - d.thr_db, two = 2.0 * over;
    double g_db;
    if (two > d.knee_db) g_db = d.slope * over;
    else if (two < -d.knee_db) g_db = 0.0;
    else { const double h = over + 0.5 * d.knee_db; g_db = d.knee_q * (h * h); }
    return g_db;
}
// the linear gain at level s (s >= 0 or +inf, never a NaN): the static curve and the makeup gain
PTTS_HD inline double cmp_gain(const CmpScan& d, double s) {
#pragma clang fp contract(off)
    if (!(s > d.s_lo)) return d.g_lo;
    return cmp_exp2((cmp_curve_db(d, s) + d.makeup_db) * kCmpLog2PerDb);
}

// one sample of each recurrence: the detector from p at the level a = |x| (a NaN never wins), the smoothing from s at the detector's new state
PTTS_HD inline double cmp_step_p(const CmpScan& d, double a, double p) {
#pragma clang fp contract(off)
    const double r = d.rho * p;
    return (a > r) ? a : r;
}
PTTS_HD inline double cmp_step_s(const CmpScan& d, double p, double s) {
#pragma clang fp contract(off)
    return d.alpha * s + d.beta * p;
}

// the detector over `count` samples from state p: the state behind them
PTTS_HD inline double cmp_run_p(const CmpScan& d, const float* x, int count, double p) {
#pragma clang fp contract(off)
    for (int i = 0; i < count; i++) p = cmp_step_p(d, __builtin_fabs((double)x[i]), p);
    return p;
}
// t_(l+1) = max(pw t_l, e_l), S_(f+1) = max(pw S_f, E_f): e is never a NaN
PTTS_HD inline double cmp_fold_p(double pw, double t, double e) {
#pragma clang fp contract(off)
    const double r = pw * t;
    return (e > r) ? e : r;
}
// detector and smoothing over `count` samples, the detector from p and the smoothing from s: the smoothing's state behind them
PTTS_HD inline double cmp_run_s(const CmpScan& d, const float* x, int count, double p, double s) {
#pragma clang fp contract(off)
    for (int i = 0; i < count; i++) {
        p = cmp_step_p(d, __builtin_fabs((double)x[i]), p);
        s = cmp_step_s(d, p, s);
    }
    return s;
}
// the run itself from its entering states: y (may be x) receives the compressed samples
PTTS_HD inline void cmp_run_y(const CmpScan& d, const float* x, int count, double p, double s, float* y) {
#pragma clang fp contract(off)
    for (int i = 0; i < count; i++) {
        const double xi = (double)x[i];
        p = cmp_step_p(d, __builtin_fabs(xi), p);
        s = cmp_step_s(d, p, s);
        y[i] = (float)(xi * cmp_gain(d, s));
    }
}

// The detector's tile step on the host: tp[l] and ts[l], the detector and the smoothing state entering run l of src[0, cnt) (a tile's samples, or the
// de-esser's band of them; tp, ts: [kDspLanes]), from the states Sp and Ss entering the tile, which are left at the states behind it.  Inline: called out of line, cmp_apply_blocked measured 3 % slower
inline void cmp_tile_states(const CmpScan& d, const float* src, int cnt, double& Sp, double& Ss, double* tp, double* ts) {
    double t = Sp, Ep = 0.0;
    for (int l = 0; l < kDspLanes; l++) {
        const double e = cmp_run_p(d, src + l * kDspRun, scan_run_count(cnt, l), 0.0);
        tp[l] = t;
        t = cmp_fold_p(d.rho_run, t, e);
        Ep = cmp_fold_p(d.rho_run, Ep, e);
    }
    double u[1] = {Ss}, Es[1] = {0.0};
    for (int l = 0; l < kDspLanes; l++) {
        const double e[1] = {cmp_run_s(d, src + l * kDspRun, scan_run_count(cnt, l), tp[l], 0.0)};
        ts[l] = u[0];
        scan_advance<1>(&d.alpha_run, u, e);
        scan_advance<1>(&d.alpha_run, Es, e);
    }
    Sp = cmp_fold_p(d.rho_tile, Sp, Ep);
    scan_advance<1>(&d.alpha_tile, &Ss, Es);
}

// A row's per-tile states in scratch: [F][2] doubles for each of the two recurrences, E_f then S_f (scan_E<1>, scan_S<1>)
PTTS_HD inline size_t cmp_state_doubles(int64_t F) { return 2 * scan_state_doubles<1>(F); }

// ---- the host side (compressor.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, every field in its range); otherwise the message, naming the field
std::string cmp_opts_error(const ptts_compressor_opts* c);
// the design of well-formed options
CmpScan cmp_design(const ptts_compressor_opts& c);
// the compressor over x[0, n) in place, in blocked form: what the five k_cmp_* kernels compute for one row
void cmp_apply_blocked(const CmpScan& d, float* x, int64_t n);

}  // namespace ptts
