// formant.h -- "keep the formants" around the pitch of one part of a joined text (include/ptts.h ptts_formant_opts, ptts_formant_*; DESIGN.md
// section 8, N3): the part's spectral envelope is estimated by linear prediction, the part is flattened with it, only the flat residual goes through
// the pitch's resampler (pitch.h, unchanged), and the envelope is put back on the resampled residual.  The pitch moves by p, the envelope stays.
// Written once for the host (formant.cpp is the statement) and the device (formant.hip).  No HIP header: formant.cpp builds with a plain C++ compiler.
//
// On the 24 kHz row x[0, n) with p = pitch_permille (800 .. 1500 with the option); samples outside a row read as 0.0f; every index is an integer:
//     frames:   K = ceil(n / 240); frame f looks at x[240 f - 240 + j], j in [0, 720): its centre is 240 f + 120.
//     analysis (float64, per frame): v[j] = (double)x * w[j], w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / 720); r[l], l = 0 .. 24: one fma chain from 0.0
//               over ascending j = l .. 719 of v[j] * v[j - l]; r[0] not finite or not > 0: the identity (a[1 .. 24] = 0).  r[l] *= lag[l], with
//               lag[l] = exp(-0.5 (2 pi 60 l / 24000)^2) and lag[0] = 1.0001 (the white-noise factor on exp(0) = 1).  Levinson-Durbin, stage
//               i = 1 .. 24 with E = r[0] at the start: acc = r[i], then over ascending j = 1 .. i - 1 acc = fma(a[j], r[i - j], acc); k = -acc / E;
//               k not finite or |k| >= 1: the identity; a'[j] = a[j] + k * a[i - j] for j = 1 .. i - 1 (a product, then a sum), a'[i] = k;
//               E = E * (1 - k * k) (a product, a difference, a product); E not > 0: the identity.  a32[k] = (float)(a[k] * g[k]), g[k] = 0.99^k.
//               The tables w, lag and g are made once on the host in float64 (formant.cpp) and uploaded as they are.
//     the pair of a source time tau: b = tau - 120, f0 = floor(b / 240), rho = b - 240 f0, fa = clamp(f0, 0, K - 1), fb = clamp(f0 + 1, 0, K - 1),
//               u = (float)rho / 240.0f (one IEEE f32 division), mix(A, B) = A * (1.0f - u) + B * u: one difference, two products, one sum, each
//               rounded once, nothing fused.
//     whiten:   E_f[i] is one f32 chain: acc = x[i], then for k = 1 .. 24 ascending acc = fmaf(a32_f[k], x[i - k], acc);
//               e[i] = mix(E_fa[i], E_fb[i]) with tau = i, i in [0, n).
//     resample: e' = the pitch's resample of e at p, n_r samples.
//     shape:    output j lies in tile t = j / 240, which starts its recursions at m0 = 240 t - 720.  For a frame f, Y[m] for m >= m0 is one f32 chain:
//               acc = e'[m] (0.0f outside [0, n_r)), then for k = 1 .. 24 ascending acc = fmaf(-a32_f[k], Y[m - k], acc), with Y[m] = 0.0f for
//               m < m0.  out[j] = mix(Y_fa[j], Y_fb[j]) with tau = (j * p) / 1000 in int64.  A tile's outputs name at most kFormantSlots = 4
//               consecutive frames (p <= 1500: its source times span less than 2 x 240).
// Every tile restarts from zero state kFormantWarm samples earlier, so tiles are independent and what a NaN or a click reaches is bounded.  The host
// and the device run the same chains in the same order (the functions below, contraction off) and give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ptts.h"
#include "pitch.h"

namespace ptts {

constexpr int kFormantHop = 240;       // Hf: the hop of the frames and the outputs of a shape tile
constexpr int kFormantWin = 720;       // Lw: the samples a frame looks at
constexpr int kFormantOrder = 24;      // P
constexpr int kFormantWarm = 720;      // Tw: how far in front of a shape tile its recursions start from zero state
constexpr int kFormantSlots = 4;       // the frames a shape tile's outputs may name
constexpr int kFormantMinPitch = 800, kFormantMaxPitch = 1500;
constexpr int kFormantTableDoubles = kFormantWin + 2 * (kFormantOrder + 1);   // w[720], lag[25], g[25]

// the option as it travels with a handle and a resolved row
struct FormantScan { int32_t keep; int32_t pad[3]; };

#if defined(__HIP_DEVICE_COMPILE__)   // (the device alone: there the static indices keep the arrays in registers; a host compiler gains nothing from it)
#define PTTS_FORMANT_UNROLL _Pragma("unroll")
#else
#define PTTS_FORMANT_UNROLL
#endif

PTTS_HD inline int64_t formant_frames(int64_t n) { return n > 0 ? (n + kFormantHop - 1) / kFormantHop : 0; }

// the frame pair of a source time and its weight
struct FormantPair { int64_t fa, fb; float u; };
PTTS_HD inline FormantPair formant_pair(int64_t tau, int64_t K) {
    const int64_t b = tau - kFormantHop / 2, f0 = pitch_floor_div(b, kFormantHop), rho = b - kFormantHop * f0;
    FormantPair q;
    q.fa = f0 < 0 ? 0 : f0 > K - 1 ? K - 1 : f0;
    q.fb = f0 + 1 < 0 ? 0 : f0 + 1 > K - 1 ? K - 1 : f0 + 1;
#if defined(__HIP_DEVICE_COMPILE__)
    q.u = __fdiv_rn((float)rho, 240.0f);
#else
    q.u = (float)rho / 240.0f;
#endif
    return q;
}
PTTS_HD inline float formant_mix(float A, float B, float u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float wa = 1.0f - u;
    const float pa = A * wa, pb = B * u;
    return pa + pb;
}

// r[l] of a windowed frame v[0, 720)
PTTS_HD inline double formant_lag(const double* v, int l) {
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 8
#endif
    for (int j = l; j < kFormantWin; j++) acc = __builtin_fma(v[j], v[j - l], acc);   // (unrolled: the reads of eight steps are in flight, acc alone runs through them in order)
    return acc;
}

// The frame's coefficients from its lags r[0 .. 24] (as formant_lag gave them) into out[0 .. 24), a32[1 .. 24]; lag and g: the tables.  Every index
// below is static once the loops are unrolled, so on the device r and a are registers.  The stage's update runs in place on the pairs (j, i - j),
// each from the two old values: the sums of the statement, in another order of evaluation and the same roundings
PTTS_HD inline void formant_solve(const double* lags, const double* lag, const double* g, float* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double r[kFormantOrder + 1], a[kFormantOrder + 1];
    PTTS_FORMANT_UNROLL
    for (int l = 0; l <= kFormantOrder; l++) {
        r[l] = lags[l] * lag[l];
        a[l] = 0.0;
    }
    bool ok = lags[0] - lags[0] == 0.0 && lags[0] > 0.0;   // finite and positive
    double E = r[0];
    PTTS_FORMANT_UNROLL
    for (int i = 1; i <= kFormantOrder; i++) {
        if (!ok) continue;
        double acc = r[i];
        PTTS_FORMANT_UNROLL
        for (int j = 1; j < i; j++) acc = __builtin_fma(a[j], r[i - j], acc);
        const double k = -acc / E;
        if (!(k - k == 0.0) || !(k > -1.0 && k < 1.0)) { ok = false; continue; }
        PTTS_FORMANT_UNROLL
        for (int j = 1; 2 * j < i; j++) {
            const double lo = a[j], hi = a[i - j];
            const double tl = k * hi, th = k * lo;
            a[j] = lo + tl;
            a[i - j] = hi + th;
        }
        if (i % 2 == 0) {
            const double m = a[i / 2];
            const double t = k * m;
            a[i / 2] = m + t;
        }
        a[i] = k;
        const double kk = k * k;
        const double d = 1.0 - kk;
        E = E * d;
        if (!(E > 0.0)) ok = false;
    }
    PTTS_FORMANT_UNROLL
    for (int k = 1; k <= kFormantOrder; k++) {
        const double s = a[k] * g[k];
        out[k - 1] = ok ? (float)s : 0.0f;
    }
}

// E_f[i]: x(i - k) reads the row, 0.0f outside it; a: a32[1 .. 24]
template <class X>
PTTS_HD inline float formant_residual(const float* a, X&& x, int64_t i) {
    float acc = x(i);
    for (int k = 1; k <= kFormantOrder; k++) acc = __builtin_fmaf(a[k - 1], x(i - k), acc);
    return acc;
}

// the frames a shape tile's outputs name: the first of them, for the tile's first output j0 (the others follow it, kFormantSlots at the most)
PTTS_HD inline int64_t formant_tile_first(int64_t j0, int32_t p, int64_t K) { return formant_pair((j0 * (int64_t)p) / 1000, K).fa; }

// ---- the host side (formant.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, keep 0 or 1, reserved 0); otherwise the message, naming the field
std::string formant_opts_error(const ptts_formant_opts* f);
// empty: the option serves the pitch p (800 .. 1500); otherwise the message, naming both fields and both values
std::string formant_pitch_error(int32_t p);
FormantScan formant_design(const ptts_formant_opts& f);
// the tables: w[720], lag[25], g[25], one behind the other (kFormantTableDoubles), made once
const double* formant_tables();
// K x 24 coefficients of x[0, n)
void formant_analyse_host(const float* x, int64_t n, float* coeffs);
// e[0, n) of x[0, n) (not x)
void formant_whiten_host(const float* coeffs, const float* x, int64_t n, float* e);
// out[0, n_r) from the resampled residual e_r[0, n_r) (not e_r), with the K = formant_frames(n) frames of the part in front of the resample
void formant_shape_host(const float* coeffs, int64_t n, int32_t p, const float* e_r, int64_t n_r, float* out);

}  // namespace ptts
