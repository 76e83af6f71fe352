// pitch.h -- the pitch of one part of a joined text (include/ptts.h ptts_pitch_opts, ptts_pitch_*): a resampling by the
// pitch ratio, which scales every frequency (formants too) and the length, followed by the tempo (tempo.h) at the speed that takes the length
// back.  The resampling is band-limited interpolation from ONE prototype table with linearly interpolated coefficients, so any ratio is served
// without a table of its own; written once for the host (pitch.cpp is the statement) and the device (pitch.hip).  No HIP header: pitch.cpp
// builds with a plain C++ compiler.
//
// On the 24 kHz row x[0, n) with p = pitch_permille (500 .. 2000) and s the tempo's speed_permille (1000 without one); every index is an integer:
//     resample: z = x read at step p / 1000, n_r = (n * 1000 + p - 1) / p samples; p == 1000: z is x.
//     tempo:    E = (1000 * s + p / 2) / p (integer division), 500 .. 2000; the tempo's statement on z at speed E; E == 1000: the identity.
// The resample, with R = 256 table steps per input sample, fc = 0.45, W = 80 / 3 samples, Kaiser beta 8.6 (rate_taps.h's prototype):
//     h[q] = (float)(2 fc sinc(2 fc q / R) I0(beta sqrt(1 - (q / (R W))^2)) / I0(beta)) where 3 q < 80 R, else 0: float64 rounded once,
//     kPitchEntries = 6828 of them; hd[q] = h[q + 1] - h[q], one f32 subtraction of the rounded entries (h[6828] is 0).
//     per row D = max(1000, p) and g = (float)(1000.0 / D).
//     out[j], j in [0, n_r), c = j * p (int64): over the inputs i with 3 |c - 1000 i| < 80 D in ascending i, a = |c - 1000 i|,
//     q = (a * R) / D, r = (a * R) % D, frac = (float)r / (float)D (one IEEE f32 division), coef = fmaf(hd[q], frac, h[q]),
//     acc = fmaf(x[i], coef, acc) from 0.0f, x outside [0, n) reading as 0.0f; out[j] = acc * g, one f32 product.
// Nothing else is rounded and nothing else is contracted, so the host and the device give the same bits (outside NaNs, whose bits are the
// processor's).  An input outside the row adds fmaf(0.0f, coef, acc) = acc (acc is never -0.0f), so skipping it is the same statement.
//   - 3 a < 80 D gives q <= 6826: hd[q] reads h up to 6827, inside the table.
//   - a * R stays below 80 * 2000 / 3 * 256: an int32.
//   - rows whose resampled or final length would reach kTempoMaxSamples (2^31 - 240) are refused.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ptts.h"
#include "tempo.h"

namespace ptts {

constexpr int kPitchR = 256;              // R: table steps per input sample
constexpr int kPitchEntries = 6828;       // the q with 3 q < 80 R, and one zero behind them
constexpr int kPitchSupport = 80;         // the support test is 3 a < kPitchSupport * D (W = 80 / 3 samples at D == 1000)

// A designed pitch (pitch.cpp pitch_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct PitchScan {
    int32_t p;      // pitch_permille, 500 .. 2000
    int32_t D;      // max(1000, p)
    float g;        // (float)(1000.0 / D)
    int32_t pad;
};

// the samples of the resampled row; monotone in n
PTTS_HD inline int64_t pitch_resample_length(int64_t n, int32_t p) { return n > 0 ? (n * 1000 + (int64_t)p - 1) / (int64_t)p : 0; }
// the speed the tempo runs at behind the resample, so that the length comes back to what the speed s alone gives
PTTS_HD inline int32_t pitch_speed(int32_t s, int32_t p) { return (int32_t)((1000 * (int64_t)s + p / 2) / p); }
// the first and the last input of output position c's support (either may lie outside the row): 3 |c - 1000 i| < 80 D
PTTS_HD inline int64_t pitch_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
PTTS_HD inline int64_t pitch_first(int64_t c, int32_t D) { return pitch_floor_div(3 * c - (int64_t)kPitchSupport * D, 3000) + 1; }
PTTS_HD inline int64_t pitch_last(int64_t c, int32_t D) { return pitch_floor_div(3 * c + (int64_t)kPitchSupport * D - 1, 3000); }

// ---- the host side (pitch.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, pitch_permille in its range, reserved 0); otherwise the
// message, naming the field
std::string pitch_opts_error(const ptts_pitch_opts* p);
// The pair (pitch p, speed s) of one row, both in permille (1000: none), resolved to the steps that run -- the one place that states the rule:
// the resample unless p is 1000, the tempo at the effective speed E unless E is 1000
struct PitchSteps { int32_t E; bool resample, tempo; };
// empty: the pair resolves to an effective speed from 500 to 2000 (*st says what runs); otherwise the message, naming both fields and both
// values, and *st holds E alone
std::string pitch_steps(int32_t p, int32_t s, PitchSteps* st);
// empty: a row of n samples keeps its resampled and its final length below kTempoMaxSamples
std::string pitch_length_error(int64_t n, int32_t p, int32_t E);
// the design of well-formed options
PitchScan pitch_design(const ptts_pitch_opts& p);
// the table: h[0, kPitchEntries) and hd[0, kPitchEntries), made once
const float* pitch_table_h();
const float* pitch_table_hd();
// the resampled row into out (holds pitch_resample_length(n, d.p) floats; not x)
void pitch_resample_host(const PitchScan& d, const float* x, int64_t n, float* out);

}  // namespace ptts
