// true_peak.h -- the true-peak meter of a request's ceiling (include/ptts.h ptts_true_peak; the handle that carries it: dsp_ext.h), written once
// for the host (true_peak.cpp) and the device (true_peak.hip).  No HIP header: true_peak.cpp builds with a plain C++ compiler.
//
// The meter oversamples the 24 kHz row eight times, to the 192 kHz of ITU-R BS.1770-4 Annex 2, with the project's own polyphase design
// (rate_taps.h) for the pair 24000 -> 192000: L = 8 phases of K = 54 taps, cutoff 0.45 cycles per input sample, Kaiser beta 8.6, tap k of a
// phase on input i + dlo + k with dlo = -26, float64 rounded once to f32.  Output y[8 i + p], for i in [0, n) and p in [0, 8), is ONE f32 fmaf
// chain from 0.0f over ascending k of x[i + dlo + k] * h[p][k]; samples outside [0, n) read as zero; nothing before sample 0 or at or beyond
// sample n is an output.  TP = max(max |x[i]|, max |y[j]|) as an f32.  A NaN candidate never wins (a > pk is false), as in k_dsp_peak; TP is
// never below the sample peak.  A max has no order and fmaf rounds once, so host and device give the same bits whatever the schedule.
// KNOWN LIMIT: content above about 10 kHz lies in the filter's transition band (the passband ends at 0.45 x 24 kHz = 10.8 kHz) and is
// under-read: a 10 kHz tone reads 0.16 dB low.  Speech from this decoder has little energy there.
#pragma once
#include <cmath>
#include <string>

#include "scan_block.h"

namespace ptts {

constexpr int kTpPhases = 8, kTpTaps = 54, kTpDlo = -26;
constexpr int kTpBefore = -kTpDlo, kTpAfter = kTpTaps - 1 + kTpDlo;   // samples a window reaches in front of and behind its own: 26, 27

// h[k][p]: tap k of phase p.  The eight taps of one k lie together: one scalar load on the device, one vector on the host.  1728 bytes: the
// struct travels by value in k_tp_peak's arguments
struct TpTaps { float h[kTpTaps][kTpPhases]; };
static_assert(sizeof(TpTaps) == 1728, "k_tp_peak takes the taps by value");

// The meter, for J samples side by side.  acc[j][p] is the chain of y[8 i_j + p]: tp_step is its step k, for every phase at once -- h8 is h[k],
// xv[j] is x[i_j + dlo + k], zero outside the row -- and is called for k = 0 .. kTpTaps - 1 in ascending order on chains that start at 0.0f;
// tp_fold then takes the maximum.  The J * 8 chains are independent and share each tap, and a sample's eight share its window word.
template <int J>
PTTS_HD __attribute__((always_inline)) inline void tp_step(float (&acc)[J][kTpPhases], const float (&xv)[J], const float (&h8)[kTpPhases]) {
#pragma unroll
    for (int j = 0; j < J; j++) {
#pragma unroll
        for (int p = 0; p < kTpPhases; p++) acc[j][p] = fmaf(xv[j], h8[p], acc[j][p]);
    }
}
template <int J>
PTTS_HD __attribute__((always_inline)) inline float tp_fold(const float (&acc)[J][kTpPhases], float pk) {
#pragma unroll
    for (int j = 0; j < J; j++) {
#pragma unroll
        for (int p = 0; p < kTpPhases; p++) { const float a = fabsf(acc[j][p]); if (a > pk) pk = a; }
    }
    return pk;
}

// the f32 taps, designed once (rate_taps.h)
const TpTaps& tp_taps();
// TP of x[0, n) on the host; y (optional, 8 n floats) receives the oversampled signal
float tp_measure(const float* x, int64_t n, float* y = nullptr);
// empty: the ceiling is a finite value from -60 to 0 dBTP
std::string tp_ceiling_error(double ceiling_dbtp);
// c = (float)pow(10, dBTP / 20)
inline float tp_ceiling(double ceiling_dbtp) { return (float)std::pow(10.0, ceiling_dbtp / 20.0); }

}  // namespace ptts
