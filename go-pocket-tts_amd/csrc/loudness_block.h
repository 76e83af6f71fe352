// loudness_block.h -- the BS.1770-4 measurement (mono, 24 kHz) in blocked form, written once for the host and the device (loudness.hip's
// kernels; loudness.cpp's loud_measure, which IS ptts_loudness).  DESIGN.md section 8 (N3).
//
// K-weighting is two biquads in cascade (a high shelf, then a high-pass), both direct form II transposed with float64 state: one linear system
//     z' = A z + B x   with the four states z = (shelf z1, shelf z2, high-pass z1, high-pass z2)
// evaluated exactly as dsp_block.h evaluates the DC block: tiles of kDspTile samples on the row's own grid, kDspLanes runs of kDspRun samples,
//     e_l          end state of run l from zero state                              (loud_run, parallel over runs)
//     t_0 = S_f,   t_(l+1) = A^kDspRun t_l + e_l                                   (loud_advance, in run order)
//     E_f = the same fold from t_0 = 0;   S_(f+1) = A^kDspTile S_f + E_f           (in tile order)
//     q_l          the sum of the run's 30 squared outputs, in sample order, the recurrence started from t_l
// Energies: a sub-block is kLoudSub = 480 samples = 16 runs (a tile has 4, the 100 ms hop 5, the 400 ms block 20); its energy is the sum of
// its runs' q in run order; block j (samples [2400 j, 2400 j + 9600), whole blocks only) is the sum of its 20 sub-blocks in order, over 9600.
// Gating is linear: the absolute gate z > abs_gate, the relative gate z > 0.1 * mean of the absolutely gated z, M the mean of the doubly
// gated z, all sums in block order.  No logarithm here: LUFS = -0.691 + 10 log10(M) is the host's.
// Every product and sum is a separate float64 operation (no contraction); the division and the square root are the correctly rounded IEEE
// operations on both sides, so the host and the device instantiation agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "dsp_block.h"

namespace ptts {

constexpr int kLoudSub = 480, kLoudRunsPerSub = kLoudSub / kDspRun, kLoudSubsPerTile = kDspTile / kLoudSub;   // 16 runs, 4 per tile
constexpr int kLoudHopSubs = 5, kLoudBlockSubs = 20;
constexpr int64_t kLoudBlock = (int64_t)kLoudBlockSubs * kLoudSub, kLoudHop = (int64_t)kLoudHopSubs * kLoudSub;   // 9600, 2400
static_assert(kLoudSub % kDspRun == 0 && kDspTile % kLoudSub == 0, "sub-blocks lie on the run grid and tiles on the sub-block grid");

// the two sections, the powers A^kDspRun and A^kDspTile of the cascade's state matrix (row-major 4 x 4) and the absolute gate
// 10^((-70 + 0.691) / 10): made on the host by loud_scan_coeffs and passed by value
struct LoudScan { DspBiquad s1, s2; double a_run[16], a_tile[16]; double abs_gate; };

// `count` samples of the cascade from state z; returns the sum of the squared outputs in sample order
PTTS_HD inline double loud_run(const LoudScan& c, const float* x, int count, double* z) {
#pragma clang fp contract(off)
    double q = 0.0;
    double z1 = z[0], z2 = z[1], z3 = z[2], z4 = z[3];
    for (int i = 0; i < count; i++) {
        const double xi = (double)x[i];
        const double u = c.s1.b0 * xi + z1;
        z1 = c.s1.b1 * xi - c.s1.a1 * u + z2;
        z2 = c.s1.b2 * xi - c.s1.a2 * u;
        const double y = c.s2.b0 * u + z3;
        z3 = c.s2.b1 * u - c.s2.a1 * y + z4;
        z4 = c.s2.b2 * u - c.s2.a2 * y;
        q = q + y * y;
    }
    z[0] = z1; z[1] = z2; z[2] = z3; z[3] = z4;
    return q;
}

// s <- P s + e
PTTS_HD inline void loud_advance(const double* P, double* s, const double* e) {
#pragma clang fp contract(off)
    double n[4];
    for (int i = 0; i < 4; i++) n[i] = P[4 * i + 0] * s[0] + P[4 * i + 1] * s[1] + P[4 * i + 2] * s[2] + P[4 * i + 3] * s[3] + e[i];
    for (int i = 0; i < 4; i++) s[i] = n[i];
}

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
