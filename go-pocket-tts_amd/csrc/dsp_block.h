// dsp_block.h -- the DC block's recurrence in blocked form, written once for the host and the device (dsp.hip's kernels, dsp.cpp's
// dsp_dc_block_blocked, which a CPU test drives through libptts_hooks.so).  DESIGN.md section 8 (N3).
//
// The biquad of dsp_dc_block (direct form II transposed, float64 state) is the linear system
//     y = b0 x + z1,   z' = A z + B x,   A = [[-a1, 1], [-a2, 0]]
// so a run of samples started from state z gives what the same run gives from state 0 plus the free response of z, and the state behind
// the run is A^len z + e with e the end state of the zero-state run.  A row is cut on a grid that depends on nothing but the sample index:
// tiles of kDspTile samples (one decoder frame), each of kDspLanes runs of kDspRun samples.
//     e_l          end state of run l from zero state                              (dsp_run, parallel over runs)
//     t_0 = S_f,   t_(l+1) = A^kDspRun t_l + e_l                                   (dsp_advance, in run order)
//     E_f = the same fold from t_0 = 0;   S_(f+1) = A^kDspTile S_f + E_f           (in tile order)
//     y of run l   the recurrence itself, started from t_l                         (dsp_run again)
// Every product and sum below is a separate float64 operation (no contraction), so the host and the device instantiation agree bit for bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTTS_HD __host__ __device__
#else
#define PTTS_HD
#endif

namespace ptts {

constexpr int kDspRun = 30, kDspLanes = 64, kDspTile = kDspRun * kDspLanes;   // 1920 = samples per frame at 24 kHz

struct DspBiquad { double b0, b1, b2, a1, a2; };
// the section and the two powers of A the blocked form needs (row-major 2 x 2), made on the host by dsp_scan_coeffs and passed by value
struct DspScan { DspBiquad c; double a_run[4], a_tile[4]; };

// `count` samples of the section from state (z1, z2): x its f32 inputs, y (optional, may be x) receives the outputs rounded to f32
PTTS_HD inline void dsp_run(const DspBiquad& c, const float* x, float* y, int count, double& z1, double& z2) {
#pragma clang fp contract(off)
    for (int i = 0; i < count; i++) {
        const double xi = (double)x[i];
        const double yi = c.b0 * xi + z1;
        z1 = c.b1 * xi - c.a1 * yi + z2;
        z2 = c.b2 * xi - c.a2 * yi;
        if (y) y[i] = (float)yi;
    }
}

// s <- P s + e
PTTS_HD inline void dsp_advance(const double* P, double& s1, double& s2, double e1, double e2) {
#pragma clang fp contract(off)
    const double n1 = P[0] * s1 + P[1] * s2 + e1;
    const double n2 = P[2] * s1 + P[3] * s2 + e2;
    s1 = n1; s2 = n2;
}

}  // namespace ptts
