// deesser.h -- a request's de-esser (include/ptts.h ptts_deesser_opts, ptts_deess_*), written once for the host
// (deesser.cpp) and the device (deesser.hip).  No HIP header: deesser.cpp builds with a plain C++ compiler.
//
// The compressor's detector on a side chain: a high-passed copy of the 24 kHz row, whose gain is applied to that band alone.  Float64 throughout.
// Per sample, from zero state:
//     b = (float) HP(x)                         one PTTS_EQ_HIGHPASS section at (freq_hz, q), as eq.cpp designs it (eq_design), rounded to f32 where
//                                               ptts_eq_apply rounds its output: b IS ptts_eq_apply of that one section on x
//     a = |b|                                   (as a double)
//     p = (a > rho p) ? a : rho p               compressor.h's detector (cmp_step_p): a NaN never wins
//     s = alpha s + (1 - alpha) p               compressor.h's attack smoothing (cmp_step_s)
//     G = max(curve(20 log10 s), -max_reduction_db)     compressor.h's soft-knee curve in dB (cmp_curve_db; 0 at or under the knee's lower edge,
//                                               where neither log2 nor exp2 is evaluated), makeup 0, held at the floor
//     y = x                                     where G == 0: the sample's 32 bits, untouched
//     y = (float)((double)x + (g - 1.0) (double)b),  g = cmp_exp2(G log2(10) / 20)      elsewhere: one product, one sum, one rounding
// Only the band is turned down, by at most max_reduction_db; where the band's level stays under the knee the row comes back bit for bit.
//
// All three recurrences are evaluated in blocked form on the grid of scan_block.h (runs of kDspRun samples, tiles of kDspTile), and the blocked
// form IS the definition (de_apply_blocked is ptts_deess_apply).  They depend on one another, so the scan has three levels:
//   b   is the equaliser's linear scan with N = 2 (EqSys<1> on this design's section and its powers; scan_advance<2>): the bits of eq_apply_blocked.
//   p   is compressor.h's (max, times) scan (cmp_run_p, cmp_fold_p) over the band of the tile, which is made again from the section's entering
//       states wherever it is needed and never stored beside the row.
//   s   is compressor.h's linear scan with N = 1 (cmp_run_s, scan_advance<1>), its runs recomputing p from their entering state.
// The functions that walk samples are compressor.h's and scan_block.h's own; this header adds the gain's floor and the output (de_run_y).
// Non-finite samples are not treated specially.  A NaN sample poisons what the section's state carries: b is NaN from that sample to the end of
// the row (through the runs' and the tiles' entering states too).  A NaN level never wins, so the detector decays from where it stood; y is NaN
// wherever G != 0 behind the sample, and x bit for bit wherever G == 0 (at once if the level was under the knee, else once it has fallen there).
// An infinite sample does too: b is infinite at the sample and not finite behind it (inf - inf), p and with it s are +inf for the rest of
// the row (rho * inf = inf), cmp_log2 reads that as 2^1024, and G stands at the floor: every sample from there on comes out non-finite.  With
// ratio 1 or max_reduction_db 0, G is 0 everywhere and the row comes back bit for bit whatever it holds.  Samples in front are untouched.
// Host and device agree on which samples come out as NaN and on every other sample's bits; which NaN it is (its sign and payload, made by
// inf - inf or carried through a sum) is the processor's choice and is not part of the statement.
#pragma once
#include <string>

#include "compressor.h"

struct ptts_deesser_opts;

namespace ptts {

// A designed de-esser (deesser.cpp de_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct DeScan {
    DspBiquad c;                   // the side chain's high-pass (eq.cpp eq_design)
    double a_run[4], a_tile[4];    // its state matrix to the powers kDspRun and kDspTile, 2 x 2 row-major (eq.cpp eq_scan_coeffs of that one section)
    CmpScan det;                   // the detector, the smoothing and the curve: cmp_design of the same fields with makeup 0
    double floor_db;               // 0 - max_reduction_db
    double pad[2];
};

// the side chain as the equaliser's system of one section
PTTS_HD inline EqSys<1> de_band(const DeScan& d) { return EqSys<1>(&d.c, d.a_run, d.a_tile); }

// G at level s (s >= 0 or +inf, never a NaN)
PTTS_HD inline double de_gain_db(const DeScan& d, double s) {
    if (!(s > d.det.s_lo)) return 0.0;
    const double g_db = cmp_curve_db(d.det, s);
    return (g_db > d.floor_db) ? g_db : d.floor_db;
}

// the run itself from its entering states, in place: b[0, count) is the run's band
PTTS_HD inline void de_run_y(const DeScan& d, float* x, const float* b, int count, double p, double s) {
#pragma clang fp contract(off)
    for (int i = 0; i < count; i++) {
        const double bi = (double)b[i];
        p = cmp_step_p(d.det, __builtin_fabs(bi), p);
        s = cmp_step_s(d.det, p, s);
        const double G = de_gain_db(d, s);
        if (G == 0.0) continue;
        const double g = cmp_exp2(G * kCmpLog2PerDb);
        x[i] = (float)((double)x[i] + (g - 1.0) * bi);
    }
}

// A row's per-tile states in scratch: [F][4] doubles for the section (E_f then S_f, two each; scan_E<2>, scan_S<2>), then [F][2] for each of the
// detector's two recurrences, as the compressor's
PTTS_HD inline size_t de_state_doubles(int64_t F) { return scan_state_doubles<2>(F) + 2 * scan_state_doubles<1>(F); }

// ---- the host side (deesser.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, every field in its range); otherwise the message, naming the field
std::string de_opts_error(const ptts_deesser_opts* o);
// the design of well-formed options
DeScan de_design(const ptts_deesser_opts& o);
// the band of x[0, n) into band[0, n) (band may be x): eq_apply_blocked of the design's one section
void de_band_blocked(const DeScan& d, const float* x, int64_t n, float* band);
// the de-esser over x[0, n) in place, in blocked form: what the k_de_* kernels compute for one row
void de_apply_blocked(const DeScan& d, float* x, int64_t n);

}  // namespace ptts
