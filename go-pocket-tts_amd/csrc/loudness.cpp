// loudness.cpp -- integrated loudness after ITU-R BS.1770-4 (mono, the decoder's 24 kHz) and the gain to a target, on the host: ptts_loudness
// and ptts_loudness_normalize.  The host function is the blocked evaluation of scan_block.h itself -- the functions dsp.hip's k_loud_* kernels
// call, instantiated for the host, in the order the kernels run them -- so a request's `loudness`, ptts_loudness_rows and
// ptts_loudness_normalize_rows give these bits.  DESIGN.md section 8 (N3).
#include <cmath>

#include "scan_block.h"
#include "runtime.h"

namespace ptts {

namespace {
// BS.1770's two K-weighting stages re-derived for the sample rate (the standard tabulates them at 48 kHz only): the bilinear forms whose
// parameters reproduce that table
DspBiquad k_shelf(double fs) {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(M_PI * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    return DspBiquad{(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0};
}
DspBiquad k_highpass(double fs) {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(M_PI * f0 / fs);
    const double a0 = 1.0 + K / Q + K * K;
    return DspBiquad{1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0};
}
}  // namespace

void loud_kweight_coeffs(int sample_rate, double out[10]) {
    const DspBiquad s = k_shelf((double)sample_rate), h = k_highpass((double)sample_rate);
    const double v[10] = {s.b0, s.b1, s.b2, s.a1, s.a2, h.b0, h.b1, h.b2, h.a1, h.a2};
    for (int i = 0; i < 10; i++) out[i] = v[i];
}

// the cascade's state matrix over (shelf z1, shelf z2, high-pass z1, high-pass z2) -- with x = 0: u = z1, y = c0 u + z3 -- and its powers
// A^kDspRun, A^kDspTile
LoudScan loud_scan_coeffs(int sample_rate) {
    LoudScan sc;
    sc.s1 = k_shelf((double)sample_rate);
    sc.s2 = k_highpass((double)sample_rate);
    const DspBiquad &a = sc.s1, &b = sc.s2;
    const double A[16] = {-a.a1, 1.0, 0.0, 0.0,
                          -a.a2, 0.0, 0.0, 0.0,
                          b.b1 - b.a1 * b.b0, 0.0, -b.a1, 1.0,
                          b.b2 - b.a2 * b.b0, 0.0, -b.a2, 0.0};
    scan_powers<4>(A, sc.a_run, sc.a_tile);
    sc.abs_gate = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    return sc;
}

const LoudScan& loud_scan() {
    static const LoudScan sc = loud_scan_coeffs(kNativeRate);
    return sc;
}

double loud_target_power(double target_lufs) { return std::pow(10.0, (target_lufs + 0.691) / 10.0); }
double loud_lufs(double M) { return M > 0.0 ? -0.691 + 10.0 * std::log10(M) : (std::isnan(M) ? M : -INFINITY); }

std::string loud_target_error(double target_lufs) {
    if (!(target_lufs >= -70.0 && target_lufs <= -1.0)) return strfmt("loudness: target %g LUFS is outside -70 .. -1", target_lufs);
    return std::string();
}

// what k_loud_summary, k_loud_carry and k_loud_energy compute for one row: 4 sub-block energies per tile
void loud_sub_energies(const float* x, int64_t n, std::vector<double>& sub) {
    const LoudScan& sc = loud_scan();
    std::vector<double> q((size_t)scan_tiles(n) * kDspLanes, 0.0);   // every run's sum of squares
    scan_walk(sc, x, n, [&](int64_t i0, int count, double* z) { q[(size_t)(i0 / kDspRun)] = sc.run(x + i0, count, z); });
    sub.resize(q.size() / kLoudRunsPerSub);
    for (size_t k = 0; k < sub.size(); k++) sub[k] = loud_sub_energy(q.data() + k * kLoudRunsPerSub);
}

// what k_loud_gate computes: the doubly gated mean square of the row's whole 400 ms blocks; 0: no block above the gates
double loud_gated_mean(const double* sub, int64_t n) {
    const LoudScan& sc = loud_scan();
    const int64_t nb = loud_blocks(n);
    LoudAcc first{0.0, 0}, second{0.0, 0};
    for (int64_t j = 0; j < nb; j++) loud_gate_add(first, loud_block_energy(sub, j), sc.abs_gate, sc.abs_gate);
    if (!first.cnt) return 0.0;
    const double rel = loud_rel_gate(first);
    for (int64_t j = 0; j < nb; j++) loud_gate_add(second, loud_block_energy(sub, j), sc.abs_gate, rel);
    return second.cnt ? loud_div(second.sum, (double)second.cnt) : 0.0;
}

double loud_measure(const float* x, int64_t n) {
    std::vector<double> sub;
    loud_sub_energies(x, n, sub);
    return loud_gated_mean(sub.data(), n);
}

float loud_measure_gain(const float* x, int64_t n, double target_power, double* M_out) {
    const double M = loud_measure(x, n);
    if (M_out) *M_out = M;
    float peak = 0.0f;   // dsp_peak_normalize's: NaNs never win
    for (int64_t i = 0; i < n; i++) {
        const float a = (float)std::fabs((double)x[i]);
        if (a > peak) peak = a;
    }
    return loud_gain(M, target_power, peak);
}

double loud_normalize(float* x, int64_t n, double target_lufs) {
    double M = 0.0;
    const float g = loud_measure_gain(x, n, loud_target_power(target_lufs), &M);
    if (g != 1.0f)
        for (int64_t i = 0; i < n; i++) x[i] = x[i] * g;
    return M;
}

}  // namespace ptts
