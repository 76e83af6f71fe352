// compressor.cpp -- the host side of a request's dynamic range compressor (include/ptts.h ptts_compressor_opts, ptts_compress_*,
// ptts_dsp_ext_set_compressor): the checks of the caller's options, the design (the only place where libm is asked: exp
// for the two time constants, pow for the knee's lower edge), and ptts_compress_apply: compressor.h's functions in their blocked form -- the
// functions compressor.hip's k_cmp_* kernels call, instantiated for the host -- so a request's compressor and ptts_compress_rows give these
// bits.  No HIP header: the file builds with a plain C++ compiler (tests/test_compressor_cpu.py does, with sanitizers).
#include <cmath>
#include <cstddef>

#include "dsp_ext.h"
#include "opts_check.h"

namespace ptts {

std::string cmp_opts_error(const ptts_compressor_opts* c) {
    if (!c) return "compressor: null options";
    constexpr size_t kKnown = sizeof(ptts_compressor_opts);
    std::string e = opts_size_error("compressor", c, c->size, kKnown, kKnown, "the fields up to makeup_db");
    if (!e.empty()) return e;
    if (c->reserved) return strfmt("compressor: reserved is %d, must be 0", c->reserved);
    const auto bad = [&e](const char* field, double v, double lo, double hi) { return range_error("compressor", field, v, lo, hi, e); };
    if (bad("threshold_db", c->threshold_db, -60.0, 0.0) || bad("ratio", c->ratio, 1.0, 100.0) || bad("knee_db", c->knee_db, 0.0, 24.0) ||
        bad("attack_ms", c->attack_ms, 0.05, 200.0) || bad("release_ms", c->release_ms, 5.0, 5000.0) || bad("makeup_db", c->makeup_db, -24.0, 24.0))
        return e;
    return std::string();
}

CmpScan cmp_design(const ptts_compressor_opts& c) {
#pragma clang fp contract(off)
    CmpScan d{};
    d.rho = std::exp(-1.0 / (c.release_ms * 24.0));
    d.alpha = std::exp(-1.0 / (c.attack_ms * 24.0));
    d.beta = 1.0 - d.alpha;
    scan_powers<1>(&d.rho, &d.rho_run, &d.rho_tile);
    scan_powers<1>(&d.alpha, &d.alpha_run, &d.alpha_tile);
    d.thr_db = c.threshold_db;
    d.knee_db = c.knee_db;
    d.slope = 1.0 / c.ratio - 1.0;
    d.knee_q = c.knee_db > 0.0 ? d.slope / (2.0 * c.knee_db) : 0.0;
    d.makeup_db = c.makeup_db;
    d.s_lo = std::pow(10.0, (c.threshold_db - 0.5 * c.knee_db) / 20.0);
    d.g_lo = cmp_exp2((0.0 + c.makeup_db) * kCmpLog2PerDb);   // the curve's own value where it says 0 dB
    return d;
}

void cmp_apply_blocked(const CmpScan& d, float* x, int64_t n) {
    double Sp = 0.0, Ss = 0.0, tp[kDspLanes], ts[kDspLanes];
    for (int64_t base = 0; base < n; base += kDspTile) {
        const int cnt = (int)std::min<int64_t>(kDspTile, n - base);
        float* tile = x + base;
        cmp_tile_states(d, tile, cnt, Sp, Ss, tp, ts);
        for (int l = 0; l < kDspLanes; l++) cmp_run_y(d, tile + l * kDspRun, scan_run_count(cnt, l), tp[l], ts[l], tile + l * kDspRun);
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_dsp_ext_set_compressor(ptts_dsp_ext* e, const ptts_compressor_opts* c) {
    return ext_set(e, "compressor", c, cmp_opts_error, cmp_design, &DspExt::compress, &DspExt::cmp);
}

int ptts_compress_gain(const ptts_compressor_opts* c, double level_db, double* gain_db) {
    if (!gain_db) return fail("compressor: null argument");
    const std::string err = cmp_opts_error(c);
    if (!err.empty()) return fail(err);
    if (!std::isfinite(level_db)) return fail(strfmt("compressor: level_db %g is not finite", level_db));
    *gain_db = 20.0 * std::log10(cmp_gain(cmp_design(*c), std::pow(10.0, level_db / 20.0)));
    return PTTS_OK;
}

int ptts_compress_apply(const ptts_compressor_opts* c, float* samples, int64_t n) {
    const std::string err = cmp_opts_error(c);
    if (!err.empty()) return fail(err);
    if ((!samples && n > 0) || n < 0) return fail("compressor: null samples");
    cmp_apply_blocked(cmp_design(*c), samples, n);
    return PTTS_OK;
}

}  // extern "C"
