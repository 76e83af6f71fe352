// deesser.cpp -- the host side of a request's de-esser (include/ptts.h ptts_deesser_opts, ptts_deess_apply, ptts_deess_band,
// ptts_dsp_ext_set_deesser): the checks of the caller's options, the design (eq.cpp's for the side chain's section,
// compressor.cpp's for the detector: no formula of its own), and ptts_deess_apply: deesser.h's, compressor.h's and scan_block.h's functions in
// their blocked form -- the functions deesser.hip's k_de_* kernels call, instantiated for the host -- so a request's de-esser and
// ptts_deess_rows give these bits.  No HIP header: the file builds with a plain C++ compiler, beside eq.cpp and compressor.cpp
// (tests/test_deesser_cpu.py does, with sanitizers).
#include <cmath>
#include <cstddef>
#include <cstring>

#include "dsp_ext.h"
#include "opts_check.h"

namespace ptts {

std::string de_opts_error(const ptts_deesser_opts* o) {
    if (!o) return "deesser: null options";
    constexpr size_t kKnown = sizeof(ptts_deesser_opts);
    std::string e = opts_size_error("deesser", o, o->size, kKnown, kKnown, "the fields up to max_reduction_db");
    if (!e.empty()) return e;
    if (o->reserved) return strfmt("deesser: reserved is %d, must be 0", o->reserved);
    const auto bad = [&e](const char* field, double v, double lo, double hi) { return range_error("deesser", field, v, lo, hi, e); };
    if (bad("freq_hz", o->freq_hz, 2000.0, 10000.0) || bad("q", o->q, 0.3, 4.0) || bad("threshold_db", o->threshold_db, -60.0, 0.0) ||
        bad("ratio", o->ratio, 1.0, 100.0) || bad("knee_db", o->knee_db, 0.0, 24.0) || bad("attack_ms", o->attack_ms, 0.05, 200.0) ||
        bad("release_ms", o->release_ms, 5.0, 5000.0) || bad("max_reduction_db", o->max_reduction_db, 0.0, 40.0))
        return e;
    return std::string();
}

DeScan de_design(const ptts_deesser_opts& o) {
    DeScan d{};
    const ptts_eq_section hp = {PTTS_EQ_HIGHPASS, 0, o.freq_hz, 0.0, o.q};
    d.c = eq_design(hp);
    const EqScan one = eq_scan_coeffs(&d.c, 1);   // (N = 2: the 2 x 2 powers lie packed at the front)
    for (int i = 0; i < 4; i++) { d.a_run[i] = one.a_run[i]; d.a_tile[i] = one.a_tile[i]; }
    ptts_compressor_opts c{};
    c.size = sizeof c;
    c.threshold_db = o.threshold_db; c.ratio = o.ratio; c.knee_db = o.knee_db; c.attack_ms = o.attack_ms; c.release_ms = o.release_ms; c.makeup_db = 0.0;
    d.det = cmp_design(c);
    d.floor_db = 0.0 - o.max_reduction_db;
    return d;
}

void de_band_blocked(const DeScan& d, const float* x, int64_t n, float* band) {
    if (n <= 0) return;
    if (band != x) std::memmove(band, x, (size_t)n * sizeof(float));
    const EqSys<1> sys = de_band(d);
    scan_walk(sys, band, n, [&](int64_t i0, int count, double* z) { sys.run(band + i0, count, z, band + i0); });   // eq_apply_blocked, one section
}

void de_apply_blocked(const DeScan& d, float* x, int64_t n) {
    const EqSys<1> sys = de_band(d);
    const CmpScan& c = d.det;
    double Sb[2] = {0.0, 0.0}, Sp = 0.0, Ss = 0.0, tp[kDspLanes], ts[kDspLanes];
    float band[kDspTile];
    for (int64_t base = 0; base < n; base += kDspTile) {
        const int cnt = (int)std::min<int64_t>(kDspTile, n - base);
        float* tile = x + base;
        scan_tile(sys, tile, cnt, Sb, [&](int off, int count, double* z) { sys.run(tile + off, count, z, band + off); });   // the band of the tile
        cmp_tile_states(c, band, cnt, Sp, Ss, tp, ts);                                                                      // the detector on it
        for (int l = 0; l < kDspLanes; l++) de_run_y(d, tile + l * kDspRun, band + l * kDspRun, scan_run_count(cnt, l), tp[l], ts[l]);
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_dsp_ext_set_deesser(ptts_dsp_ext* e, const ptts_deesser_opts* d) {
    return ext_set(e, "deesser", d, de_opts_error, de_design, &DspExt::deess, &DspExt::des);
}

int ptts_deess_apply(const ptts_deesser_opts* d, float* samples, int64_t n) {
    const std::string err = de_opts_error(d);
    if (!err.empty()) return fail(err);
    if ((!samples && n > 0) || n < 0) return fail("deesser: null samples");
    de_apply_blocked(de_design(*d), samples, n);
    return PTTS_OK;
}

int ptts_deess_band(const ptts_deesser_opts* d, const float* in, int64_t n, float* band) {
    const std::string err = de_opts_error(d);
    if (!err.empty()) return fail(err);
    if (((!in || !band) && n > 0) || n < 0) return fail("deesser: null samples");
    de_band_blocked(de_design(*d), in, n, band);
    return PTTS_OK;
}

}  // extern "C"
