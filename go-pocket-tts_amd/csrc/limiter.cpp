// limiter.cpp -- the host side of a request's look-ahead peak limiter (include/ptts.h ptts_limiter_opts, ptts_limit_apply,
// ptts_dsp_ext_set_limiter): the checks of the caller's options, the design (the only place where libm is asked: pow
// for the ceiling and the drive, exp for the release, lrint for the look-ahead), and ptts_limit_apply: limiter.h's functions in their blocked
// form -- the functions limiter.hip's k_lim_* kernels call, instantiated for the host -- so a request's limiter and ptts_limit_rows give these
// bits.  No HIP header: the file builds with a plain C++ compiler (tests/test_limiter_cpu.py does, with sanitizers).
#include <cmath>
#include <cstddef>
#include <vector>

#include "dsp_ext.h"
#include "opts_check.h"

namespace ptts {

std::string lim_opts_error(const ptts_limiter_opts* l) {
    if (!l) return "limiter: null options";
    constexpr size_t kKnown = sizeof(ptts_limiter_opts);
    std::string e = opts_size_error("limiter", l, l->size, kKnown, kKnown, "the fields up to drive_db");
    if (!e.empty()) return e;
    if (l->reserved) return strfmt("limiter: reserved is %d, must be 0", l->reserved);
    const auto bad = [&e](const char* field, double v, double lo, double hi) { return range_error("limiter", field, v, lo, hi, e); };
    if (bad("ceiling_db", l->ceiling_db, -60.0, 0.0) || bad("lookahead_ms", l->lookahead_ms, 0.25, 5.0) || bad("release_ms", l->release_ms, 5.0, 5000.0) ||
        bad("drive_db", l->drive_db, 0.0, 24.0))
        return e;
    return std::string();
}

LimScan lim_design(const ptts_limiter_opts& l) {
#pragma clang fp contract(off)
    LimScan d{};
    d.c = std::pow(10.0, l.ceiling_db / 20.0);
    d.d = std::pow(10.0, l.drive_db / 20.0);
    d.L = (int32_t)std::lrint(l.lookahead_ms * 24.0);
    d.rho = std::exp(-1.0 / (l.release_ms * 24.0));
    scan_powers<1>(&d.rho, &d.rho_run, &d.rho_tile);
    d.inv = 1.0 / (double)(d.L + 1);
    return d;
}

void lim_apply_blocked(const LimScan& d, float* x, int64_t n) {
    if (n <= 0) return;
    const int L = d.L;
    // the magnitudes, zero behind the row as far as the last run's windows reach; r with r[0] in the L places in front of it
    std::vector<float> ax((size_t)n + (size_t)kDspRun + (size_t)L, 0.0f), rr((size_t)n + (size_t)L);
    for (int64_t i = 0; i < n; i++) ax[(size_t)i] = lim_mag(x[i]);
    float* r = rr.data() + L;
    std::vector<float> hold((size_t)kDspTile);
    double S = 0.0;
    for (int64_t base = 0; base < n; base += kDspTile) {
        const int cnt = (int)std::min<int64_t>(kDspTile, n - base);
        const auto count = [cnt](int l) { return std::max(0, std::min(kDspRun, cnt - l * kDspRun)); };
        float (*m)[kDspRun] = reinterpret_cast<float (*)[kDspRun]>(hold.data());
        double tp[kDspLanes];
        double t = S, E = 0.0;
        for (int l = 0; l < kDspLanes; l++) {
            if (count(l)) lim_hold(ax.data() + base + l * kDspRun, L, m[l]);
            const double e = lim_run_p(d, m[l], count(l), 0.0);
            tp[l] = t;
            t = cmp_fold_p(d.rho_run, t, e);
            E = cmp_fold_p(d.rho_run, E, e);
        }
        for (int l = 0; l < kDspLanes; l++) lim_run_r(d, m[l], count(l), tp[l], r + base + l * kDspRun);
        S = cmp_fold_p(d.rho_tile, S, E);
    }
    for (int k = 1; k <= L; k++) r[-k] = r[0];
    for (int64_t i = 0; i < n; i++) x[i] = lim_out(d, x[i], lim_box(d, r + i));
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_dsp_ext_set_limiter(ptts_dsp_ext* e, const ptts_limiter_opts* l) {
    return ext_set(e, "limiter", l, lim_opts_error, lim_design, &DspExt::limit, &DspExt::lim);
}

int ptts_limit_apply(const ptts_limiter_opts* l, float* samples, int64_t n) {
    const std::string err = lim_opts_error(l);
    if (!err.empty()) return fail(err);
    if ((!samples && n > 0) || n < 0) return fail("limiter: null samples");
    lim_apply_blocked(lim_design(*l), samples, n);
    return PTTS_OK;
}

}  // extern "C"
