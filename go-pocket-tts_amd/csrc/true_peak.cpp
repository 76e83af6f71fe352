// true_peak.cpp -- the host side of a request's true-peak ceiling (include/ptts.h ptts_true_peak*, ptts_dsp_ext_*): the
// meter's taps, the meter itself over a host row -- true_peak.h's tp_step and tp_fold, the functions k_tp_peak runs -- the static gain, and the
// handle of ptts_dsp_opts.ext, which lives in eq.cpp's registry of live handles.  No HIP header: the file builds with a plain C++ compiler.
#include <cstring>
#include <new>

#include "dsp_ext.h"
#include "opts_check.h"
#include "rate_taps.h"
#include "true_peak.h"

#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__)) && !defined(__HIP_DEVICE_COMPILE__)
#define PTTS_TP_FMA 1
#endif

namespace ptts {

namespace {
// TP of the row; one body, compiled twice on x86-64: fmaf as the fused instruction where the processor has it, the C library's fmaf (the
// same correctly rounded result) where it has not
__attribute__((always_inline)) inline float measure(const float* x, int64_t n, const TpTaps& t, float* y) {
    float pk = 0.0f;
    for (int64_t i = 0; i < n; i++) {
        const float a = fabsf(x[i]);
        if (a > pk) pk = a;
        const float* w;
        float edge[kTpTaps];
        if (i + kTpDlo >= 0 && i + kTpAfter < n) w = x + i + kTpDlo;
        else {   // the window leaves the row: zeros outside [0, n)
            for (int k = 0; k < kTpTaps; k++) {
                const int64_t at = i + kTpDlo + k;
                edge[k] = at >= 0 && at < n ? x[at] : 0.0f;
            }
            w = edge;
        }
        float acc[1][kTpPhases] = {};
        for (int k = 0; k < kTpTaps; k++) {
            const float xv[1] = {w[k]};
            tp_step<1>(acc, xv, t.h[k]);
        }
        if (y) for (int p = 0; p < kTpPhases; p++) y[i * kTpPhases + p] = acc[0][p];
        pk = tp_fold<1>(acc, pk);
    }
    return pk;
}

float measure_plain(const float* x, int64_t n, const TpTaps& t, float* y) { return measure(x, n, t, y); }
#ifdef PTTS_TP_FMA
__attribute__((target("fma"))) float measure_fma(const float* x, int64_t n, const TpTaps& t, float* y) { return measure(x, n, t, y); }
#endif
}  // namespace

const TpTaps& tp_taps() {
    static const TpTaps taps = [] {
        TpTaps t;
        std::memset(&t, 0, sizeof t);
        const RateShape sh = rate_shape(24000, 24000 * kTpPhases);
        float by_phase[kTpPhases][kTpTaps] = {};   // rate_taps' order
        if (sh.L == kTpPhases && sh.M == 1 && sh.K == kTpTaps && sh.dlo == kTpDlo) rate_taps(sh, &by_phase[0][0]);   // (else: all zero, and the tests say so)
        for (int p = 0; p < kTpPhases; p++)
            for (int k = 0; k < kTpTaps; k++) t.h[k][p] = by_phase[p][k];
        return t;
    }();
    return taps;
}

float tp_measure(const float* x, int64_t n, float* y) {
#ifdef PTTS_TP_FMA
    static const bool has_fma = __builtin_cpu_supports("fma");
    if (has_fma) return measure_fma(x, n, tp_taps(), y);
#endif
    return measure_plain(x, n, tp_taps(), y);
}

std::string tp_ceiling_error(double c) {
    if (std::isfinite(c) && c >= -60.0 && c <= 0.0) return std::string();
    return strfmt("true peak: ceiling_dbtp %g is not a finite value from -60 to 0", c);
}

bool ext_lookup(const ptts_dsp_ext* e, DspExt* out) {
    return handle_with(e, HANDLE_DSP_EXT, [&] { *out = e->v; });
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_dsp_ext_create(const ptts_dsp_ext_opts* o, ptts_dsp_ext** out) {
    if (!o || !out) return fail("dsp ext: null argument");
    *out = nullptr;
    constexpr size_t kKnown = sizeof(ptts_dsp_ext_opts), kLeast = offsetof(ptts_dsp_ext_opts, ceiling_dbtp) + sizeof(double);
    std::string e = opts_size_error("dsp ext", o, o->size, kLeast, kKnown, "true_peak and ceiling_dbtp");
    if (!e.empty()) return fail(e);
    if (o->true_peak != 0 && o->true_peak != 1) return fail(strfmt("dsp ext: true_peak %d is not 0 or 1", o->true_peak));
    e = tp_ceiling_error(o->ceiling_dbtp);
    if (!e.empty()) return fail("dsp ext: " + e);
    ptts_dsp_ext* h = new (std::nothrow) ptts_dsp_ext{};
    if (!h) { set_last_error("ptts-hip: out of host memory"); return PTTS_ENOMEM; }
    h->v.true_peak = o->true_peak == 1;
    h->v.ceiling = tp_ceiling(o->ceiling_dbtp);
    handle_add(h, HANDLE_DSP_EXT);
    *out = h;
    return PTTS_OK;
}

void ptts_dsp_ext_free(ptts_dsp_ext* e) {
    if (!e || !handle_take(e, HANDLE_DSP_EXT)) return;   // not a live handle: nothing of ours to free
    delete e;
}

int ptts_true_peak(const float* samples, int64_t n, float* peak) {
    if (!peak || (!samples && n > 0) || n < 0) return fail("true peak: null argument");
    *peak = tp_measure(samples, n);
    return PTTS_OK;
}

int ptts_true_peak_limit(float* samples, int64_t n, double ceiling_dbtp, float* peak_before) {
    if ((!samples && n > 0) || n < 0) return fail("true peak: null argument");
    const std::string e = tp_ceiling_error(ceiling_dbtp);
    if (!e.empty()) return fail(e);
    const float tp = tp_measure(samples, n), c = tp_ceiling(ceiling_dbtp);
    if (peak_before) *peak_before = tp;
    if (tp > c) {
        const float g = c / tp;
        for (int64_t i = 0; i < n; i++) samples[i] = samples[i] * g;
    }
    return PTTS_OK;
}

}  // extern "C"
