// trim.cpp -- silence control of one part of a joined text, on the host (include/ptts.h ptts_trim_opts, ptts_trim_plan, ptts_trim_apply;
// trim.h has the rule): the checks of the caller's options, the design (the only place where libm is asked: pow for the threshold) and the
// statement of the result, which the k_trim_* kernels (trim.hip) give bit for bit.  ptts_dsp_ext_set_trim is with the handle (true_peak.cpp).
// No HIP header: the file builds with a plain C++ compiler, alone (tests/test_trim_cpu.py does, with sanitizers).
#include "trim.h"

#include <cmath>
#include <cstddef>
#include <cstring>

#include "opts_check.h"

namespace ptts {

static int64_t ms_samples(double ms) { return (int64_t)(ms / 1000.0 * 24000.0); }   // dsp_fade_in's expression

std::string trim_opts_error(const ptts_trim_opts* t) {
    if (!t) return "trim: null options";
    constexpr size_t kKnown = sizeof(ptts_trim_opts);
    std::string e = opts_size_error("trim", t, t->size, kKnown, kKnown, "the fields up to max_pause_ms");
    if (!e.empty()) return e;
    if (t->edges != 0 && t->edges != 1) return strfmt("trim: edges %d is not 0 or 1", t->edges);
    if (range_error("trim", "threshold_db", t->threshold_db, -120.0, 0.0, e)) return e;
    if (range_error("trim", "pad_ms", t->pad_ms, 0.0, 500.0, e)) return e;
    if (t->max_pause_ms != 0.0 && !(std::isfinite(t->max_pause_ms) && t->max_pause_ms >= 20.0 && t->max_pause_ms <= 5000.0))
        return strfmt("trim: max_pause_ms %g is not 0 (pauses untouched) or a finite value from 20 to 5000", t->max_pause_ms);
    if (t->edges == 0 && t->max_pause_ms == 0.0) return "trim: nothing switched on (edges is 0 and max_pause_ms is 0)";
    return std::string();
}

TrimScan trim_design(const ptts_trim_opts& t) {
    TrimScan d{};
    d.t = (float)std::pow(10.0, t.threshold_db / 20.0);
    d.edges = t.edges;
    d.H = ms_samples(t.pad_ms);
    d.M = ms_samples(t.max_pause_ms);
    return d;
}

namespace {
// One walk over the row's loud samples.  emit(a, b): the samples [a, b) are output next
template <class Emit>
void trim_walk(const TrimScan& d, const float* x, int64_t n, ptts_trim_info* info, Emit&& emit) {
    int64_t first = -1, last = -1;
    for (int64_t i = 0; i < n && first < 0; i++) if (trim_loud(x[i], d.t)) first = i;
    for (int64_t i = n - 1; i >= 0 && last < 0; i--) if (trim_loud(x[i], d.t)) last = i;
    ptts_trim_info r{};
    r.hi = r.n_out = n > 0 ? n : 0;
    if (first < 0) {   // no speech: the row as it is
        emit((int64_t)0, r.hi);
        if (info) *info = r;
        return;
    }
    r.speech = 1;
    r.lo = d.edges ? std::max<int64_t>(0, first - d.H) : 0;
    r.hi = d.edges ? std::min<int64_t>(n, last + 1 + d.H) : n;
    int64_t from = r.lo, removed = 0, u = first;   // [from, ...) is pending; u: the last loud index seen
    for (int64_t v = first + 1; v <= last; v++) {
        if (!trim_loud(x[v], d.t)) continue;
        int64_t a, b;
        trim_cut(u, v, d.M, &a, &b);
        if (b > a) {
            emit(from, a);
            from = b;
            removed += b - a;
            r.cuts++;
        }
        u = v;
    }
    emit(from, r.hi);
    r.n_out = r.hi - r.lo - removed;
    if (info) *info = r;
}
}  // namespace

void trim_plan_host(const TrimScan& d, const float* x, int64_t n, ptts_trim_info* info) {
    trim_walk(d, x, n, info, [](int64_t, int64_t) {});
}

void trim_apply_host(const TrimScan& d, const float* x, int64_t n, float* out, ptts_trim_info* info) {
    int64_t at = 0;   // (at <= a for every piece: out may be x)
    trim_walk(d, x, n, info, [&](int64_t a, int64_t b) {
        if (b > a) std::memmove(out + at, x + a, (size_t)(b - a) * sizeof(float));   // bit for bit
        at += b > a ? b - a : 0;
    });
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_trim_plan(const ptts_trim_opts* t, const float* x, int64_t n, ptts_trim_info* info) {
    const std::string err = trim_opts_error(t);
    if (!err.empty()) return fail(err);
    if (n < 0 || n >= kTrimMaxSamples) return fail(strfmt("trim: n %lld is not from 0 to below 2^31", (long long)n));
    if ((!x && n > 0) || !info) return fail("trim: null argument");
    trim_plan_host(trim_design(*t), x, n, info);
    return PTTS_OK;
}

int ptts_trim_apply(const ptts_trim_opts* t, const float* in, int64_t n, float* out, ptts_trim_info* info) {
    const std::string err = trim_opts_error(t);
    if (!err.empty()) return fail(err);
    if (n < 0 || n >= kTrimMaxSamples) return fail(strfmt("trim: n %lld is not from 0 to below 2^31", (long long)n));
    if ((!in || !out) && n > 0) return fail("trim: null argument");
    trim_apply_host(trim_design(*t), in, n, out, info);
    return PTTS_OK;
}

}  // extern "C"
