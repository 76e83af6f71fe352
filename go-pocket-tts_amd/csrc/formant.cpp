// formant.cpp -- "keep the formants" around the pitch of one part of a joined text, on the host (include/ptts.h ptts_formant_opts, ptts_formant_frames,
// ptts_formant_analyse, ptts_formant_whiten, ptts_formant_shape, ptts_formant_apply; formant.h has the rule): the checks of the caller's options, the
// three tables and the statement of the result, which k_formant_analyse, k_formant_whiten and k_formant_shape (formant.hip) give bit for bit around
// the pitch's own resample (pitch.cpp) and in front of the tempo (tempo.cpp).  ptts_dsp_ext_set_formant and ptts_formant_rows are in capi_rows.cpp.
// No HIP header: the file builds with a plain C++ compiler, with pitch.cpp and tempo.cpp alone (tests/test_formant_cpu.py does, with sanitizers).
//
// The chains are formant.h's, shared with the device; nothing here may be contracted.
#include "formant.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "opts_check.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ptts {

std::string formant_opts_error(const ptts_formant_opts* f) {
    if (!f) return "formant: null options";
    constexpr size_t kKnown = sizeof(ptts_formant_opts);
    std::string e = opts_size_error("formant", f, f->size, kKnown, kKnown, "the fields up to reserved");
    if (!e.empty()) return e;
    if (f->keep != 0 && f->keep != 1) return strfmt("formant: keep %d is not 0 (formants move with the pitch) or 1 (they stay)", f->keep);
    if (f->reserved[0] != 0 || f->reserved[1] != 0) return "formant: reserved is not 0";
    return std::string();
}

std::string formant_pitch_error(int32_t p) {
    if (p >= kFormantMinPitch && p <= kFormantMaxPitch) return std::string();
    return strfmt("formant: keep 1 with pitch_permille %d: the option is served for a pitch from %d to %d", p, kFormantMinPitch, kFormantMaxPitch);
}

FormantScan formant_design(const ptts_formant_opts& f) {
    FormantScan d{};
    d.keep = f.keep;
    return d;
}

namespace {
struct Tables {
    double v[kFormantTableDoubles];
    Tables() {
        double* const w = v;
        double* const lag = v + kFormantWin;
        double* const g = lag + kFormantOrder + 1;
        for (int j = 0; j < kFormantWin; j++) w[j] = 0.5 - 0.5 * std::cos(2.0 * M_PI * ((double)j + 0.5) / (double)kFormantWin);
        for (int l = 0; l <= kFormantOrder; l++) {
            const double a = 2.0 * M_PI * 60.0 * (double)l / 24000.0;
            lag[l] = std::exp(-0.5 * a * a);
        }
        lag[0] = 1.0001;
        for (int k = 0; k <= kFormantOrder; k++) g[k] = std::pow(0.99, (double)k);
    }
};
}  // namespace

const double* formant_tables() {
    static const Tables t;
    return t.v;
}

void formant_analyse_host(const float* x, int64_t n, float* coeffs) {
    const double* const w = formant_tables();
    const double* const lag = w + kFormantWin;
    const double* const g = lag + kFormantOrder + 1;
    const int64_t K = formant_frames(n);
    double v[kFormantWin], r[kFormantOrder + 1];
    for (int64_t f = 0; f < K; f++) {
        const int64_t at = kFormantHop * f - kFormantHop;
        for (int j = 0; j < kFormantWin; j++) {
            const int64_t i = at + j;
            const float s = i >= 0 && i < n ? x[i] : 0.0f;
            v[j] = (double)s * w[j];
        }
        for (int l = 0; l <= kFormantOrder; l++) r[l] = formant_lag(v, l);
        formant_solve(r, lag, g, coeffs + f * kFormantOrder);
    }
}

void formant_whiten_host(const float* coeffs, const float* x, int64_t n, float* e) {
    const int64_t K = formant_frames(n);
    const auto at = [&](int64_t i) { return i >= 0 && i < n ? x[i] : 0.0f; };
    for (int64_t i = 0; i < n; i++) {
        const FormantPair q = formant_pair(i, K);
        const float A = formant_residual(coeffs + q.fa * kFormantOrder, at, i);
        const float B = formant_residual(coeffs + q.fb * kFormantOrder, at, i);
        e[i] = formant_mix(A, B, q.u);
    }
}

void formant_shape_host(const float* coeffs, int64_t n, int32_t p, const float* e_r, int64_t n_r, float* out) {
    const int64_t K = formant_frames(n);
    if (K <= 0) {   // (no frame: nothing to put back)
        for (int64_t j = 0; j < n_r; j++) out[j] = e_r[j];
        return;
    }
    std::vector<float> y((size_t)kFormantSlots * kFormantHop);
    for (int64_t j0 = 0; j0 < n_r; j0 += kFormantHop) {
        const int64_t j1 = std::min<int64_t>(j0 + kFormantHop, n_r);
        const int64_t f_lo = formant_tile_first(j0, p, K);
        const int64_t f_hi = formant_pair(((j1 - 1) * (int64_t)p) / 1000, K).fb;
        for (int64_t f = f_lo; f <= f_hi && f < f_lo + kFormantSlots; f++) {
            const float* const a = coeffs + f * kFormantOrder;
            float h[kFormantOrder] = {};   // h[k - 1]: Y[m - k]
            float* const yf = y.data() + (size_t)(f - f_lo) * kFormantHop;
            for (int64_t m = j0 - kFormantWarm; m < j1; m++) {
                float acc = m >= 0 && m < n_r ? e_r[m] : 0.0f;
                for (int k = 1; k <= kFormantOrder; k++) acc = __builtin_fmaf(-a[k - 1], h[k - 1], acc);
                for (int k = kFormantOrder - 1; k > 0; k--) h[k] = h[k - 1];
                h[0] = acc;
                if (m >= j0) yf[m - j0] = acc;
            }
        }
        for (int64_t j = j0; j < j1; j++) {
            const FormantPair q = formant_pair((j * (int64_t)p) / 1000, K);
            out[j] = formant_mix(y[(size_t)(q.fa - f_lo) * kFormantHop + (size_t)(j - j0)], y[(size_t)(q.fb - f_lo) * kFormantHop + (size_t)(j - j0)], q.u);
        }
    }
}

}  // namespace ptts

using namespace ptts;

namespace {
std::string row_error(int64_t n) {
    if (n < 0 || n >= kTempoMaxSamples) return strfmt("formant: n %lld is not from 0 to below 2^31 - %d", (long long)n, kTempoRadius);
    return std::string();
}
}  // namespace

extern "C" {

int32_t ptts_formant_frames(int64_t n) {
    const std::string err = row_error(n);
    if (!err.empty()) return -(int32_t)fail(err);
    return (int32_t)formant_frames(n);
}

int ptts_formant_analyse(const float* x, int64_t n, float* coeffs) {
    const std::string err = row_error(n);
    if (!err.empty()) return fail(err);
    if (n > 0 && (!x || !coeffs)) return fail("formant: null argument");
    formant_analyse_host(x, n, coeffs);
    return PTTS_OK;
}

int ptts_formant_whiten(const float* coeffs, const float* x, int64_t n, float* e) {
    const std::string err = row_error(n);
    if (!err.empty()) return fail(err);
    if (n > 0 && (!coeffs || !x || !e)) return fail("formant: null argument");
    if (n > 0 && x == e) return fail("formant: e is x (a residual sample reads the 24 inputs in front of it)");
    formant_whiten_host(coeffs, x, n, e);
    return PTTS_OK;
}

int ptts_formant_shape(const float* coeffs, int64_t n, int32_t pitch_permille, const float* e_r, int64_t n_r, float* out) {
    std::string err = row_error(n);
    if (err.empty()) err = formant_pitch_error(pitch_permille);
    if (err.empty() && n_r != pitch_resample_length(n, pitch_permille))
        err = strfmt("formant: n_r %lld is not the resampled length %lld of n %lld at pitch_permille %d", (long long)n_r, (long long)pitch_resample_length(n, pitch_permille),
                     (long long)n, pitch_permille);
    if (err.empty()) err = pitch_length_error(n, pitch_permille, 1000);
    if (!err.empty()) return fail(err);
    if (n_r > 0 && (!coeffs || !e_r || !out)) return fail("formant: null argument");
    if (n_r > 0 && e_r == out) return fail("formant: out is e_r (a tile reads the residual in front of where it writes)");
    formant_shape_host(coeffs, n, pitch_permille, e_r, n_r, out);
    return PTTS_OK;
}

int ptts_formant_apply(const ptts_formant_opts* f, const ptts_pitch_opts* p, const ptts_tempo_opts* t, const float* in, int64_t n, float* out) {
    std::string err = formant_opts_error(f);
    if (err.empty()) err = pitch_opts_error(p);
    if (!err.empty()) return fail(err);
    if (!f->keep || p->pitch_permille == 1000) return ptts_pitch_apply(p, t, in, n, out);   // the part as without the option
    if (t) err = tempo_opts_error(t);
    if (err.empty()) err = formant_pitch_error(p->pitch_permille);
    PitchSteps run{};
    if (err.empty()) err = pitch_steps(p->pitch_permille, t ? t->speed_permille : 1000, &run);
    if (err.empty()) err = pitch_length_error(n, p->pitch_permille, run.E);
    if (!err.empty()) return fail(err);
    const PitchScan d = pitch_design(*p);
    const int64_t n_r = pitch_resample_length(n, d.p), n_f = tempo_length(n_r, run.E);
    if ((n > 0 && !in) || (n_f > 0 && !out)) return fail("formant: null argument");
    if (n > 0 && in == out) return fail("formant: out is in (an output reads the inputs around where it writes)");
    if (n == 0) return PTTS_OK;
    std::vector<float> coeffs((size_t)formant_frames(n) * kFormantOrder), e((size_t)n), er((size_t)std::max<int64_t>(n_r, 1)), z;
    formant_analyse_host(in, n, coeffs.data());
    formant_whiten_host(coeffs.data(), in, n, e.data());
    pitch_resample_host(d, e.data(), n, er.data());
    if (!run.tempo) {
        formant_shape_host(coeffs.data(), n, d.p, er.data(), n_r, out);
        return PTTS_OK;
    }
    z.resize((size_t)std::max<int64_t>(n_r, 1));
    formant_shape_host(coeffs.data(), n, d.p, er.data(), n_r, z.data());
    TempoScan td{};
    td.speed = run.E;
    tempo_apply_host(td, z.data(), n_r, out);
    return PTTS_OK;
}

}  // extern "C"
