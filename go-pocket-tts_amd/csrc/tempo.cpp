// tempo.cpp -- the speaking rate of one part of a joined text, on the host (include/ptts.h ptts_tempo_opts, ptts_tempo_length, ptts_tempo_plan,
// ptts_tempo_apply; tempo.h has the rule): the checks of the caller's options and the statement of the result, which k_tempo_plan and
// k_tempo_store (tempo.hip) give bit for bit.  ptts_dsp_ext_set_tempo is with the handle's other setters (capi_rows.cpp).
// No HIP header: the file builds with a plain C++ compiler, alone (tests/test_tempo_cpu.py does, with sanitizers).
//
// The blend of a splice is two f32 divisions, two f32 products and one f32 sum, each rounded once.  Nothing here may be contracted into a fused
// multiply-add.
#include "tempo.h"

#include <cstddef>
#include <cstring>

#include "opts_check.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ptts {

std::string tempo_opts_error(const ptts_tempo_opts* t) {
    if (!t) return "tempo: null options";
    constexpr size_t kKnown = sizeof(ptts_tempo_opts);
    std::string e = opts_size_error("tempo", t, t->size, kKnown, kKnown, "the fields up to reserved");
    if (!e.empty()) return e;
    if (t->speed_permille < 500 || t->speed_permille > 2000)
        return strfmt("tempo: speed_permille %d is not from 500 to 2000 (1000: unchanged)", t->speed_permille);
    if (t->reserved[0] != 0 || t->reserved[1] != 0) return "tempo: reserved is not 0";
    return std::string();
}

TempoScan tempo_design(const ptts_tempo_opts& t) {
    TempoScan d{};
    d.speed = t.speed_permille;
    return d;
}

namespace {
inline float at(const float* x, int64_t n, int64_t i) { return i >= 0 && i < n ? x[i] : 0.0f; }

// One walk over the row's hops.  hop(k, p_k, c_k) is called for k = 0 .. F - 1 in order (c_0 = 0)
template <class Hop>
void tempo_walk(const TempoScan& d, const float* x, int64_t n, Hop&& hop) {
    const int64_t F = tempo_hops(tempo_length(n, d.speed));
    int32_t tmpl[kTempoHop], win[kTempoWindow];
    int64_t prev = 0;
    if (F > 0) hop((int64_t)0, (int64_t)0, (int64_t)0);
    for (int64_t k = 1; k < F; k++) {
        const int64_t a = tempo_target(k, d.speed), c = prev + kTempoHop;
        for (int j = 0; j < kTempoHop; j++) tmpl[j] = tempo_quant(at(x, n, c + j));
        for (int i = 0; i < kTempoWindow; i++) win[i] = tempo_quant(at(x, n, a - kTempoRadius + i));
        uint64_t best = ~(uint64_t)0;
        for (int lag = 0; lag < kTempoLags; lag++) {
            int32_t S = 0;
            for (int j = 0; j < kTempoHop; j++) {
                const int32_t e = win[lag + j] - tmpl[j];
                S += e < 0 ? -e : e;
            }
            const uint64_t key = tempo_key(S, lag - kTempoRadius);
            if (key < best) best = key;
        }
        const int64_t p = a + tempo_key_lag(best);
        hop(k, p, c);
        prev = p;
    }
}
}  // namespace

void tempo_plan_host(const TempoScan& d, const float* x, int64_t n, int32_t* p) {
    tempo_walk(d, x, n, [&](int64_t k, int64_t pk, int64_t) { p[k] = (int32_t)pk; });
}

void tempo_apply_host(const TempoScan& d, const float* x, int64_t n, float* out) {
    const int64_t n_out = tempo_length(n, d.speed);
    tempo_walk(d, x, n, [&](int64_t k, int64_t p, int64_t c) {
        const int64_t m0 = k * kTempoHop;
        const int cnt = (int)(n_out - m0 < kTempoHop ? n_out - m0 : kTempoHop);
        if (k == 0 || p == c) {   // the hop continues its predecessor: its samples' own 32 bits
            for (int j = 0; j < cnt; j++) {
                const float v = at(x, n, p + j);
                std::memcpy(out + m0 + j, &v, sizeof v);
            }
            return;
        }
        for (int j = 0; j < cnt; j++) {
            const float pa = at(x, n, c + j) * tempo_w_out(j), pb = at(x, n, p + j) * tempo_w_in(j);
            out[m0 + j] = pa + pb;
        }
    });
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int64_t ptts_tempo_length(const ptts_tempo_opts* t, int64_t n) {
    const std::string err = tempo_opts_error(t);
    if (!err.empty()) return -(int64_t)fail(err);
    if (n < 0 || n >= kTempoMaxSamples) return -(int64_t)fail(strfmt("tempo: n %lld is not from 0 to below 2^31 - %d", (long long)n, kTempoRadius));
    return tempo_length(n, t->speed_permille);
}

int ptts_tempo_plan(const ptts_tempo_opts* t, const float* x, int64_t n, int32_t* positions) {
    const std::string err = tempo_opts_error(t);
    if (!err.empty()) return fail(err);
    if (n < 0 || n >= kTempoMaxSamples) return fail(strfmt("tempo: n %lld is not from 0 to below 2^31 - %d", (long long)n, kTempoRadius));
    const TempoScan d = tempo_design(*t);
    if ((!x && n > 0) || (!positions && tempo_length(n, d.speed) > 0)) return fail("tempo: null argument");
    tempo_plan_host(d, x, n, positions);
    return PTTS_OK;
}

int ptts_tempo_apply(const ptts_tempo_opts* t, const float* in, int64_t n, float* out) {
    const std::string err = tempo_opts_error(t);
    if (!err.empty()) return fail(err);
    if (n < 0 || n >= kTempoMaxSamples) return fail(strfmt("tempo: n %lld is not from 0 to below 2^31 - %d", (long long)n, kTempoRadius));
    const TempoScan d = tempo_design(*t);
    if ((!in && n > 0) || (!out && tempo_length(n, d.speed) > 0)) return fail("tempo: null argument");
    if (in && in == out) return fail("tempo: out is in (a hop reads the input behind and in front of where it writes)");
    tempo_apply_host(d, in, n, out);
    return PTTS_OK;
}

}  // extern "C"
