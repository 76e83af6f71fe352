// pitch.cpp -- the pitch of one part of a joined text, on the host (include/ptts.h ptts_pitch_opts, ptts_pitch_speed, ptts_pitch_resample_length,
// ptts_pitch_resample, ptts_pitch_length, ptts_pitch_apply, ptts_pitch_table; pitch.h has the rule): the checks of the caller's options, the
// prototype table and the statement of the result, which k_pitch_resample (pitch.hip) gives bit for bit and the tempo (tempo.cpp) finishes.
// ptts_dsp_ext_set_pitch is in capi_rows.cpp, with the handle's trim and tempo setters (dsp_ext.h has the one setter they all call).
// No HIP header: the file builds with a plain C++ compiler, with tempo.cpp alone (tests/test_pitch_cpu.py does, with sanitizers).
//
// A tap is two fused multiply-adds, written as such; the output's gain is one f32 product.  Nothing else here may be contracted.
#include "pitch.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "opts_check.h"
#include "rate_taps.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ptts {

std::string pitch_opts_error(const ptts_pitch_opts* p) {
    if (!p) return "pitch: null options";
    constexpr size_t kKnown = sizeof(ptts_pitch_opts);
    std::string e = opts_size_error("pitch", p, p->size, kKnown, kKnown, "the fields up to reserved");
    if (!e.empty()) return e;
    if (p->pitch_permille < 500 || p->pitch_permille > 2000)
        return strfmt("pitch: pitch_permille %d is not from 500 to 2000 (1000: unchanged)", p->pitch_permille);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "pitch: reserved is not 0";
    return std::string();
}

std::string pitch_steps(int32_t p, int32_t s, PitchSteps* st) {
    const int32_t e = pitch_speed(s, p);
    *st = PitchSteps{e, false, false};
    if (e < 500 || e > 2000)
        return strfmt("pitch: speed_permille %d with pitch_permille %d needs the tempo at %d, which is not from 500 to 2000", s, p, e);
    st->resample = p != 1000;
    st->tempo = e != 1000;
    return std::string();
}

std::string pitch_length_error(int64_t n, int32_t p, int32_t E) {
    // (n below 2^33 keeps n * 1000 far inside an int64; a longer row has a resampled length of 2^32 and more anyway)
    if (n < 0 || n >= ((int64_t)1 << 33)) return strfmt("pitch: n %lld is not from 0 to where its lengths stay below 2^31 - %d", (long long)n, kTempoRadius);
    const int64_t n_r = pitch_resample_length(n, p);
    if (n_r >= kTempoMaxSamples)
        return strfmt("pitch: n %lld at pitch_permille %d has the resampled length %lld, a row must stay below 2^31 - %d", (long long)n, p, (long long)n_r, kTempoRadius);
    const int64_t n_f = tempo_length(n_r, E);
    if (n_f >= kTempoMaxSamples)
        return strfmt("pitch: n %lld at pitch_permille %d and the tempo at %d has the final length %lld, a row must stay below 2^31 - %d", (long long)n, p, E,
                      (long long)n_f, kTempoRadius);
    return std::string();
}

PitchScan pitch_design(const ptts_pitch_opts& p) {
    PitchScan d{};
    d.p = p.pitch_permille;
    d.D = d.p > 1000 ? d.p : 1000;
    d.g = (float)(1000.0 / (double)d.D);
    return d;
}

namespace {
struct PitchTable {
    std::vector<float> h, hd;
    PitchTable() : h((size_t)kPitchEntries + 1, 0.0f), hd((size_t)kPitchEntries, 0.0f) {
        const double fc = 0.45, W = (double)kPitchSupport / 3.0, i0b = bessel_i0(kKaiserBeta);
        for (int q = 0; q < kPitchEntries; q++) {
            if (3 * q >= kPitchSupport * kPitchR) continue;   // outside |t| < W: 0
            const double t = (double)q / kPitchR, x = 2.0 * fc * t;
            const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
            const double r = t / W, win = bessel_i0(kKaiserBeta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            h[(size_t)q] = (float)(2.0 * fc * sinc * win);
        }
        for (int q = 0; q < kPitchEntries; q++) hd[(size_t)q] = h[(size_t)q + 1] - h[(size_t)q];
    }
};
const PitchTable& table() {
    static const PitchTable t;
    return t;
}
}  // namespace

const float* pitch_table_h() { return table().h.data(); }
const float* pitch_table_hd() { return table().hd.data(); }

void pitch_resample_host(const PitchScan& d, const float* x, int64_t n, float* out) {
    const float* const h = pitch_table_h();
    const float* const hd = pitch_table_hd();
    const int64_t n_r = pitch_resample_length(n, d.p);
    const float fD = (float)d.D;
    for (int64_t j = 0; j < n_r; j++) {
        const int64_t c = j * (int64_t)d.p;
        const int64_t i0 = std::max<int64_t>(pitch_first(c, d.D), 0), i1 = std::min<int64_t>(pitch_last(c, d.D), n - 1);
        float acc = 0.0f;
        for (int64_t i = i0; i <= i1; i++) {
            const int64_t a = std::llabs(c - 1000 * i), num = a * kPitchR;
            const int64_t q = num / d.D, r = num % d.D;
            const float frac = (float)r / fD;
            const float coef = std::fmaf(hd[q], frac, h[q]);
            acc = std::fmaf(x[i], coef, acc);
        }
        out[j] = acc * d.g;
    }
}

}  // namespace ptts

using namespace ptts;

namespace {
// the options of one call, checked: the design and what the pair resolves to (pitch_steps), the tempo's speed being 1000 without one
struct Stage { PitchScan d; PitchSteps run; };
std::string stage_of(const ptts_pitch_opts* p, const ptts_tempo_opts* t, Stage* st) {
    std::string e = pitch_opts_error(p);
    if (e.empty() && t) e = tempo_opts_error(t);
    if (!e.empty()) return e;
    st->d = pitch_design(*p);
    return pitch_steps(st->d.p, t ? t->speed_permille : 1000, &st->run);
}
}  // namespace

extern "C" {

int32_t ptts_pitch_speed(const ptts_pitch_opts* p, const ptts_tempo_opts* t) {
    Stage st;
    const std::string err = stage_of(p, t, &st);
    if (!err.empty()) return -(int32_t)fail(err);
    return st.run.E;
}

int64_t ptts_pitch_resample_length(const ptts_pitch_opts* p, int64_t n) {
    std::string err = pitch_opts_error(p);
    if (err.empty()) err = pitch_length_error(n, p->pitch_permille, 1000);
    if (!err.empty()) return -(int64_t)fail(err);
    return pitch_resample_length(n, p->pitch_permille);
}

int ptts_pitch_resample(const ptts_pitch_opts* p, const float* in, int64_t n, float* out) {
    std::string err = pitch_opts_error(p);
    if (err.empty()) err = pitch_length_error(n, p->pitch_permille, 1000);
    if (!err.empty()) return fail(err);
    const PitchScan d = pitch_design(*p);
    if (n > 0 && (!in || !out)) return fail("pitch: null argument");
    if (n > 0 && in == out) return fail("pitch: out is in (an output reads the inputs around where it writes)");
    if (d.p == 1000) {   // z is x
        if (n > 0) std::memcpy(out, in, (size_t)n * sizeof(float));
        return PTTS_OK;
    }
    pitch_resample_host(d, in, n, out);
    return PTTS_OK;
}

int64_t ptts_pitch_length(const ptts_pitch_opts* p, const ptts_tempo_opts* t, int64_t n) {
    Stage st;
    std::string err = stage_of(p, t, &st);
    if (err.empty()) err = pitch_length_error(n, st.d.p, st.run.E);
    if (!err.empty()) return -(int64_t)fail(err);
    return tempo_length(pitch_resample_length(n, st.d.p), st.run.E);
}

int ptts_pitch_apply(const ptts_pitch_opts* p, const ptts_tempo_opts* t, const float* in, int64_t n, float* out) {
    Stage st;
    std::string err = stage_of(p, t, &st);
    if (err.empty()) err = pitch_length_error(n, st.d.p, st.run.E);
    if (!err.empty()) return fail(err);
    const int64_t n_r = pitch_resample_length(n, st.d.p), n_f = tempo_length(n_r, st.run.E);
    if ((n > 0 && !in) || (n_f > 0 && !out)) return fail("pitch: null argument");
    if (n > 0 && in == out) return fail("pitch: out is in (an output reads the inputs around where it writes)");
    // ptts_tempo_apply at E over ptts_pitch_resample; either step may be the identity
    std::vector<float> z;
    const float* zr = in;
    if (st.run.resample) {
        if (!st.run.tempo) { pitch_resample_host(st.d, in, n, out); return PTTS_OK; }
        z.resize((size_t)std::max<int64_t>(n_r, 1));
        pitch_resample_host(st.d, in, n, z.data());
        zr = z.data();
    }
    if (!st.run.tempo) {
        if (n > 0) std::memcpy(out, in, (size_t)n * sizeof(float));
        return PTTS_OK;
    }
    TempoScan td{};
    td.speed = st.run.E;
    tempo_apply_host(td, zr, n_r, out);
    return PTTS_OK;
}

int ptts_pitch_table(const float** h, const float** hd, int32_t* entries) {
    if (h) *h = pitch_table_h();
    if (hd) *hd = pitch_table_hd();
    if (entries) *entries = kPitchEntries;
    return PTTS_OK;
}

}  // extern "C"
