// eq.cpp -- a request's equaliser on the host (include/ptts.h ptts_eq_*): the design of its sections (the published
// RBJ cookbook, Q form, float64), the handle with the cascade's state matrix and its powers, the registry of live handles (every kind's: true_peak.cpp's too), and ptts_eq_apply:
// the cascade in the blocked form of scan_block.h -- the functions dsp.hip's k_eq_* kernels call, instantiated for the host -- so a request's
// `eq` and ptts_eq_rows give these bits.  No HIP header: the file builds with a plain C++ compiler (tests/test_eq_cpu.py does, with sanitizers).
#include <cmath>
#include <complex>
#include <mutex>
#include <new>
#include <set>
#include <utility>

#include "eq.h"
#include "opts_check.h"

namespace ptts {

namespace {
constexpr double kEqRate = 24000.0;

std::mutex g_live_mu;
std::set<std::pair<const void*, int>>& live() {
    static std::set<std::pair<const void*, int>>* s = new std::set<std::pair<const void*, int>>();   // (never destroyed: handles may be freed while the process exits)
    return *s;
}

std::string sections_error(const ptts_eq_section* s, int32_t n) {
    if (!s) return "eq: null sections";
    if (n < 1 || n > kEqMaxSections) return strfmt("eq: n is %d, a cascade has 1 to %d sections", n, kEqMaxSections);
    for (int i = 0; i < n; i++) {
        const std::string e = eq_section_error(s[i], i);
        if (!e.empty()) return e;
    }
    return std::string();
}
}  // namespace

std::string eq_section_error(const ptts_eq_section& s, int index) {
    if (s.type < PTTS_EQ_LOWPASS || s.type > PTTS_EQ_PEAKING) return strfmt("eq: section %d: type %d is not a PTTS_EQ_* type", index, s.type);
    if (s.reserved) return strfmt("eq: section %d: reserved is %d, must be 0", index, s.reserved);
    std::string e;
    const std::string stage = strfmt("eq: section %d", index);
    if (range_error(stage.c_str(), "freq_hz", s.freq_hz, 10.0, 11000.0, e)) return e;
    if (range_error(stage.c_str(), "q", s.q, 0.1, 10.0, e)) return e;
    const bool pass = s.type == PTTS_EQ_LOWPASS || s.type == PTTS_EQ_HIGHPASS;
    if (pass && !(s.gain_db == 0.0)) return strfmt("eq: section %d: gain_db %g must be 0 for a low-pass or a high-pass", index, s.gain_db);
    if (range_error(stage.c_str(), "gain_db", s.gain_db, -24.0, 24.0, e)) return e;
    return std::string();
}

DspBiquad eq_design(const ptts_eq_section& s) {
#pragma clang fp contract(off)
    const double w0 = 2.0 * M_PI * s.freq_hz / kEqRate;
    const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * s.q);
    double b0, b1, b2, a0, a1, a2;
    if (s.type == PTTS_EQ_LOWPASS || s.type == PTTS_EQ_HIGHPASS) {
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        if (s.type == PTTS_EQ_LOWPASS) { b0 = (1.0 - cw) / 2.0; b1 = 1.0 - cw; b2 = b0; }
        else { b0 = (1.0 + cw) / 2.0; b1 = -(1.0 + cw); b2 = b0; }
    } else {
        const double A = std::pow(10.0, s.gain_db / 40.0);
        if (s.type == PTTS_EQ_PEAKING) {
            b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A;
            a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A;
        } else {
            const double sq = 2.0 * std::sqrt(A) * alpha, p = A + 1.0, m = A - 1.0;
            if (s.type == PTTS_EQ_LOWSHELF) {
                b0 = A * (p - m * cw + sq); b1 = 2.0 * A * (m - p * cw); b2 = A * (p - m * cw - sq);
                a0 = p + m * cw + sq; a1 = -2.0 * (m + p * cw); a2 = p + m * cw - sq;
            } else {
                b0 = A * (p + m * cw + sq); b1 = -2.0 * A * (m + p * cw); b2 = A * (p + m * cw - sq);
                a0 = p - m * cw + sq; a1 = 2.0 * (m - p * cw); a2 = p - m * cw - sq;
            }
        }
    }
    return DspBiquad{b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
}

// The state matrix with x = 0: section k reads v_k (v_0 = 0, v_(k+1) = u_k) and gives u_k = b0 v_k + z1_k, z1_k' = b1 v_k - a1 u_k + z2_k,
// z2_k' = b2 v_k - a2 u_k; v and u are carried as their coefficients over the N states
EqScan eq_scan_coeffs(const DspBiquad* c, int n) {
#pragma clang fp contract(off)
    EqScan sc{};
    sc.S = n;
    for (int k = 0; k < n; k++) sc.c[k] = c[k];
    const int N = 2 * n;
    double A[4 * kEqMaxSections * kEqMaxSections] = {};
    double v[2 * kEqMaxSections] = {}, u[2 * kEqMaxSections];
    for (int k = 0; k < n; k++) {
        const DspBiquad& q = c[k];
        for (int j = 0; j < N; j++) u[j] = q.b0 * v[j] + (j == 2 * k ? 1.0 : 0.0);
        for (int j = 0; j < N; j++) {
            A[N * (2 * k) + j] = q.b1 * v[j] - q.a1 * u[j] + (j == 2 * k + 1 ? 1.0 : 0.0);
            A[N * (2 * k + 1) + j] = q.b2 * v[j] - q.a2 * u[j];
        }
        for (int j = 0; j < N; j++) v[j] = u[j];
    }
    switch (n) {
        case 1: scan_powers<2>(A, sc.a_run, sc.a_tile); break;
        case 2: scan_powers<4>(A, sc.a_run, sc.a_tile); break;
        case 3: scan_powers<6>(A, sc.a_run, sc.a_tile); break;
        default: scan_powers<8>(A, sc.a_run, sc.a_tile); break;
    }
    return sc;
}

void eq_apply_blocked(const EqScan& sc, float* x, int64_t n) {
    eq_dispatch(sc, [&](const auto& sys) {
        scan_walk(sys, x, n, [&](int64_t i0, int count, double* z) { sys.run(x + i0, count, z, x + i0); });
    });
}

void handle_add(const void* h, HandleKind kind) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    live().insert({h, kind});
}

bool handle_take(const void* h, HandleKind kind) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    return live().erase({h, kind}) != 0;
}

bool handle_live(const void* h, HandleKind kind) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    return h && live().count({h, kind});
}

bool handle_locked(const void* h, HandleKind kind, void (*f)(void* ctx), void* ctx) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    if (!h || !live().count({h, kind})) return false;
    f(ctx);
    return true;
}

const EqScan* eq_lookup(const ptts_eq* e) { return handle_live(e, HANDLE_EQ) ? &e->sc : nullptr; }

}  // namespace ptts

using namespace ptts;

extern "C" {

int ptts_eq_design(const ptts_eq_section* s, double coeffs[5]) {
    if (!s || !coeffs) return fail("eq: null argument");
    const std::string e = eq_section_error(*s, 0);
    if (!e.empty()) return fail(e);
    const DspBiquad c = eq_design(*s);
    coeffs[0] = c.b0; coeffs[1] = c.b1; coeffs[2] = c.b2; coeffs[3] = c.a1; coeffs[4] = c.a2;
    return PTTS_OK;
}

int ptts_eq_response(const ptts_eq_section* s, int32_t n, double freq_hz, double* gain_db) {
    if (!gain_db) return fail("eq: null argument");
    const std::string e = sections_error(s, n);
    if (!e.empty()) return fail(e);
    if (!(freq_hz > 0.0 && freq_hz < kEqRate / 2.0)) return fail(strfmt("eq: response: freq_hz %g is not above 0 and below %g", freq_hz, kEqRate / 2.0));
    const double w = 2.0 * M_PI * freq_hz / kEqRate;
    const std::complex<double> z1 = std::polar(1.0, -w), z2 = std::polar(1.0, -2.0 * w);
    double db = 0.0;
    for (int i = 0; i < n; i++) {
        const DspBiquad c = eq_design(s[i]);
        db += 20.0 * std::log10(std::abs(c.b0 + c.b1 * z1 + c.b2 * z2) / std::abs(1.0 + c.a1 * z1 + c.a2 * z2));
    }
    *gain_db = db;
    return PTTS_OK;
}

int ptts_eq_create(const ptts_eq_section* s, int32_t n, ptts_eq** out) {
    if (!out) return fail("eq: null argument");
    *out = nullptr;
    const std::string e = sections_error(s, n);
    if (!e.empty()) return fail(e);
    DspBiquad c[kEqMaxSections];
    for (int i = 0; i < n; i++) c[i] = eq_design(s[i]);
    ptts_eq* h = new (std::nothrow) ptts_eq{eq_scan_coeffs(c, n)};
    if (!h) { set_last_error("ptts-hip: out of host memory"); return PTTS_ENOMEM; }
    handle_add(h, HANDLE_EQ);
    *out = h;
    return PTTS_OK;
}

void ptts_eq_free(ptts_eq* e) {
    if (!e) return;
    if (!handle_take(e, HANDLE_EQ)) return;   // not a live handle: nothing of ours to free
    delete e;
}

int ptts_eq_apply(const ptts_eq* e, float* samples, int64_t n) {
    const EqScan* sc = eq_lookup(e);
    if (!sc) return fail("eq: the handle is not a live equaliser of ptts_eq_create");
    if ((!samples && n > 0) || n < 0) return fail("eq: null samples");
    eq_apply_blocked(*sc, samples, n);
    return PTTS_OK;
}

}  // extern "C"
