// resample.cpp -- rates, the polyphase filter and the launches of k_resample (resample.hip).
//
// For a pair (R_in, R_out): g = gcd, L = R_out / g, M = R_in / g, rho = min(1, L / M), cutoff fc = 0.5 rho 0.9 cycles per input sample,
// half-width W = 24 / (2 fc) input samples, Kaiser window beta 8.6:
//     h(t) = 2 fc sinc(2 fc t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta)   for |t| < W, else 0
// computed in float64 and rounded once to f32 (no per-phase normalisation).  Output j sits at input position j M / L; it sums
// x[i] h(j M / L - i) over the i with |j M / L - i| < W in ascending i.  W = 80 / (3 rho) = 80 max(L, M) / (3 L), so with A = 80 max(L, M)
// the support test |p / L - d| < W is the exact integer test 3 |p - d L| < A.
#include <numeric>

#include "rate_taps.h"
#include "runtime.h"

namespace ptts {

namespace {
constexpr int64_t kMaxOut = 48000, kMaxIn = 192000, kMinRate = 8000;

using Shape = RateShape;   // (rate_taps.h: the design, shared with the true-peak meter)

int pair_tile(const Shape& s) {   // outputs per workgroup: the input window of a tile stays within kResampleWindow floats
    const int64_t t = ((int64_t)(kResampleWindow - s.K - 8) * s.L) / s.M + 1;
    return (int)std::max<int64_t>(4, std::min<int64_t>(kResampleMaxTile, t) & ~(int64_t)3);
}
}  // namespace

std::string rate_error(int64_t rate, bool input) {
    const int64_t hi = input ? kMaxIn : kMaxOut;
    if (rate < kMinRate || rate > hi || rate % 25 != 0)
        return strfmt("ptts-hip: %s sample rate %lld Hz is not supported (a multiple of 25 Hz from %lld to %lld)", input ? "input" : "output", (long long)rate,
                      (long long)kMinRate, (long long)hi);
    return std::string();
}

std::string rate_pair_error(int in_rate, int out_rate) {
    std::string e = rate_error(in_rate, true);
    if (e.empty()) e = rate_error(out_rate, false);
    if (!e.empty() || in_rate == out_rate) return e;
    const Shape s = rate_shape(in_rate, out_rate);
    if (s.L > kResampleMaxL || (int64_t)s.L * s.K > kResampleMaxTaps || s.K + 8 >= kResampleWindow)
        return strfmt("ptts-hip: resampling %d Hz -> %d Hz needs a %d x %d tap table, more than k_resample takes (%d phases, %d taps)", in_rate, out_rate,
                      s.L, s.K, kResampleMaxL, kResampleMaxTaps);
    return std::string();
}

int64_t resample_length(int64_t n_in, int in_rate, int out_rate) {
    if (in_rate == out_rate) return n_in;
    const int g = std::gcd(in_rate, out_rate);
    const int64_t L = out_rate / g, M = in_rate / g;
    return (n_in * L + M - 1) / M;
}

const RateFilter* rate_filter(Model& m, int in_rate, int out_rate, hipStream_t s) {
    const std::string e = rate_pair_error(in_rate, out_rate);
    if (!e.empty()) throw Error(PTTS_EINVAL, e);
    if (in_rate == out_rate) return nullptr;
    std::unique_ptr<RateFilter>& slot = m.rate_filters[{in_rate, out_rate}];
    if (slot) {
        if (slot->up != s) PTTS_HIP(hipStreamWaitEvent(s, slot->ready, 0));   // (the upload's event: complete long ago in the normal case)
        return slot.get();
    }
    const Shape sh = rate_shape(in_rate, out_rate);
    std::unique_ptr<RateFilter> f(new RateFilter());
    f->L = sh.L; f->M = sh.M; f->K = sh.K; f->dlo = sh.dlo; f->A = sh.A; f->tile = pair_tile(sh);
    f->n_taps = ((size_t)sh.L * sh.K + 3) & ~(size_t)3;
    PTTS_HIP(hipHostMalloc((void**)&f->staged, f->n_taps * sizeof(float), hipHostMallocDefault));
    std::memset(f->staged, 0, f->n_taps * sizeof(float));
    rate_taps(sh, f->staged);
    f->taps.ensure(f->n_taps * sizeof(float));
    // (first use: queued on s from page-locked memory, nothing waits on the host; launches on s follow it, other streams wait for `ready`)
    PTTS_HIP(hipMemcpyAsync(f->taps.p, f->staged, f->n_taps * sizeof(float), hipMemcpyHostToDevice, s));
    PTTS_HIP(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
    PTTS_HIP(hipEventRecord(f->ready, s));
    f->up = s;
    slot = std::move(f);
    return slot.get();
}

int64_t resample_ready(const RateFilter* f, int64_t n_dec) {
    if (!f) return n_dec;
    // output j reads inputs up to ceil((3 j M + A) / (3 L)) - 1: inside [0, n_dec) iff 3 j M + A <= 3 L n_dec
    const int64_t lim = 3 * (int64_t)f->L * n_dec - f->A;
    if (lim < 0) return 0;
    return std::min(lim / (3 * (int64_t)f->M) + 1, resample_length(n_dec, f->M, f->L));
}

ResampleRow resample_row(const RateFilter* f, const float* src, int64_t n_in, void* dst, int64_t o0, int64_t o1, int fmt) {
    ResampleRow r{};
    r.src = src; r.dst = dst; r.taps = f ? f->taps.as<float>() : nullptr;
    r.n_in = n_in; r.o0 = o0; r.o1 = o1; r.o_cap = o1;
    r.L = f ? f->L : 1; r.M = f ? f->M : 1; r.K = f ? f->K : 1; r.dlo = f ? f->dlo : 0;
    r.fmt = fmt; r.tile = f ? f->tile : kResampleMaxTile;
    return r;
}

RateFilter::~RateFilter() {
    if (ready) { (void)hipEventSynchronize(ready); (void)hipEventDestroy(ready); }
    if (staged) (void)hipHostFree(staged);
}

void resample_launch(Model& m, const std::vector<ResampleRow>& rows, hipStream_t s) {
    constexpr int kRows = RowRing<ResampleRow>::kRows;
    for (size_t at = 0; at < rows.size(); at += kRows) {
        const int n = (int)std::min<size_t>(kRows, rows.size() - at);
        int64_t tiles = 0;
        size_t lds = 16;
        for (int i = 0; i < n; i++) {
            const ResampleRow& r = rows[at + (size_t)i];
            if (r.o_cap <= r.o0) continue;
            tiles = std::max(tiles, (r.o_cap - r.o0 + r.tile - 1) / r.tile);
            const int ntap = r.taps ? r.L * r.K : 0;
            const int64_t tap_floats = ntap <= kResampleTapsLds ? (ntap + 3) & ~3 : 0;
            const int64_t win = ((((int64_t)(r.tile - 1) * r.M) / r.L + r.K + 8) + 3) & ~(int64_t)3;
            lds = std::max(lds, (size_t)(tap_floats + win) * sizeof(float));
        }
        if (tiles == 0) continue;
        if (tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: resample: too many samples for one launch");
        launch_resample(m.rs_ring.stage(rows.data() + at, n, s), n, (int)tiles, lds, s);
        m.rs_ring.done(s);
    }
}

}  // namespace ptts
