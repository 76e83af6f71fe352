// join.cpp -- a text's parts joined into one utterance, on the host (include/ptts.h ptts_join_length, ptts_join; join.h).  The reference appends
// the chunks' PCM (internal/tts/service.go:107-153); a gap of silence or a crossfade at the seams is this library's addition.  This file is
// the statement of the result: k_join (join.hip) gives these bits.  No HIP header.
//
// The crossfade at a seam of K samples is dsp_fade_out of the predecessor's tail plus dsp_fade_in of the successor's head (dsp.cpp): two f32
// divisions, two f32 products, one f32 sum, each rounded once.  Nothing here may be contracted into a fused multiply-add.
#include "join.h"

#include <cmath>
#include <cstddef>
#include <cstring>

#include "opts_check.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ptts {

static int64_t ms_samples(double ms) { return (int64_t)(ms / 1000.0 * (double)kJoinRate); }   // dsp_fade_in's expression

std::string join_opts_error(const ptts_join_opts* o, JoinLens* out) {
    if (!o) return "join: null options";
    constexpr size_t kKnown = sizeof(ptts_join_opts);
    std::string e = opts_size_error("join", o, o->size, kKnown, kKnown, "the fields up to crossfade_ms");
    if (!e.empty()) return e;
    if (range_error("join", "gap_ms", o->gap_ms, 0.0, kJoinMaxMs, e)) return e;
    if (range_error("join", "crossfade_ms", o->crossfade_ms, 0.0, kJoinMaxMs, e)) return e;
    if (o->gap_ms > 0.0 && o->crossfade_ms > 0.0)
        return strfmt("join: gap_ms %g and crossfade_ms %g are both set, at most one of them may be above 0", o->gap_ms, o->crossfade_ms);
    if (out) *out = JoinLens{ms_samples(o->gap_ms), ms_samples(o->crossfade_ms)};
    return std::string();
}

std::string join_stream_opts_error(const ptts_join_stream_opts* so) {
    if (!so) return "join: stream: null options";
    constexpr size_t kKnown = sizeof(ptts_join_stream_opts);
    std::string e = opts_size_error("join: stream", so, so->size, kKnown, kKnown, "the fields up to pcm_user");
    if (!e.empty()) return e;
    if (so->first_group < 0) return strfmt("join: stream: first_group %d is negative (0: max_batch, else the parts of the first group)", so->first_group);
    return std::string();
}

int64_t join_stream_hold(const ptts_join_opts& o, const JoinLens& l) {
    const int64_t fo = o.dsp && o.dsp->fade_out_ms > 0.0 ? ms_samples(o.dsp->fade_out_ms) : 0;
    return std::max(l.xfade, fo);
}

std::string join_plan(const int64_t* n, int32_t rows, const JoinLens& l, int64_t* offsets, int64_t* seams, int64_t* total) {
    if (rows < 1 || rows > kJoinMaxRows) return strfmt("join: rows %d is not from 1 to %d", rows, kJoinMaxRows);
    if (!n) return "join: null lengths";
    int64_t off = 0;
    for (int32_t i = 0; i < rows; i++) {
        if (n[i] < 0) return strfmt("join: part %d has a negative length %lld", i, (long long)n[i]);
        if (n[i] >= kJoinMaxSamples) return strfmt("join: part %d has %lld samples, the joined length must stay below 2^31", i, (long long)n[i]);
        const int64_t k = i ? join_seam(l.xfade, n[i - 1], n[i]) : 0;
        if (i) off += n[i - 1] + l.gap - k;
        if (off + n[i] >= kJoinMaxSamples) return strfmt("join: the joined length reaches %lld samples at part %d, it must stay below 2^31", (long long)(off + n[i]), i);
        if (offsets) offsets[i] = off;
        if (seams) seams[i] = k;
    }
    if (total) *total = off + n[rows - 1];
    return std::string();
}

void join_host(const float* const* in, const int64_t* n, int32_t rows, const JoinLens& l, float* out) {
    int64_t off = 0;
    for (int32_t i = 0; i < rows; i++) {
        const int64_t k = i ? join_seam(l.xfade, n[i - 1], n[i]) : 0;           // the seam in front of part i
        const int64_t k_next = i + 1 < rows ? join_seam(l.xfade, n[i], n[i + 1]) : 0;   // ... and behind it: the successor writes those samples
        if (i) {
            for (int64_t g = 0; g < l.gap; g++) out[off + n[i - 1] + g] = 0.0f;
            off += n[i - 1] + l.gap - k;
        }
        const float* b = in[i];
        const float* a = k ? in[i - 1] + (n[i - 1] - k) : nullptr;
        const float kf = (float)k;
        for (int64_t j = 0; j < k; j++) {
            const float wa = (float)(k - 1 - j) / kf, wb = (float)j / kf;
            const float pa = a[j] * wa, pb = b[j] * wb;
            out[off + j] = pa + pb;
        }
        if (n[i] - k_next > k) std::memcpy(out + off + k, b + k, (size_t)(n[i] - k_next - k) * sizeof(float));   // bit for bit
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" {

int64_t ptts_join_length(const int64_t* n, int32_t rows, const ptts_join_opts* opts, int64_t* offsets) {
    JoinLens l;
    std::string e = join_opts_error(opts, &l);
    int64_t total = 0;
    if (e.empty()) e = join_plan(n, rows, l, offsets, nullptr, &total);
    if (!e.empty()) return -(int64_t)fail(e);
    return total;
}

int64_t ptts_join_stream_ready(const ptts_join_opts* o, int64_t joined) {
    JoinLens l;
    std::string e = join_opts_error(o, &l);
    if (e.empty() && joined < 0) e = strfmt("join: stream: joined %lld is negative", (long long)joined);
    if (!e.empty()) return -(int64_t)fail(e);
    return join_stream_ready(joined, join_stream_hold(*o, l));
}

int ptts_join(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* opts, float* out) {
    JoinLens l;
    std::string e = join_opts_error(opts, &l);
    int64_t total = 0;
    if (e.empty()) e = join_plan(n, rows, l, nullptr, nullptr, &total);
    if (!e.empty()) return fail(e);
    if (!in || (!out && total > 0)) return fail("join: null argument");
    for (int32_t i = 0; i < rows; i++)
        if (!in[i] && n[i] > 0) return fail(strfmt("join: part %d is null", i));
    join_host(in, n, rows, l, out);
    return PTTS_OK;
}

}  // extern "C"
