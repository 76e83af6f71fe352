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
#include <memory>

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

// the plan and the join themselves, for any seam lengths: seam(i) is the pair of the seam in front of part i (i >= 1)
template <class Seam>
static std::string plan_with(const int64_t* n, int32_t rows, Seam&& seam, int64_t* offsets, int64_t* seams, int64_t* total) {
    if (rows < 1 || rows > kJoinMaxRows) return strfmt("join: rows %d is not from 1 to %d", rows, kJoinMaxRows);
    if (!n) return "join: null lengths";
    int64_t off = 0;
    for (int32_t i = 0; i < rows; i++) {
        if (n[i] < 0) return strfmt("join: part %d has a negative length %lld", i, (long long)n[i]);
        if (n[i] >= kJoinMaxSamples) return strfmt("join: part %d has %lld samples, the joined length must stay below 2^31", i, (long long)n[i]);
        const JoinLens l = i ? seam(i) : JoinLens{};
        const int64_t k = i ? join_seam(l.xfade, n[i - 1], n[i]) : 0;
        if (i) off += n[i - 1] + l.gap - k;
        if (off + n[i] >= kJoinMaxSamples) return strfmt("join: the joined length reaches %lld samples at part %d, it must stay below 2^31", (long long)(off + n[i]), i);
        if (offsets) offsets[i] = off;
        if (seams) seams[i] = k;
    }
    if (total) *total = off + n[rows - 1];
    return std::string();
}

// g null: no part has a gain, every sample outside a seam moves as its bits
template <class Seam>
static void join_with(const float* const* in, const int64_t* n, int32_t rows, Seam&& seam, const float* g, const bool* apply, float* out) {
    int64_t off = 0;
    for (int32_t i = 0; i < rows; i++) {
        const JoinLens l = i ? seam(i) : JoinLens{};
        const int64_t k = i ? join_seam(l.xfade, n[i - 1], n[i]) : 0;           // the seam in front of part i
        const int64_t k_next = i + 1 < rows ? join_seam(seam(i + 1).xfade, n[i], n[i + 1]) : 0;   // ... and behind it: the successor writes those samples
        if (i) {
            for (int64_t q = 0; q < l.gap; q++) out[off + n[i - 1] + q] = 0.0f;
            off += n[i - 1] + l.gap - k;
        }
        const float* b = in[i];
        const float* a = k ? in[i - 1] + (n[i - 1] - k) : nullptr;
        const bool sb = g && apply[i], sa = g && k && apply[i - 1];
        const float gb = sb ? g[i] : 1.0f, ga = sa ? g[i - 1] : 1.0f;
        const float kf = (float)k;
        for (int64_t j = 0; j < k; j++) {
            const float wa = (float)(k - 1 - j) / kf, wb = (float)j / kf;
            const float va = sa ? a[j] * ga : a[j], vb = sb ? b[j] * gb : b[j];   // the scaled samples: one product each, in front of the seam's
            const float pa = va * wa, pb = vb * wb;
            out[off + j] = pa + pb;
        }
        if (n[i] - k_next <= k) continue;
        if (sb) for (int64_t j = k; j < n[i] - k_next; j++) out[off + j] = b[j] * gb;
        else std::memcpy(out + off + k, b + k, (size_t)(n[i] - k_next - k) * sizeof(float));   // bit for bit
    }
}

std::string join_plan(const int64_t* n, int32_t rows, const JoinLens& l, int64_t* offsets, int64_t* seams, int64_t* total) {
    return plan_with(n, rows, [&](int32_t) { return l; }, offsets, seams, total);
}

void join_host(const float* const* in, const int64_t* n, int32_t rows, const JoinLens& l, float* out) {
    join_with(in, n, rows, [&](int32_t) { return l; }, nullptr, nullptr, out);
}

// ---- per-part options ----

ptts_part_opts part_opts_known(const ptts_part_opts* po, int32_t i) {
    ptts_part_opts k;
    std::memset(&k, 0, sizeof k);
    const ptts_part_opts& e = part_opts_at(po, i);
    std::memcpy(&k, &e, std::min<size_t>(e.size, sizeof k));
    return k;
}

std::string part_seam_error(const char* what, double gap_ms, double crossfade_ms, const JoinLens& dflt, JoinLens* out) {
    if (std::isnan(gap_ms)) return strfmt("join: parts: %s: gap_ms is NaN", what);
    if (std::isnan(crossfade_ms)) return strfmt("join: parts: %s: crossfade_ms is NaN", what);
    if (gap_ms < 0.0 && crossfade_ms < 0.0) {   // the pair of the join options
        if (out) *out = dflt;
        return std::string();
    }
    const double g = gap_ms < 0.0 ? 0.0 : gap_ms, c = crossfade_ms < 0.0 ? 0.0 : crossfade_ms;
    std::string e;
    const std::string stage = std::string("join: parts: ") + what;
    if (range_error(stage.c_str(), "gap_ms", g, 0.0, kJoinMaxMs, e)) return e;
    if (range_error(stage.c_str(), "crossfade_ms", c, 0.0, kJoinMaxMs, e)) return e;
    if (g > 0.0 && c > 0.0) return strfmt("join: parts: %s: gap_ms %g and crossfade_ms %g are both set, at most one of them may be above 0", what, g, c);
    if (out) *out = JoinLens{ms_samples(g), ms_samples(c)};
    return std::string();
}

std::string join_parts_error(const ptts_part_opts* po, int32_t rows, const JoinLens& dflt, JoinSeams* seams, std::vector<PartVolume>* vol) {
    if (rows < 1 || rows > kJoinMaxRows) return strfmt("join: rows %d is not from 1 to %d", rows, kJoinMaxRows);
    if (!po) return "join: parts: null list";
    constexpr size_t kKnown = sizeof(ptts_part_opts);
    if (seams) seams->lens.assign((size_t)rows, JoinLens{});
    if (vol) vol->assign((size_t)rows, PartVolume{});
    if (po->size < kKnown) return strfmt("join: parts: part 0: size %u is smaller than the fields up to crossfade_ms (%zu bytes)", po->size, kKnown);
    for (int32_t i = 0; i < rows; i++) {
        const ptts_part_opts& e = part_opts_at(po, i);
        const std::string what = strfmt("part %d", i);
        if (e.size != po->size) return strfmt("join: parts: %s: size %u differs from part 0's %u, the elements of a list lie `size` bytes apart", what.c_str(), e.size, po->size);
        std::string err = opts_size_error(("join: parts: " + what).c_str(), &e, e.size, kKnown, kKnown, "the fields up to crossfade_ms");
        if (!err.empty()) return err;
        err = part_seam_error(what.c_str(), e.gap_ms, e.crossfade_ms, dflt, seams ? &seams->lens[(size_t)i] : nullptr);
        if (!err.empty()) return err;
        if (!vol) continue;
        PartVolume& v = (*vol)[(size_t)i];
        if (range_error(("join: parts: " + what).c_str(), "gain_db", e.gain_db, kPartMinGainDb, kPartMaxGainDb, err)) return err;
        if (e.level && (e.level < kPartMinLevel || e.level > kPartMaxLevel))
            return strfmt("join: parts: %s: level %d is not 0 (off) or a target from %d to %d (0.01 LUFS)", what.c_str(), e.level, kPartMinLevel, kPartMaxLevel);
        if (e.level && e.gain_db != 0.0)
            return strfmt("join: parts: %s: level %d and gain_db %g are both set (one gain)", what.c_str(), e.level, e.gain_db);
        if (e.gain_db != 0.0) { v.fixed = true; v.g = (float)std::pow(10.0, e.gain_db / 20.0); }
        else if (e.level) { v.level = true; v.target_lufs = (double)e.level / 100.0; }
    }
    return std::string();
}

std::string join_parts_plan(const int64_t* n, int32_t rows, const JoinSeams& s, int64_t* offsets, int64_t* seams, int64_t* total) {
    return plan_with(n, rows, [&](int32_t i) { return s.lens[(size_t)i - 1]; }, offsets, seams, total);
}

void join_parts_host(const float* const* in, const int64_t* n, int32_t rows, const JoinSeams& s, const float* g, const bool* apply, float* out) {
    join_with(in, n, rows, [&](int32_t i) { return s.lens[(size_t)i - 1]; }, g, apply, out);
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

int64_t ptts_join_parts_length(const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, int64_t* offsets) {
    JoinLens l;
    JoinSeams seams;
    std::string e = join_opts_error(o, &l);
    if (e.empty()) e = join_parts_error(po, rows, l, &seams, nullptr);
    int64_t total = 0;
    if (e.empty()) e = join_parts_plan(n, rows, seams, offsets, nullptr, &total);
    if (!e.empty()) return -(int64_t)fail(e);
    return total;
}

int64_t ptts_join_parts_stream_ready(const ptts_join_opts* o, const ptts_part_opts* last, int64_t joined) {
    JoinLens l;
    JoinSeams seams;
    std::string e = join_opts_error(o, &l);
    if (e.empty() && !last) e = "join: parts: null list";
    if (e.empty()) e = join_parts_error(last, 1, l, &seams, nullptr);
    if (e.empty() && joined < 0) e = strfmt("join: stream: joined %lld is negative", (long long)joined);
    if (!e.empty()) return -(int64_t)fail(e);
    return join_stream_ready(joined, join_stream_hold(*o, seams.lens[0]));
}

}  // extern "C"

int ptts::join_parts_run(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, float* out, float* gains,
                         PartLevelGain level_gain) {
    JoinLens l;
    JoinSeams seams;
    std::vector<PartVolume> vol;
    std::string e = join_opts_error(o, &l);
    if (e.empty()) e = join_parts_error(po, rows, l, &seams, &vol);
    int64_t total = 0;
    if (e.empty()) e = join_parts_plan(n, rows, seams, nullptr, nullptr, &total);
    if (!e.empty()) return fail(e);
    if (!in || (!out && total > 0)) return fail("join: null argument");
    for (int32_t i = 0; i < rows; i++)
        if (!in[i] && n[i] > 0) return fail(strfmt("join: part %d is null", i));
    std::vector<float> g((size_t)rows, 1.0f);
    std::unique_ptr<bool[]> apply(new bool[(size_t)rows]);
    for (int32_t i = 0; i < rows; i++) {
        const PartVolume& v = vol[(size_t)i];
        if (v.level && n[i] > 0) g[(size_t)i] = level_gain(in[i], n[i], v.target_lufs);   // ptts_loudness_normalize's
        else if (v.fixed) g[(size_t)i] = v.g;
        apply[(size_t)i] = v.fixed || (v.level && g[(size_t)i] != 1.0f);
        if (gains) gains[i] = g[(size_t)i];
    }
    join_parts_host(in, n, rows, seams, g.data(), apply.get(), out);
    return PTTS_OK;
}
