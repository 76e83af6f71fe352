// join.h -- a text's parts joined into one utterance (include/ptts.h ptts_join_opts; join.cpp is the host statement, join.hip the device form;
// DESIGN.md section 8, N3): the lengths, the seams and the part offsets, shared by ptts_join, ptts_join_rows and ptts_generate_joined.  No HIP
// header: a plain compiler builds join.cpp (tests/test_join_cpu.py does, with sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ptts.h"

namespace ptts {

std::string strfmt(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // (common.h's, restated: this header includes no HIP header)
void set_last_error(const std::string& m);

constexpr int32_t kJoinMaxRows = 4096;
constexpr int64_t kJoinMaxSamples = (int64_t)1 << 31;   // the joined length stays below it
constexpr double kJoinMaxMs = 2000.0;
constexpr int kJoinRate = 24000;

// the gap and the crossfade in samples, (int64)(ms / 1000 * 24000) as dsp_fade_in counts a fade; at most one of them is not 0
struct JoinLens { int64_t gap = 0, xfade = 0; };

// empty: o is well formed as far as the join goes (the size rules of ptts_dsp_ext_opts, gap_ms and crossfade_ms finite values from 0 to 2000,
// not both above 0), and *out has the two lengths; otherwise the message, naming the field.  The egress fields and `dsp` are the device call's
// to check (generate.cpp join_egress_error)
std::string join_opts_error(const ptts_join_opts* o, JoinLens* out);

// Streamed joined synthesis (include/ptts.h ptts_join_stream_opts).  Empty: so is well formed as far as the host can tell (there, its size by the
// rules of ptts_dsp_ext_opts, first_group not negative; the upper end is the model's max_batch, the device call's to check)
std::string join_stream_opts_error(const ptts_join_stream_opts* so);
// what a hand-over holds back behind the joined length: max(K, Fo), the crossfade and the fade out of o.dsp (a plain read, no handle is looked up)
int64_t join_stream_hold(const ptts_join_opts& o, const JoinLens& l);
// the samples that are final once `joined` have been joined and more parts follow: on the grid of the chain's scans (1920: kDspTile)
constexpr int64_t kJoinStreamGrid = 1920;
inline int64_t join_stream_ready(int64_t joined, int64_t hold) { return std::max<int64_t>(0, joined - hold) / kJoinStreamGrid * kJoinStreamGrid; }

// samples of the seam between a part of na samples and its successor of nb: two seams never touch the same sample
inline int64_t join_seam(int64_t xfade, int64_t na, int64_t nb) { return std::min(xfade, std::min(na / 2, nb / 2)); }

// offsets[i] (optional): where part i's first sample lies in the joined audio; seams[i] (optional): the samples of the seam in front of part i
// (seams[0] = 0); *total: the joined length.  Empty, or the message naming the limit that was broken
std::string join_plan(const int64_t* n, int32_t rows, const JoinLens& l, int64_t* offsets, int64_t* seams, int64_t* total);

// the joined audio of in[0 .. rows) into out[0, total): every sample written once
void join_host(const float* const* in, const int64_t* n, int32_t rows, const JoinLens& l, float* out);

// ---- per-part options (include/ptts.h ptts_part_opts): a seam of its own behind every part, a volume per part ----

constexpr double kPartMinGainDb = -60.0, kPartMaxGainDb = 24.0;
constexpr int32_t kPartMinLevel = -7000, kPartMaxLevel = -100;

// element i of a caller's list: its elements lie po[0].size bytes apart (join_parts_error has checked the sizes)
inline const ptts_part_opts& part_opts_at(const ptts_part_opts* po, int32_t i) {
    return *reinterpret_cast<const ptts_part_opts*>(reinterpret_cast<const char*>(po) + (size_t)i * po->size);
}
// the bytes of an element that this library knows, the rest read as 0
ptts_part_opts part_opts_known(const ptts_part_opts* po, int32_t i);

// the seams of a list: lens[i] is the seam BEHIND part i, in samples ([rows]; the last one is unused)
struct JoinSeams { std::vector<JoinLens> lens; };
// A part's volume, resolved: a fixed gain is applied to every sample (apply), a level's is measured -- on the host by a PartLevelGain, on the
// device by the loudness rows' kernels -- and applied where it is not 1
struct PartVolume { float g = 1.0f; bool fixed = false; double target_lufs = 0.0; bool level = false; };
// the gain ptts_loudness_normalize(x, n, target_lufs, NULL) applies (loudness.cpp measures it: this file and join.cpp build without it)
using PartLevelGain = float (*)(const float* x, int64_t n, double target_lufs);

// empty: the list is well formed as far as the host join goes, *seams (optional) has the seams resolved against dflt (the pair of the join options)
// and *vol (optional: the volume fields are then not read) the volumes; otherwise the message, naming the field and the part index
std::string join_parts_error(const ptts_part_opts* po, int32_t rows, const JoinLens& dflt, JoinSeams* seams, std::vector<PartVolume>* vol);
// one seam's pair against dflt: the rule of the list; what: "part 3" in the message
std::string part_seam_error(const char* what, double gap_ms, double crossfade_ms, const JoinLens& dflt, JoinLens* out);
// join_plan with a seam of its own behind every part
std::string join_parts_plan(const int64_t* n, int32_t rows, const JoinSeams& s, int64_t* offsets, int64_t* seams, int64_t* total);
// join_host with the seams of the list and the parts' gains: g[i] multiplies every sample of part i where apply[i] is set (one f32 product, in
// front of the seam arithmetic), the other parts move as their bits
void join_parts_host(const float* const* in, const int64_t* n, int32_t rows, const JoinSeams& s, const float* g, const bool* apply, float* out);
// ptts_join_parts (capi_rows.cpp hands in loudness.cpp's measurement): the checks, the parts' gains, join_parts_host.  PTTS_OK, or PTTS_EINVAL with the message set
int join_parts_run(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, float* out, float* gains,
                   PartLevelGain level_gain);

}  // namespace ptts
