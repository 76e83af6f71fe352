// join.h -- a text's parts joined into one utterance (include/ptts.h ptts_join_opts; join.cpp is the host statement, join.hip the device form;
// DESIGN.md section 8, N3): the lengths, the seams and the part offsets, shared by ptts_join, ptts_join_rows and ptts_generate_joined.  No HIP
// header: a plain compiler builds join.cpp (tests/test_join_cpu.py does, with sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

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

}  // namespace ptts
