// trim.h -- silence control of one part of a joined text (include/ptts.h ptts_trim_opts, ptts_trim_*): the row's silent
// head and tail cut off and its over-long pauses capped, written once for the host (trim.cpp is the statement) and the device (trim.hip).  No HIP
// header: trim.cpp builds with a plain C++ compiler.
//
// On the 24 kHz row x[0, n), with t the linear threshold, H the pad and M the longest pause that stays, both in samples:
//     a sample is LOUD when fabsf(x) > t: a NaN never is, an infinity is, |x| == t is not.  L is the ascending set of loud indices.
//     L empty: the row comes back whole -- lo = 0, hi = n, n_out = n, cuts = 0, speech = 0.
//     otherwise speech = 1 and, with `edges`, lo = max(0, L.first - H), hi = min(n, L.last + 1 + H); without, lo = 0 and hi = n.
//     M > 0: consecutive loud indices u < v with q = v - u - 1 > M lose the samples [u + 1 + (M - M / 2), v - M / 2) (integer division): the
//            first ceil(M / 2) and the last floor(M / 2) samples of the pause stay, q - M go.  cuts counts such pairs.
//     every sample of [lo, hi) that is not removed is output, in order, moved as its 32 bits: n_out = hi - lo - sum(q - M).
// Everything is an integer comparison on indices, plus one float comparison per sample against t: the host and the device cannot disagree by a
// rounding.  A cut lies between two loud samples, so inside [L.first, L.last] and with it inside [lo, hi).
//
// The device form decides a quiet sample i from the two loud indices around it alone (trim_keep): u the last loud index in front of i, v the
// first one behind it.  A tile records its own first and last loud index and what its inner pauses lose (k_trim_mark); one workgroup per row
// carries "the last loud index in front of tile f" forward and "the first one behind it" backward, and from the two computes what every tile
// keeps -- the part of a tile-crossing cut that falls into a tile is the overlap of two intervals (trim_cut_in) -- and the exclusive prefix of
// those counts (k_trim_carry); every tile then stores what it keeps at its offset (k_trim_store).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ptts.h"
#include "scan_block.h"

namespace ptts {

std::string strfmt(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // (common.h's, restated: this header includes no HIP header)
void set_last_error(const std::string& m);

// A designed trim (trim.cpp trim_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct TrimScan {
    float t;           // the linear threshold, (float)pow(10, threshold_db / 20)
    int32_t edges;     // 0 or 1
    int64_t H;         // the pad, (int64)(pad_ms / 1000 * 24000)
    int64_t M;         // the longest pause that stays, (int64)(max_pause_ms / 1000 * 24000); 0: pauses untouched
    int64_t pad;
};

constexpr int32_t kTrimNone = -1;                // no loud sample in front
constexpr int32_t kTrimNoneBehind = INT32_MAX;   // no loud sample behind: never an index, a row has fewer than 2^31 samples
constexpr int64_t kTrimMaxSamples = (int64_t)1 << 31;

PTTS_HD inline bool trim_loud(float x, float t) { return __builtin_fabsf(x) > t; }

// [a, b): what the pause between the loud indices u < v loses; empty (a == b == 0) when either is missing or the pause is no longer than M
PTTS_HD inline void trim_cut(int64_t u, int64_t v, int64_t M, int64_t* a, int64_t* b) {
    *a = *b = 0;
    if (M <= 0 || u < 0 || v == kTrimNoneBehind || v - u - 1 <= M) return;
    *a = u + 1 + (M - M / 2);
    *b = v - M / 2;
}
// how many of those samples lie in [A, B)
PTTS_HD inline int64_t trim_cut_in(int64_t u, int64_t v, int64_t M, int64_t A, int64_t B) {
    int64_t a, b;
    trim_cut(u, v, M, &a, &b);
    const int64_t lo = a > A ? a : A, hi = b < B ? b : B;
    return hi > lo ? hi - lo : 0;
}
// whether the quiet sample i of a row with speech is output: u, v the loud indices around it (kTrimNone, kTrimNoneBehind: none)
PTTS_HD inline bool trim_keep(int64_t i, int64_t u, int64_t v, int64_t M, int64_t lo, int64_t hi) {
    if (i < lo || i >= hi) return false;
    int64_t a, b;
    trim_cut(u, v, M, &a, &b);
    return !(i >= a && i < b);
}

// ---- the host side (trim.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, every field in its range, something switched on); otherwise
// the message, naming the field
std::string trim_opts_error(const ptts_trim_opts* t);
// the design of well-formed options
TrimScan trim_design(const ptts_trim_opts& t);
// what the trim makes of x[0, n)
void trim_plan_host(const TrimScan& d, const float* x, int64_t n, ptts_trim_info* info);
// ... and the row itself into out (holds n floats; may be x)
void trim_apply_host(const TrimScan& d, const float* x, int64_t n, float* out, ptts_trim_info* info);

}  // namespace ptts
