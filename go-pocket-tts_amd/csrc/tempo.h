// tempo.h -- the speaking rate of one part of a joined text (include/ptts.h ptts_tempo_opts, ptts_tempo_*): a
// time-scale change that keeps the pitch, by overlap-add of hops whose read positions a waveform-similarity search chooses, written once for
// the host (tempo.cpp is the statement) and the device (tempo.hip).  No HIP header: tempo.cpp builds with a plain C++ compiler.
//
// On the 24 kHz row x[0, n), n below kTempoMaxSamples, with s = speed_permille (500 .. 2000), the hop Hs = 480 and the search radius D = 240;
// every index is an integer, a sample outside [0, n) reads as 0.0f and its quantised value as 0:
//     n_out = (n * 1000) / s (int64, integer division), F = ceil(n_out / Hs) hops; n == 0 or n_out == 0: an empty row.
//     q[i] = 0 for a NaN, else (int32)(clamp(x[i], -1, 1) * 32767.0f), truncated towards zero (the PCM16 egress's value; infinities clamp).
//     p_0 = 0; for hop k >= 1: a_k = (k * Hs * s) / 1000 is where the input should be read, c_k = p_(k-1) + Hs where the previous hop's
//     segment continues, S(d) = sum over j in [0, Hs) of |q[a_k + d + j] - q[c_k + j]| for d in [-D, D] (at most 480 * 65534: an int32),
//     d* minimises (S(d), |d|, d > 0) lexicographically -- the least S, then the least |d|, then the negative one -- and p_k = a_k + d*.
//     out[m], m in [0, n_out), k = m / Hs, j = m % Hs:  k == 0 or p_k == c_k (the hop continues its predecessor): x[p_k + j], moved as its 32
//     bits; else x[c_k + j] * ((float)(Hs - j) / (float)Hs) + x[p_k + j] * ((float)j / (float)Hs): two f32 divisions, two f32 products, one
//     f32 sum, each rounded once, nothing fused.
// Every decision is integer arithmetic (the quantisation is one f32 product and a truncation of exactly representable steps), so the host and
// the device cannot disagree by a rounding; the blend is the join's seam arithmetic (join.hip).
//   - s == 1000 returns the row bit for bit: d = 0 has S = 0 and the least |d|, so every hop continues.
//   - the continuation, whenever it lies inside the search window, has S = 0, the least there is: it wins unless a lag nearer to a_k is a
//     perfect match too (silence, an exactly periodic stretch), so stretches of the input pass through untouched between splices.
//   - the last hop of a slowed row may fade into the zeros behind n.
//   - audio above +-1 is clamped in the search only, never in the output.
//   - a_k <= n - 1 (k * Hs <= n_out - 1 and n_out * s <= n * 1000), so p_k <= n + D - 1: with n below kTempoMaxSamples a position is an int32.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ptts.h"
#include "scan_block.h"

namespace ptts {

std::string strfmt(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // (common.h's, restated: this header includes no HIP header)
void set_last_error(const std::string& m);

constexpr int kTempoHop = 480;       // Hs: 20 ms
constexpr int kTempoRadius = 240;    // D: +-10 ms
constexpr int kTempoLags = 2 * kTempoRadius + 1;
constexpr int kTempoWindow = 2 * kTempoRadius + kTempoHop;   // the samples a hop's search reads around a_k: [a_k - D, a_k + D + Hs)
constexpr int64_t kTempoMaxSamples = ((int64_t)1 << 31) - kTempoRadius;   // a row stays below it: a position fits an int32

// A designed tempo (tempo.cpp tempo_design): it travels to the device as it is, behind a table's rows (dsp_device.cpp)
struct TempoScan {
    int32_t speed;     // speed_permille, 500 .. 2000
    int32_t pad[3];
};

// the quantised view of a sample: the PCM16 egress's value; a NaN is 0
PTTS_HD inline int32_t tempo_quant(float x) {
    if (x != x) return 0;
    const float c = x < -1.0f ? -1.0f : x > 1.0f ? 1.0f : x;
    return (int32_t)(c * 32767.0f);
}
// where hop k should read the input
PTTS_HD inline int64_t tempo_target(int64_t k, int32_t speed) { return (k * kTempoHop * (int64_t)speed) / 1000; }
// the samples of the time-scaled row; monotone in n
PTTS_HD inline int64_t tempo_length(int64_t n, int32_t speed) { return n > 0 ? (n * 1000) / (int64_t)speed : 0; }
PTTS_HD inline int64_t tempo_hops(int64_t n_out) { return (n_out + kTempoHop - 1) / kTempoHop; }
// the key of lag d with the sum S, least first: (S, |d|, d > 0) in one word (S takes 25 bits, |d| 8)
PTTS_HD inline uint64_t tempo_key(int32_t S, int32_t d) {
    return (uint64_t)(uint32_t)S << 9 | (uint64_t)(uint32_t)(d < 0 ? -d : d) << 1 | (uint64_t)(d > 0 ? 1 : 0);
}
PTTS_HD inline int32_t tempo_key_lag(uint64_t key) {
    const int32_t a = (int32_t)(key >> 1 & 255u);
    return key & 1u ? a : -a;
}
// the blend's weights at sample j of a hop: the predecessor's continuation fades out, the new segment in
PTTS_HD inline float tempo_w_out(int j) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)(kTempoHop - j), (float)kTempoHop);
#else
    return (float)(kTempoHop - j) / (float)kTempoHop;
#endif
}
PTTS_HD inline float tempo_w_in(int j) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)j, (float)kTempoHop);
#else
    return (float)j / (float)kTempoHop;
#endif
}

// ---- the host side (tempo.cpp) ----
// empty: the caller's options are well formed (the size rules of ptts_dsp_ext_opts, speed_permille in its range, reserved 0); otherwise the
// message, naming the field
std::string tempo_opts_error(const ptts_tempo_opts* t);
// the design of well-formed options
TempoScan tempo_design(const ptts_tempo_opts& t);
// the positions p[0, F) of x[0, n)'s hops, F = tempo_hops(tempo_length(n, speed))
void tempo_plan_host(const TempoScan& d, const float* x, int64_t n, int32_t* p);
// ... and the row itself into out (holds tempo_length(n, speed) floats; not x)
void tempo_apply_host(const TempoScan& d, const float* x, int64_t n, float* out);

}  // namespace ptts
