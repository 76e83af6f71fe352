// dsp_spec.h -- what one row of the post-processing chain gets, as a plain value: a ptts_dsp_opts with its handles looked
// up, plus the row's loudness.  dsp_spec.cpp is the only code that reads a ptts_dsp_opts; like eq.cpp it builds with a plain C++ compiler (no HIP header).
#pragma once
#include "true_peak.h"

namespace ptts {

struct DspSpec {
    bool normalize = false, dc_block = false;
    double fade_in_ms = 0.0, fade_out_ms = 0.0;        // <= 0: none
    const EqScan* eq = nullptr;                        // a live handle's system (borrowed for the call), or null
    bool true_peak = false; float ceiling = 1.0f;      // measured and held at or under `ceiling` (linear)
    bool loud = false; double target_power = 0.0;      // measured (BS.1770) on the samples as the compressor leaves them; 10^((target LUFS + 0.691) / 10) is what its gain aims at
    bool compress = false; CmpScan cmp{};              // the first stage (compressor.h): everything above is measured and applied behind it
    bool limit = false; LimScan lim{};                 // the limiter (limiter.h): behind the fades, in front of the true-peak ceiling
    bool rest() const { return normalize || dc_block || fade_in_ms > 0 || fade_out_ms > 0 || eq || true_peak || loud || limit; }   // the chain behind the compressor
    bool any() const { return compress || rest(); }
};

// o (NULL: nothing) with its handles looked up, into *out.  Empty: fine.  Otherwise the message of the first bad field -- a fade that is negative
// or not a number, an eq or ext that is not a live handle (looked up by address, never read) -- and *out is not to be used.
std::string dsp_resolve(const ptts_dsp_opts* o, DspSpec* out);
inline std::string dsp_opts_error(const ptts_dsp_opts& o) { DspSpec spec; return dsp_resolve(&o, &spec); }
// whether o switches anything on, without an error: what dsp_resolve's spec says with any(), except that an eq counts unseen (so a dead one is
// active, and refused where the row is resolved) and an ext that is not live counts for nothing.  One registry look-up at the most: it is
// asked per request before the decode and per streamed hand-over
bool dsp_active(const ptts_dsp_opts* o);

}  // namespace ptts
