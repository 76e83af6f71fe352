// dsp_spec.h -- what one row of the post-processing chain gets, as a plain value: a ptts_dsp_opts with its handles looked
// up, plus the row's loudness; and the scratch such a row's stages need on the device (dsp_scratch).  dsp_spec.cpp is the only code that reads a ptts_dsp_opts; like eq.cpp it builds with a plain C++ compiler (no HIP header).
#pragma once
#include "dsp_ext.h"
#include "true_peak.h"

namespace ptts {

struct DspSpec {
    bool normalize = false, dc_block = false;
    double fade_in_ms = 0.0, fade_out_ms = 0.0;        // <= 0: none
    const EqScan* eq = nullptr;                        // a live handle's system (borrowed for the call), or null
    bool true_peak = false; float ceiling = 1.0f;      // measured and held at or under `ceiling` (linear)
    bool loud = false; double target_power = 0.0;      // measured (BS.1770) on the samples as the compressor leaves them; 10^((target LUFS + 0.691) / 10) is what its gain aims at
    bool compress = false; CmpScan cmp{};              // the first stage (compressor.h): everything above is measured and applied behind it
    bool deess = false; DeScan des{};                  // the de-esser (deesser.h): directly behind the compressor; "behind it" above means behind the pair
    bool limit = false; LimScan lim{};                 // the limiter (limiter.h): behind the fades, in front of the true-peak ceiling
    bool trim = false; TrimScan trm{};                 // the trim of a joined call's parts (trim.h): no stage of the chain, neither rest() nor any() counts it
    bool tempo = false; TempoScan tmp{};               // the tempo of a joined call's parts (tempo.h), behind the trim: no stage of the chain either
    bool pitch = false; PitchScan pit{};               // the pitch of a joined call's parts (pitch.h), between the trim and the tempo: no stage of the chain either
    bool formant = false;                              // keep the formants around that pitch (formant.h): set with keep == 1 alone; without a pitch it says nothing
    bool rest() const { return normalize || dc_block || fade_in_ms > 0 || fade_out_ms > 0 || eq || true_peak || loud || limit; }   // the chain behind the compressor and the de-esser
    bool any() const { return compress || deess || rest(); }
};

// The scratch plan: the doubles of WORK_DSP_SCRATCH each stage of a row of n samples needs (dsp_device.cpp sizes the buffer by total() and carves
// it by the fields, and nothing else decides either).  apply false: a measurement alone, which rewrites nothing -- no compressor, equaliser or limiter
struct DspScratch {
    size_t cmp = 0;    // the compressor's per-tile states of both recurrences (compressor.h cmp_state_doubles)
    size_t dc = 0;     // the DC block's per-tile states (scan_block.h scan_state_doubles)
    size_t loud = 0;   // the loudness block: M, the gain, the K-weighting's per-tile states, the sub-block energies (scan_block.h loud_doubles)
    size_t eq = 0;     // the equaliser's per-tile states, 2 S doubles each for E_f and S_f
    size_t lim = 0;    // the limiter's per-tile states, then its gains, one f32 a sample (limiter.h lim_scratch_doubles)
    size_t de = 0;     // the de-esser's per-tile states: the side chain's, the detector's, the smoothing's (deesser.h de_state_doubles)
    size_t total() const { return cmp + dc + loud + eq + lim + de; }
    // where each region starts within the row's total(): one behind the other, in the order above
    size_t cmp_at() const { return 0; }
    size_t dc_at() const { return cmp; }
    size_t loud_at() const { return dc_at() + dc; }
    size_t eq_at() const { return loud_at() + loud; }
    size_t lim_at() const { return eq_at() + eq; }
    size_t de_at() const { return lim_at() + lim; }
};
inline DspScratch dsp_scratch(const DspSpec& sp, int64_t n, bool apply) {
    DspScratch q;
    if (n <= 0) return q;
    const int64_t F = scan_tiles(n);
    if (sp.compress && apply) q.cmp = cmp_state_doubles(F);
    if (sp.dc_block) q.dc = scan_state_doubles<DspScan::N>(F);
    if (sp.loud) q.loud = loud_doubles(F);
    if (sp.eq && apply) q.eq = (size_t)F * 4 * (size_t)sp.eq->S;
    if (sp.limit && apply) q.lim = lim_scratch_doubles(n);
    if (sp.deess && apply) q.de = de_state_doubles(F);
    return q;
}

// o (NULL: nothing) with its handles looked up, into *out.  Empty: fine.  Otherwise the message of the first bad field -- a fade that is negative
// or not a number, an eq or ext that is not a live handle (looked up by address, never read) -- and *out is not to be used.
std::string dsp_resolve(const ptts_dsp_opts* o, DspSpec* out);
inline std::string dsp_opts_error(const ptts_dsp_opts& o) { DspSpec spec; return dsp_resolve(&o, &spec); }
// Where a row's length is fixed before the decode (a request's own dsp, ptts_dsp_rows) a resolved spec with a trim is refused: the message, or empty
inline std::string dsp_trim_refusal(const DspSpec& s) {
    return s.trim ? std::string("dsp: ext: trim changes a row's length; it is served by ptts_generate_joined and ptts_trim_rows") : std::string();
}
// ... and one with a tempo, likewise
inline std::string dsp_tempo_refusal(const DspSpec& s) {
    return s.tempo ? std::string("dsp: ext: tempo changes a row's length; it is served by ptts_generate_joined and ptts_tempo_rows") : std::string();
}
// Where a row is handed over window after window (a joined call with a pcm_callback, ptts_debug_dsp_windows) only the causal stages run: the
// compressor, the DC block, the equaliser and the fades.  The message naming the first stage of s that is none, or empty.  The de-esser is causal
// too, but its states are not carried from window to window yet: it is refused last, in words of its own
inline std::string dsp_window_refusal(const DspSpec& s) {
    const char* f = s.normalize ? "normalize" : s.loud ? "loudness" : s.true_peak ? "ext: true_peak" : nullptr;
    if (f) return strfmt("stream: %s needs the whole text; it cannot be combined with pcm_callback", f);
    if (s.limit) return std::string("stream: ext: limiter looks ahead of the samples it hands over; it cannot be combined with pcm_callback yet");
    return s.deess ? std::string("stream: ext: deesser is not carried from window to window yet; it cannot be combined with pcm_callback yet") : std::string();
}
// ... and one with a pitch, likewise
inline std::string dsp_pitch_refusal(const DspSpec& s) {
    return s.pitch ? std::string("dsp: ext: pitch changes a row's length; it is served by ptts_generate_joined and ptts_pitch_rows") : std::string();
}
// whether o switches anything on, without an error: what dsp_resolve's spec says with any(), except that an eq counts unseen (so a dead one is
// active, and refused where the row is resolved) and an ext that is not live counts for nothing.  One registry look-up at the most: it is
// asked per request before the decode and per streamed hand-over
bool dsp_active(const ptts_dsp_opts* o);

}  // namespace ptts
