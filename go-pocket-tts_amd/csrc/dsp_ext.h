// dsp_ext.h -- the handle behind ptts_dsp_opts.ext (include/ptts.h ptts_dsp_ext): what true_peak.cpp (which makes and
// frees it), compressor.cpp, deesser.cpp and limiter.cpp (which set its compressor, its de-esser and its limiter), capi_rows.cpp (which sets its trim, its tempo, its pitch and its formant option) and
// dsp_spec.cpp (which reads it) share, and the one setter behind the seven ptts_dsp_ext_set_*.  No HIP header.
#pragma once
#include "compressor.h"
#include "deesser.h"
#include "eq.h"
#include "formant.h"
#include "limiter.h"
#include "opts_check.h"
#include "pitch.h"
#include "tempo.h"
#include "trim.h"

namespace ptts {

// what a live ptts_dsp_ext says, by value (false: e is NULL or not live, and e is not read): the ceiling, the compressor that
// ptts_dsp_ext_set_compressor attached (compressor.cpp), the de-esser that ptts_dsp_ext_set_deesser attached (deesser.cpp) and the limiter that
// ptts_dsp_ext_set_limiter attached (limiter.cpp), all as designed.
// The trim that ptts_dsp_ext_set_trim attached (trim.h: t, H, M, edges) is no stage of the chain: ptts_generate_joined serves it per part in
// front of the join, and whatever fixes a row's length before the decode refuses it (dsp_spec.h dsp_trim_refusal).
// The tempo that ptts_dsp_ext_set_tempo attached (tempo.h: the speed) is served and refused like the trim, behind it (dsp_spec.h dsp_tempo_refusal).
// The pitch that ptts_dsp_ext_set_pitch attached (pitch.h: p, D, g) likewise, between the trim and the tempo (dsp_spec.h dsp_pitch_refusal).
// The option that ptts_dsp_ext_set_formant attached (formant.h: keep) goes with the pitch: it changes how the resampling step runs, nothing else.
// Copied out under the registry's mutex, which the setters take too
struct DspExt { bool true_peak = false; float ceiling = 1.0f; bool compress = false; CmpScan cmp{}; bool limit = false; LimScan lim{}; bool deess = false; DeScan des{}; bool trim = false; TrimScan trm{}; bool tempo = false; TempoScan tmp{}; bool pitch = false; PitchScan pit{}; bool formant = false; FormantScan fmt{}; };
bool ext_lookup(const ptts_dsp_ext* e, DspExt* out);

}  // namespace ptts

struct ptts_dsp_ext { ptts::DspExt v; };

namespace ptts {

// Every ptts_dsp_ext_set_<stage>: the options checked by the stage's *_opts_error (null options: the stage off), the design made outside the
// registry's mutex, then the flag and the design stored under it; a handle that is not live is refused under the stage's name.  The callers are
// compressor.cpp, deesser.cpp and limiter.cpp for their own stage, and capi_rows.cpp for the trim, the tempo and the pitch, whose files build alone without the registry
template <class Opts, class Design>
int ext_set(ptts_dsp_ext* e, const char* stage, const Opts* o, std::string (*opts_error)(const Opts*), Design (*design)(const Opts&), bool DspExt::*on,
            Design DspExt::*d) {
    bool flag = false;
    Design made{};
    if (o) {
        const std::string err = opts_error(o);
        if (!err.empty()) return fail(err);
        flag = true;
        made = design(*o);
    }
    if (!handle_with(e, HANDLE_DSP_EXT, [&] { e->v.*on = flag; e->v.*d = made; }))
        return fail(strfmt("%s: ext %p is not a live handle of ptts_dsp_ext_create", stage, (const void*)e));
    return PTTS_OK;
}

}  // namespace ptts
