// dsp_spec.cpp -- a ptts_dsp_opts resolved into a DspSpec (dsp_spec.h).  No HIP header.
#include "dsp_spec.h"

namespace ptts {

std::string dsp_resolve(const ptts_dsp_opts* o, DspSpec* out) {
    *out = DspSpec();
    if (!o) return std::string();
    if (std::isnan(o->fade_in_ms) || o->fade_in_ms < 0) return strfmt("dsp: fade_in_ms %g is negative or not a number", o->fade_in_ms);
    if (std::isnan(o->fade_out_ms) || o->fade_out_ms < 0) return strfmt("dsp: fade_out_ms %g is negative or not a number", o->fade_out_ms);
    if (o->eq && !(out->eq = eq_lookup(o->eq))) return strfmt("dsp: eq %p is not a live handle of ptts_eq_create", (const void*)o->eq);
    DspExt ext;   // (no reserved word is left to check: whatever lies in reserved[2..3] is a handle the registry knows, or refused unread)
    if (o->ext && !ext_lookup(o->ext, &ext)) return strfmt("dsp: ext %p (reserved[2..3]) is not a live handle of ptts_dsp_ext_create", (const void*)o->ext);
    out->normalize = o->normalize != 0;
    out->dc_block = o->dc_block != 0;
    out->fade_in_ms = o->fade_in_ms;
    out->fade_out_ms = o->fade_out_ms;
    out->true_peak = ext.true_peak;
    out->ceiling = ext.ceiling;
    out->compress = ext.compress;
    out->cmp = ext.cmp;
    out->deess = ext.deess;
    out->des = ext.des;
    out->limit = ext.limit;
    out->lim = ext.lim;
    out->trim = ext.trim;
    out->trm = ext.trm;
    out->tempo = ext.tempo;
    out->tmp = ext.tmp;
    out->pitch = ext.pitch;
    out->pit = ext.pit;
    out->formant = ext.formant && ext.fmt.keep != 0;
    return std::string();
}

bool dsp_active(const ptts_dsp_opts* o) {
    DspExt ext;
    return o && (o->normalize || o->dc_block || o->fade_in_ms > 0 || o->fade_out_ms > 0 || o->eq || (o->ext && ext_lookup(o->ext, &ext) && (ext.true_peak || ext.compress || ext.deess || ext.limit)));
}

}  // namespace ptts
