// capi_rows.cpp -- extern "C": the entry points on rows of host samples: resample, the chain's stages and a joined call's part stages on host rows, the
// ptts_dsp_ext_set_* of the part stages, join rows, loudness, true peak, PCM encoding and the WAV headers.  Each checks its arguments under its own name
// and forwards to the engine's round trip (dsp_rows_device, part_rows_device, join_rows_device, staged_convert).
#include "capi_internal.h"
#include "eq.h"

using namespace ptts;
using namespace ptts::capi;

extern "C" {

int64_t ptts_resample_length(int64_t n_in, int32_t in_rate, int32_t out_rate) {
    const std::string e = rate_pair_error(in_rate, out_rate);
    if (!e.empty()) { set_last_error(e); return -PTTS_EINVAL; }
    if (n_in < 0) { set_last_error(strfmt("ptts-hip: resample: negative sample count %lld", (long long)n_in)); return -PTTS_EINVAL; }
    return resample_length(n_in, in_rate, out_rate);
}

// the argument checks the host-rows entry points share, under the entry point's name in the messages
struct RowsCheck {
    const char* what; const char* bad = "negative";
    void args(int32_t rows, bool any_null) const { if (rows < 0 || (rows > 0 && any_null)) throw Error(PTTS_EINVAL, strfmt("ptts-hip: %s: null argument", what)); }
    void row(int i, int64_t n, bool any_null) const { if (n < 0 || (n > 0 && any_null)) throw Error(PTTS_EINVAL, strfmt("ptts-hip: %s: row %d is %s or null", what, i, bad)); }
};

static Model& model_of(ptts_model* h) {
    if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model is not fully initialized");
    return *h->m;
}

int ptts_resample(ptts_model* h, const float* const* in, const int64_t* n_in, int32_t n, int32_t in_rate, int32_t out_rate, float* const* out) {
    return guard([&] {
        Model& m = model_of(h);
        const std::string e = rate_pair_error(in_rate, out_rate);
        if (!e.empty()) throw Error(PTTS_EINVAL, e);
        const RowsCheck check{"resample", "empty"};
        check.args(n, !in || !n_in || !out);
        std::vector<int64_t> n_out((size_t)n);
        for (int i = 0; i < n; i++) {
            check.row(i, n_in[i], !in[i] || !out[i]);
            n_out[(size_t)i] = resample_length(n_in[i], in_rate, out_rate);
        }
        if (in_rate == out_rate) {   // the identity: no taps, no launch
            for (int i = 0; i < n; i++) if (n_in[i] > 0) std::memcpy(out[i], in[i], (size_t)n_in[i] * sizeof(float));
            return;
        }
        const Locked lock(m);
        staged_convert(m, in, n_in, n, rate_filter(m, in_rate, out_rate, m.stream), n_out.data(), RS_F32, (void* const*)out);
    });
}

// the device chain of ptts_request.dsp on host rows (dsp_rows_device: upload, the same launches, download)
int ptts_dsp_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, const ptts_dsp_opts* opts, float* const* out) {
    return guard([&] {
        Model& m = model_of(h);
        const RowsCheck check{"dsp"};
        check.args(rows, !in || !n || !out);
        DspSpec spec;
        std::string e = dsp_resolve(opts, &spec);
        if (e.empty()) e = dsp_trim_refusal(spec);   // the output rows have the input's length
        if (e.empty()) e = dsp_tempo_refusal(spec);
        if (e.empty()) e = dsp_pitch_refusal(spec);
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        for (int i = 0; i < rows; i++) check.row(i, n[i], !in[i] || !out[i]);
        if (!spec.any()) {   // nothing switched on: a copy, no lock, no launch
            for (int i = 0; i < rows; i++) if (n[i] > 0 && out[i] != in[i]) std::memmove(out[i], in[i], (size_t)n[i] * sizeof(float));
            return;
        }
        dsp_rows_device(m, in, n, rows, std::vector<DspSpec>((size_t)rows, spec).data(), true, {out});
    });
}

// The host-rows entry points with one stage and one option per row (ptts_eq_rows, ptts_compress_rows, ptts_deess_rows, ptts_limit_rows): the argument checks
// under the stage's name, each row's spec from per_row(i, spec) -- which returns the row's refusal, or nothing -- and the round trip.  A row
// whose spec stays empty is copied on the host
static int stage_rows(ptts_model* h, const char* what, bool opts_null, const float* const* in, const int64_t* n, int32_t rows, float* const* out,
                      const std::function<std::string(int, DspSpec&)>& per_row) {
    return guard([&] {
        Model& m = model_of(h);
        const RowsCheck check{what};
        check.args(rows, opts_null || !in || !n || !out);
        std::vector<DspSpec> specs((size_t)rows);
        for (int i = 0; i < rows; i++) {
            check.row(i, n[i], !in[i] || !out[i]);
            const std::string e = per_row(i, specs[(size_t)i]);
            if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        }
        dsp_rows_device(m, in, n, rows, specs.data(), true, {out});
    });
}

// the device form of ptts_eq_apply on host rows: the launches of a request's `eq`; a row without an equaliser is copied on the host
int ptts_eq_rows(ptts_model* h, const ptts_eq* const* eq, const float* const* in, const int64_t* n, int32_t rows, float* const* out) {
    return stage_rows(h, "eq", !eq, in, n, rows, out, [&](int i, DspSpec& spec) {
        if (eq[i] && !(spec.eq = eq_lookup(eq[i]))) return strfmt("eq: row %d: the handle is not a live equaliser of ptts_eq_create", i);
        return std::string();
    });
}

// the device form of ptts_compress_apply on host rows: the launches of a request's compressor; a row without one is copied on the host
int ptts_compress_rows(ptts_model* h, const ptts_compressor_opts* const* c, const float* const* in, const int64_t* n, int32_t rows, float* const* out) {
    return stage_rows(h, "compressor", !c, in, n, rows, out, [&](int i, DspSpec& spec) {
        if (!c[i]) return std::string();
        const std::string e = cmp_opts_error(c[i]);
        if (!e.empty()) return strfmt("row %d: ", i) + e;
        spec.compress = true;
        spec.cmp = cmp_design(*c[i]);
        return std::string();
    });
}

// the device form of ptts_deess_apply on host rows: the launches of a request's de-esser; a row without one is copied on the host
int ptts_deess_rows(ptts_model* h, const ptts_deesser_opts* const* d, const float* const* in, const int64_t* n, int32_t rows, float* const* out) {
    return stage_rows(h, "deesser", !d, in, n, rows, out, [&](int i, DspSpec& spec) {
        if (!d[i]) return std::string();
        const std::string e = de_opts_error(d[i]);
        if (!e.empty()) return strfmt("row %d: ", i) + e;
        spec.deess = true;
        spec.des = de_design(*d[i]);
        return std::string();
    });
}

// the device form of ptts_limit_apply on host rows: the launches of a request's limiter; a row without one is copied on the host
int ptts_limit_rows(ptts_model* h, const ptts_limiter_opts* const* l, const float* const* in, const int64_t* n, int32_t rows, float* const* out) {
    return stage_rows(h, "limiter", !l, in, n, rows, out, [&](int i, DspSpec& spec) {
        if (!l[i]) return std::string();
        const std::string e = lim_opts_error(l[i]);
        if (!e.empty()) return strfmt("row %d: ", i) + e;
        spec.limit = true;
        spec.lim = lim_design(*l[i]);
        return std::string();
    });
}

// The host-rows entry points of a joined call's part stages (ptts_trim_rows, ptts_tempo_rows, ptts_pitch_rows): the argument checks under the entry
// point's name, each row's stages from per_row(i, stages) -- which throws the row's refusal -- and the one round trip (part_rows_device).  A
// row whose stages stay empty is copied on the host.  designs: the caller's vectors of designs, sized here to one a row before the first row is
// looked at, so that what per_row points a row's stages to stays where it is
extern "C++" {
template <class... Design>
static int part_rows(ptts_model* h, const char* what, bool args_null, const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out,
                     ptts_trim_info* info, const std::function<void(int, PartStages&)>& per_row, std::vector<Design>&... designs) {
    return guard([&] {
        Model& m = model_of(h);
        const RowsCheck check{what};
        check.args(rows, args_null || !in || !n || !out);
        std::vector<PartStages> stages((size_t)rows);
        (designs.resize((size_t)rows), ...);
        for (int i = 0; i < rows; i++) {
            check.row(i, n[i], !in[i] || !out[i]);
            per_row(i, stages[(size_t)i]);
        }
        if (rows > 0) part_rows_device(m, stages.data(), in, n, rows, out, n_out, info);
    });
}
}  // extern "C++"
// such a row's refusal (e empty: none), as a stage's *_opts_error or a length check words it, behind the row's number
static void row_refuse(int i, const std::string& e) {
    if (!e.empty()) throw Error(PTTS_EINVAL, strfmt("ptts-hip: row %d: ", i) + e);
}

// the device form of ptts_trim_apply on host rows: the launches of a joined call's trim; a row without one is copied on the host
int ptts_trim_rows(ptts_model* h, const ptts_trim_opts* const* t, const float* const* in, const int64_t* n, int32_t rows, float* const* out, ptts_trim_info* info) {
    std::vector<TrimScan> designs;
    return part_rows(h, "trim", !t || !info, in, n, rows, out, nullptr, info, [&](int i, PartStages& st) {
        if (n[i] >= kTrimMaxSamples) throw Error(PTTS_EINVAL, strfmt("ptts-hip: trim: row %d has %lld samples, a row must stay below 2^31", i, (long long)n[i]));
        if (!t[i]) return;
        row_refuse(i, trim_opts_error(t[i]));
        designs[(size_t)i] = trim_design(*t[i]);
        st.trim = &designs[(size_t)i];
    }, designs);
}

// the trim of a joined call's parts, attached to the handle (trim.cpp checks and designs it, and stays a file that builds alone)
int ptts_dsp_ext_set_trim(ptts_dsp_ext* e, const ptts_trim_opts* t) { return ext_set(e, "trim", t, trim_opts_error, trim_design, &DspExt::trim, &DspExt::trm); }

// the device form of ptts_tempo_apply on host rows: the launches of a joined call's tempo; a row without one is copied on the host
int ptts_tempo_rows(ptts_model* h, const ptts_tempo_opts* const* t, const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out) {
    std::vector<TempoScan> designs;
    return part_rows(h, "tempo", !t || !n_out, in, n, rows, out, n_out, nullptr, [&](int i, PartStages& st) {
        if (n[i] >= kTempoMaxSamples) throw Error(PTTS_EINVAL, strfmt("ptts-hip: tempo: row %d has %lld samples, a row must stay below 2^31 - %d", i, (long long)n[i], kTempoRadius));
        if (!t[i]) return;
        row_refuse(i, tempo_opts_error(t[i]));
        if (n[i] > 0 && in[i] == out[i]) throw Error(PTTS_EINVAL, strfmt("ptts-hip: tempo: row %d: out is in", i));
        designs[(size_t)i] = tempo_design(*t[i]);
        st.tempo = &designs[(size_t)i];
    }, designs);
}

// the tempo of a joined call's parts, attached to the handle (tempo.cpp checks and designs it, and stays a file that builds alone)
int ptts_dsp_ext_set_tempo(ptts_dsp_ext* e, const ptts_tempo_opts* t) { return ext_set(e, "tempo", t, tempo_opts_error, tempo_design, &DspExt::tempo, &DspExt::tmp); }

// the device form of ptts_pitch_apply on host rows: the launches of a joined call's pitch and of the tempo behind it; a row with neither is copied on
// the host.  p[i] null: the tempo alone, as ptts_tempo_rows
// f null: ptts_pitch_rows.  Otherwise ptts_formant_rows: row i keeps its formants where f[i] says so and the row has a resampling step
static int pitch_rows(ptts_model* h, const char* what, const ptts_formant_opts* const* f, bool args_null, const ptts_pitch_opts* const* p, const ptts_tempo_opts* const* t,
                      const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out) {
    std::vector<PitchScan> pitches;
    std::vector<TempoScan> tempos;
    return part_rows(h, what, args_null || !p || !t || !n_out, in, n, rows, out, n_out, nullptr, [&](int i, PartStages& st) {
        if (f && f[i]) row_refuse(i, formant_opts_error(f[i]));
        if (p[i]) row_refuse(i, pitch_opts_error(p[i]));
        if (t[i]) row_refuse(i, tempo_opts_error(t[i]));
        PitchSteps run{t[i] ? t[i]->speed_permille : 1000, false, t[i] != nullptr};
        if (p[i]) {   // the pair resolves to the effective speed, and the tempo at 1000 is the identity
            std::string e = pitch_steps(p[i]->pitch_permille, run.E, &run);
            if (e.empty()) e = pitch_length_error(n[i], p[i]->pitch_permille, run.E);
            row_refuse(i, e);
            if (run.resample) pitches[(size_t)i] = pitch_design(*p[i]);
        } else if (n[i] >= kTempoMaxSamples) {
            row_refuse(i, strfmt("tempo: %lld samples, a row must stay below 2^31 - %d", (long long)n[i], kTempoRadius));
        }
        tempos[(size_t)i].speed = run.E;
        st.pitch = run.resample ? &pitches[(size_t)i] : nullptr;
        st.tempo = run.tempo ? &tempos[(size_t)i] : nullptr;
        if (n[i] > 0 && in[i] == out[i] && (st.pitch || st.tempo)) row_refuse(i, "pitch: out is in");
        if (f && f[i] && f[i]->keep && st.pitch) {
            row_refuse(i, formant_pitch_error(st.pitch->p));
            st.formant = true;
        }
    }, pitches, tempos);
}

int ptts_pitch_rows(ptts_model* h, const ptts_pitch_opts* const* p, const ptts_tempo_opts* const* t, const float* const* in, const int64_t* n, int32_t rows,
                    float* const* out, int64_t* n_out) {
    return pitch_rows(h, "pitch", nullptr, false, p, t, in, n, rows, out, n_out);
}

// the device form of ptts_formant_apply on host rows: ptts_pitch_rows, and for the rows with the option the formant kernels around the resample
int ptts_formant_rows(ptts_model* h, const ptts_formant_opts* const* f, const ptts_pitch_opts* const* p, const ptts_tempo_opts* const* t, const float* const* in,
                      const int64_t* n, int32_t rows, float* const* out, int64_t* n_out) {
    return pitch_rows(h, "formant", f, !f, p, t, in, n, rows, out, n_out);
}

// the option of a joined call's parts, attached to the handle (formant.cpp checks it, and stays a file that builds without HIP)
int ptts_dsp_ext_set_formant(ptts_dsp_ext* e, const ptts_formant_opts* f) { return ext_set(e, "formant", f, formant_opts_error, formant_design, &DspExt::formant, &DspExt::fmt); }

// the pitch of a joined call's parts, attached to the handle (pitch.cpp checks and designs it, and stays a file that builds without HIP)
int ptts_dsp_ext_set_pitch(ptts_dsp_ext* e, const ptts_pitch_opts* p) { return ext_set(e, "pitch", p, pitch_opts_error, pitch_design, &DspExt::pitch, &DspExt::pit); }

// the device form of ptts_join on host rows: k_join, as ptts_generate_joined launches it
int ptts_join_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* opts, float* out) {
    return guard([&] {
        Model& m = model_of(h);
        JoinLens l;
        std::string e = join_opts_error(opts, &l);
        int64_t total = 0;
        if (e.empty()) e = join_plan(n, rows, l, nullptr, nullptr, &total);
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        if (!in || (!out && total > 0)) throw Error(PTTS_EINVAL, "ptts-hip: join: null argument");
        for (int i = 0; i < rows; i++)
            if (!in[i] && n[i] > 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: join: part %d is null", i));
        join_rows_device(m, in, n, rows, l, out);
    });
}

// the statement of volume plus join (join.cpp join_parts_run), with the level's gain as ptts_loudness_normalize measures it
int ptts_join_parts(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, float* out, float* gains) {
    return join_parts_run(in, n, rows, o, po, out, gains,
                          [](const float* x, int64_t len, double target_lufs) { return loud_measure_gain(x, len, loud_target_power(target_lufs), nullptr); });
}

// the device form of ptts_join_parts on host rows: the loudness rows' measuring kernels for the levels, then k_join_gain (k_join for a table without a gain)
int ptts_join_parts_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* opts, const ptts_part_opts* po, float* out,
                         float* gains) {
    return guard([&] {
        Model& m = model_of(h);
        JoinLens l;
        JoinSeams seams;
        std::vector<PartVolume> vol;
        std::string e = join_opts_error(opts, &l);
        if (e.empty()) e = join_parts_error(po, rows, l, &seams, &vol);
        int64_t total = 0;
        if (e.empty()) e = join_parts_plan(n, rows, seams, nullptr, nullptr, &total);
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        if (!in || (!out && total > 0)) throw Error(PTTS_EINVAL, "ptts-hip: join: null argument");
        for (int i = 0; i < rows; i++)
            if (!in[i] && n[i] > 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: join: part %d is null", i));
        join_parts_rows_device(m, in, n, rows, seams, vol, out, gains);
    });
}

// target NULL: measurement only (lufs is required); otherwise out is, and lufs receives what was measured before
static void loudness_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, const double* target, float* const* out, double* lufs) {
    Model& m = model_of(h);
    const RowsCheck check{"loudness"};
    check.args(rows, !in || !n || (target && !out) || (!target && !lufs));
    if (target) {
        const std::string e = loud_target_error(*target);
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
    }
    for (int i = 0; i < rows; i++) check.row(i, n[i], !in[i] || (target && !out[i]));
    DspSpec spec;
    dsp_spec_loudness(spec, target);
    dsp_rows_device(m, in, n, rows, std::vector<DspSpec>((size_t)rows, spec).data(), target != nullptr, {target ? out : nullptr, lufs});
    if (lufs) for (int i = 0; i < rows; i++) lufs[i] = loud_lufs(lufs[i]);
}

int ptts_loudness_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, double* lufs) {
    return guard([&] { loudness_rows(h, in, n, rows, nullptr, nullptr, lufs); });
}

int ptts_loudness_normalize_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, double target_lufs, float* const* out, double* measured) {
    return guard([&] { loudness_rows(h, in, n, rows, &target_lufs, out, measured); });
}

// the device form of ptts_true_peak on host rows: the measuring launch of a request's ceiling alone, the rows' words back
int ptts_true_peak_rows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, float* peaks) {
    return guard([&] {
        Model& m = model_of(h);
        const RowsCheck check{"true peak"};
        check.args(rows, !in || !n || !peaks);
        for (int i = 0; i < rows; i++) check.row(i, n[i], !in[i]);
        DspSpec spec;
        spec.true_peak = true;
        dsp_rows_device(m, in, n, rows, std::vector<DspSpec>((size_t)rows, spec).data(), false, {nullptr, nullptr, nullptr, peaks});
    });
}

int ptts_pcm_encode(ptts_model* h, const float* in, int64_t n, int32_t pcm_format, void* out) {
    return guard([&] {
        Model& m = model_of(h);
        if (pcm_format < PTTS_PCM_F32 || pcm_format > PTTS_PCM_ALAW) throw Error(PTTS_EINVAL, strfmt("ptts-hip: pcm_format %d is not a PTTS_PCM_* format", pcm_format));
        if (n < 0 || (n > 0 && (!in || !out))) throw Error(PTTS_EINVAL, "ptts-hip: pcm encode: null argument");
        if (n == 0) return;
        const Locked lock(m);
        staged_convert(m, &in, &n, 1, nullptr, &n, pcm_format, &out);
    });
}

int ptts_wav_header(uint8_t* out, int32_t cap, int32_t sample_rate, int32_t pcm_format, int64_t n_samples) {
    const int rate = sample_rate ? sample_rate : kNativeRate;
    std::string e = rate_error(rate, false);
    if (e.empty() && (pcm_format < PTTS_PCM_F32 || pcm_format > PTTS_PCM_ALAW)) e = strfmt("ptts-hip: wav header: pcm_format %d is not a PTTS_PCM_* format", pcm_format);
    const bool pcm16 = pcm_format == PTTS_PCM_S16;
    const int len = pcm16 ? 44 : 58;
    const uint32_t bytes_per = (uint32_t)pcm_bytes(pcm_format);
    if (e.empty() && (!out || cap < len)) e = strfmt("ptts-hip: wav header: %d bytes of room, the header takes %d", cap, len);
    if (e.empty() && n_samples >= 0 && (uint64_t)n_samples * bytes_per > 0xFFFFFFFFull - (uint64_t)len) e = "ptts-hip: wav header: more data than a RIFF file holds";
    if (!e.empty()) { set_last_error(e); return -PTTS_EINVAL; }
    const bool streaming = n_samples < 0;
    const uint32_t data = streaming ? 0xFFFFFFFFu : (uint32_t)(n_samples * bytes_per);
    const uint32_t riff = streaming ? 0xFFFFFFFFu : data + (uint32_t)len - 8;
    uint8_t* p = out;
    auto tag = [&](const char* t) { std::memcpy(p, t, 4); p += 4; };
    auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) *p++ = (uint8_t)(v >> (8 * k)); };
    auto u16 = [&](uint32_t v) { *p++ = (uint8_t)v; *p++ = (uint8_t)(v >> 8); };
    // WAVE format tags: 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law
    const uint32_t fmt_tag = pcm16 ? 1 : pcm_format == PTTS_PCM_F32 ? 3 : pcm_format == PTTS_PCM_ALAW ? 6 : 7;
    tag("RIFF"); u32(riff); tag("WAVE");
    tag("fmt "); u32(pcm16 ? 16 : 18);
    u16(fmt_tag); u16(1); u32((uint32_t)rate); u32((uint32_t)rate * bytes_per); u16(bytes_per); u16(8 * bytes_per);
    if (!pcm16) {
        u16(0);                                                      // cbSize
        tag("fact"); u32(4); u32(streaming ? 0xFFFFFFFFu : (uint32_t)n_samples);
    }
    tag("data"); u32(data);
    return len;
}

void ptts_wav_header_streaming(uint8_t out[44]) {   // internal/audio/wav_stream.go:15-41
    static const uint8_t hdr[44] = {'R', 'I', 'F', 'F', 0xFF, 0xFF, 0xFF, 0xFF, 'W', 'A', 'V', 'E', 'f', 'm', 't', ' ', 16, 0, 0, 0, 1, 0, 1, 0,
                                    0xC0, 0x5D, 0, 0 /* 24000 */, 0x80, 0xBB, 0, 0 /* 48000 B/s */, 2, 0, 16, 0, 'd', 'a', 't', 'a', 0xFF, 0xFF, 0xFF, 0xFF};
    memcpy(out, hdr, 44);
}

}  // extern "C"
