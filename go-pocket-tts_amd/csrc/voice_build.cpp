// voice_build.cpp -- device voices made on the GPU from voice embeddings (cloned voices as model states), and a device voice read back in the
// reference's cache layout.  The state is the one runtime_native_safetensors.go:104-119 builds when it prepends a voice embedding to the prompt:
// the embedding alone, prefilled from position 0 (flow_lm.go:155-187); what the reference's `pocket-tts export-voice --format model-state`
// stores per layer as `transformer.layers.N.self_attn/cache` [2,1,T,H,Dh] + `/offset` (cmd/pockettts/export_voice.go).
#include "runtime.h"

namespace ptts {

std::vector<std::unique_ptr<Voice>> voice_build(Model& m, const float* const* emb, const int64_t* frames, int64_t width, int n) {
    const Desc& d = m.d;
    if (n <= 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice build needs at least one embedding, got %d", n));
    if (!emb || !frames) throw Error(PTTS_EINVAL, "ptts-hip: voice build: null embedding list");
    if (width != d.d_model) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice embedding width %lld, the model's d_model is %d", (long long)width, d.d_model));
    for (int i = 0; i < n; i++) {
        if (!emb[i]) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice build: embedding %d is null", i));
        if (frames[i] < 1 || frames[i] > ROPE_SEQ)
            throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice embedding %d has %lld frames, outside [1, %d] (RoPE table rows)", i, (long long)frames[i], ROPE_SEQ));
    }
    const size_t es = m.opts.kv == PTTS_KV_BF16 ? 2 : 4;
    if ((d.hd * es) % 16 != 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: head dim %d does not fill whole 16-byte chunks", d.hd));
    std::vector<std::unique_ptr<Voice>> out;
    out.reserve((size_t)n);
    // one prefill per group of at most kStepMaxRows embeddings (a batch's slot limit): every call that fits one batch is one prefill
    for (int g0 = 0; g0 < n; g0 += kStepMaxRows) {
        const int B = std::min(n - g0, kStepMaxRows);
        int cap = 0;
        std::vector<int64_t> row_off((size_t)B + 1, 0);
        for (int i = 0; i < B; i++) {
            cap = std::max(cap, (int)frames[g0 + i]);
            row_off[(size_t)i + 1] = row_off[(size_t)i] + frames[g0 + i];
        }
        std::unique_ptr<Batch> b(batch_new(m, B, cap, 1));
        DevBuf& rows = m.work(WORK_VOICE_BUILD_ROWS, (size_t)row_off[(size_t)B] * d.d_model * sizeof(float));
        for (int i = 0; i < B; i++)
            PTTS_HIP(hipMemcpyAsync(rows.as<float>() + row_off[(size_t)i] * d.d_model, emb[g0 + i], (size_t)frames[g0 + i] * d.d_model * sizeof(float),
                                    hipMemcpyHostToDevice, m.stream));
        batch_prompt(*b, rows.as<float>(), row_off.data());   // voice first, no text: positions 0 .. frames - 1 of each slot
        std::vector<VoiceDst> tab((size_t)B);
        for (int i = 0; i < B; i++) {
            std::unique_ptr<Voice> v(new Voice());
            v->m = &m;
            v->device = m.device;
            v->offset = (int)frames[g0 + i];
            const size_t lb = v->layer_bytes();
            v->k.ensure(lb * d.n_layers);
            v->v.ensure(lb * d.n_layers);
            tab[(size_t)i] = VoiceDst{v->k.p, v->v.p, v->offset, i};
            out.push_back(std::move(v));
        }
        DevBuf& dt = m.work(WORK_VOICE_BUILD_TABLE, tab.size() * sizeof(VoiceDst));
        PTTS_HIP(hipMemcpyAsync(dt.p, tab.data(), tab.size() * sizeof(VoiceDst), hipMemcpyHostToDevice, m.stream));
        launch_voice_extract(b->kcache.p, b->vcache.p, B, b->cap, d.heads, d.hd, (int)es, d.n_layers, dt.as<VoiceDst>(), B, cap, m.stream);
        PTTS_HIP(hipStreamSynchronize(m.stream));   // (the batch and the host table go out of scope)
    }
    return out;
}

void voice_export(const Voice& v, int layer0, int n_layers, float* out) {
    Model& m = *v.m;
    const Desc& d = m.d;
    if (layer0 < 0 || n_layers < 1 || layer0 + n_layers > d.n_layers)
        throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice layers [%d, %d) outside [0, %d)", layer0, layer0 + n_layers, d.n_layers));
    if (d.hd % 8 != 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: head dim %d is not a multiple of 8", d.hd));
    const size_t n = (size_t)n_layers * 2 * v.offset * d.heads * d.hd;
    if (n == 0) return;
    const size_t lb = v.layer_bytes();
    DevBuf& o = m.work(WORK_VOICE_EXPORT, n * sizeof(float));
    launch_voice_export((const char*)v.k.p + lb * layer0, (const char*)v.v.p + lb * layer0, v.offset, d.heads, d.hd, n_layers,
                        m.opts.kv == PTTS_KV_BF16, o.as<float>(), m.stream);
    d2h(out, o.p, n * sizeof(float), m.stream);
}

void voice_read_state(const Voice& v, int layer, float* out) { voice_export(v, layer, 1, out); }

std::vector<uint8_t> voice_state_bytes(const Voice& v) {
    const Desc& d = v.m->d;
    const size_t per = (size_t)2 * v.offset * d.heads * d.hd;
    std::vector<float> all(per * d.n_layers);
    voice_export(v, 0, d.n_layers, all.data());
    std::vector<const float*> caches((size_t)d.n_layers);
    for (int l = 0; l < d.n_layers; l++) caches[(size_t)l] = all.data() + per * l;
    return voice_state_file(caches.data(), v.offset, d.n_layers, d.heads, d.hd);
}

}  // namespace ptts
