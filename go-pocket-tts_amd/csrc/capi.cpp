// capi.cpp -- extern "C" surface of libptts_hip.so (include/ptts.h): options, plan, model, generate and joined calls, dispatcher, text and tokenizer, voices
// and voice files, profile, and the forwards of the staged entry points (staged.cpp).  Host rows: capi_rows.cpp; ptts_op_*: capi_ops.cpp.
#include "capi_internal.h"

using namespace ptts;
using namespace ptts::capi;

extern "C" {

void ptts_default_opts(ptts_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->device = 0;
    o->weights = PTTS_WEIGHTS_F32;
    o->kv = PTTS_KV_F32;
    o->max_batch = 64;
    o->use_graph = 0;
}

const char* ptts_last_error(void) { return last_error_ref().c_str(); }
const char* ptts_version(void) { return "ptts-hip 0.3 gfx950"; }

int ptts_plan_create(const char* path, const ptts_opts* opts, ptts_plan** out) {
    return guard([&] {
        if (!path || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_plan> pl(new ptts_plan());
        pl->p.opts = resolve_opts(opts);
        st_open_path(path, pl->p.file);
        plan_build(pl->p);
        *out = pl.release();
    });
}

int ptts_plan_create_bytes(const void* data, size_t len, const ptts_opts* opts, ptts_plan** out) {
    return guard([&] {
        if (!data || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_plan> pl(new ptts_plan());
        pl->p.opts = resolve_opts(opts);
        pl->p.file.owned.assign((const uint8_t*)data, (const uint8_t*)data + len);  // OpenStoreFromBytes keeps the bytes
        pl->p.file.data = pl->p.file.owned.data();
        pl->p.file.size = len;
        st_parse(pl->p.file);
        plan_build(pl->p);
        *out = pl.release();
    });
}

size_t ptts_plan_arena_bytes(const ptts_plan* p) { return p ? p->p.desc.total_bytes : 0; }

int ptts_plan_fill_host(const ptts_plan* p, void* host_arena) {
    return guard([&] {
        if (!p || !host_arena) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::memset(host_arena, 0, p->p.desc.total_bytes);
        plan_fill(p->p, reinterpret_cast<uint8_t*>(host_arena));
    });
}
void ptts_plan_free(ptts_plan* p) { delete p; }

int ptts_dsp_apply(float* samples, int64_t n, int32_t normalize, int32_t dc_block, double fade_in_ms, double fade_out_ms) {
    return guard([&] {
        if ((!samples && n > 0) || n < 0) throw Error(PTTS_EINVAL, "audio: nil samples");
        const int sr = 24000;   // audio.ExpectedSampleRate
        if (normalize) dsp_peak_normalize(samples, n);
        if (dc_block) dsp_dc_block(samples, n, sr);
        if (fade_in_ms > 0) dsp_fade_in(samples, n, sr, fade_in_ms);
        if (fade_out_ms > 0) dsp_fade_out(samples, n, sr, fade_out_ms);
    });
}

int ptts_loudness(const float* samples, int64_t n, double* lufs) {
    return guard([&] {
        if ((!samples && n > 0) || n < 0 || !lufs) throw Error(PTTS_EINVAL, "ptts-hip: loudness: null argument");
        *lufs = loud_lufs(loud_measure(samples, n));
    });
}

int ptts_loudness_normalize(float* samples, int64_t n, double target_lufs, double* measured) {
    return guard([&] {
        if ((!samples && n > 0) || n < 0) throw Error(PTTS_EINVAL, "ptts-hip: loudness: null argument");
        const std::string e = loud_target_error(target_lufs);
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        const double M = loud_normalize(samples, n, target_lufs);
        if (measured) *measured = loud_lufs(M);
    });
}

int ptts_rccl_unique_id(uint8_t out[128]) {
    return guard([&] {
        if (!out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        require_device();
        rccl_unique_id(out);
    });
}

int ptts_rccl_broadcast(void* device_buf, size_t bytes, int32_t rank, int32_t n_ranks, const uint8_t id[128], int32_t device) {
    return guard([&] {
        require_device();
        rccl_broadcast(device_buf, bytes, rank, n_ranks, id, device);
    });
}

int ptts_model_open_planned(ptts_plan* p, void* device_arena, int fill, ptts_model** out) {
    int rc = guard([&] {
        if (!p || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_model> h(new ptts_model());
        h->m = model_open(&p->p, device_arena, fill);
        *out = h.release();
    });
    delete p;
    return rc;
}

int ptts_model_share(ptts_model* base, ptts_model** out) {
    return guard([&] {
        if (!base || !base->m || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_model> h(new ptts_model());
        h->m = model_share(*base->m);
        *out = h.release();
    });
}

int ptts_model_replicate(ptts_model* base, int32_t device, ptts_model** out) {
    return guard([&] {
        if (!base || !base->m || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_model> h(new ptts_model());
        h->m = model_replicate(*base->m, device);
        *out = h.release();
    });
}

int ptts_model_set_use_graph(ptts_model* m, int32_t use_graph) {
    return guard([&] {
        if (!m || !m->m) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::lock_guard<std::mutex> lock(m->m->mu);   // not under a running generate
        m->m->opts.use_graph = use_graph ? 1 : 0;
    });
}

int ptts_model_set_max_batch(ptts_model* m, int32_t max_batch) {
    return guard([&] {
        if (!m || !m->m) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        if (max_batch < 1 || max_batch > kStepMaxRows) throw Error(PTTS_EINVAL, strfmt("ptts-hip: max_batch %d outside [1, %d]", max_batch, kStepMaxRows));
        std::lock_guard<std::mutex> lock(m->m->mu);   // not under a running generate
        m->m->opts.max_batch = max_batch;
    });
}

int ptts_model_open(const char* path, const ptts_opts* opts, ptts_model** out) {
    ptts_plan* pl = nullptr;
    int rc = ptts_plan_create(path, opts, &pl);
    if (rc) return rc;
    return ptts_model_open_planned(pl, nullptr, 1, out);
}

int ptts_model_open_bytes(const void* data, size_t len, const ptts_opts* opts, ptts_model** out) {
    ptts_plan* pl = nullptr;
    int rc = ptts_plan_create_bytes(data, len, opts, &pl);
    if (rc) return rc;
    return ptts_model_open_planned(pl, nullptr, 1, out);
}

void ptts_model_close(ptts_model* m) {
    if (!m) return;
    if (m->m) {
        (void)hipSetDevice(m->m->device);
        delete m->m;
    }
    delete m;
}

int ptts_model_info(const ptts_model* h, ptts_info* o) {
    return guard([&] {
        if (!h || !h->m || !o) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        const Desc& d = h->m->d;
        std::memset(o, 0, sizeof *o);
        o->d_model = d.d_model; o->n_heads = d.heads; o->n_layers = d.n_layers; o->ffn = d.ffn; o->ldim = d.ldim; o->n_bins = d.n_bins;
        o->flow_dim = d.flow_dim; o->flow_depth = d.flow_depth;
        o->mimi_dim = d.mimi_dim; o->mimi_heads = d.mimi_heads; o->mimi_layers = d.mimi_layers; o->mimi_context = d.mimi_ctx;
        o->sample_rate = 24000; o->samples_per_frame = d.samples_per_frame; o->steps_per_latent = d.up_stride;
        o->frame_rate = 12.5; o->encoder_frame_rate = 200.0;  // mimi.go:25-34
        o->n_params = d.n_params; o->arena_bytes = (int64_t)d.total_bytes;
        o->weights = h->m->opts.weights; o->kv = h->m->opts.kv;
    });
}

int ptts_generate(ptts_model* h, const ptts_request* reqs, int32_t n, ptts_result* results) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        if (!reqs || !results || n <= 0) throw Error(PTTS_EINVAL, "ptts-hip: no requests");
        set_last_error("");
        generate(*h->m, reqs, n, results);
        for (int i = 0; i < n; i++)
            if (results[i].status != PTTS_OK) {
                std::string msg = last_error_ref();
                throw Error(results[i].status, msg.empty() ? "generate: request failed" : msg);
            }
    });
}

void ptts_free_result(ptts_result* r) {
    if (!r) return;
    result_free(r->pcm);
    result_free(r->pcm16);
    result_free(r->pcm8);
    free(r->latents);
    r->pcm = nullptr;
    r->pcm16 = nullptr;
    r->pcm8 = nullptr;
    r->latents = nullptr;
    r->n_samples = 0;
    r->n_frames = 0;
}

struct ptts_chunks { std::vector<TextChunk> v; };

int32_t ptts_text_estimate_max_frames(int64_t token_count, double frame_rate) { return text_estimate_max_frames(token_count, frame_rate); }
int32_t ptts_text_frames_after_eos(int64_t num_words) { return text_frames_after_eos(num_words); }

int ptts_text_prepare(const char* utf8, int64_t len, char* out, int64_t cap, int64_t* out_len) {
    return guard([&] {
        if ((!utf8 && len > 0) || len < 0 || !out_len) throw Error(PTTS_EINVAL, "text: nil argument");
        const std::string r = text_prepare(std::string(utf8 ? utf8 : "", (size_t)len));
        *out_len = (int64_t)r.size();
        if (out && cap > 0) memcpy(out, r.data(), (size_t)std::min<int64_t>(cap, (int64_t)r.size()));
    });
}

struct ptts_tokenizer { Tokenizer* t; };

int ptts_tokenizer_open(const char* model_path, ptts_tokenizer** out) {
    return guard([&] {
        if (!out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_tokenizer> h(new ptts_tokenizer());
        h->t = tokenizer_from_path(model_path ? model_path : "");
        *out = h.release();
    });
}

int ptts_tokenizer_open_bytes(const void* data, size_t len, ptts_tokenizer** out) {
    return guard([&] {
        if (!out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<ptts_tokenizer> h(new ptts_tokenizer());
        h->t = tokenizer_from_bytes(data, len);
        *out = h.release();
    });
}

void ptts_tokenizer_free(ptts_tokenizer* t) {
    if (!t) return;
    tokenizer_free(t->t);
    delete t;
}

int64_t ptts_tokenizer_vocab_size(const ptts_tokenizer* t) { return t && t->t ? (int64_t)tokenizer_vocab(*t->t) : 0; }

int64_t ptts_tokenizer_encode(const ptts_tokenizer* t, const char* utf8, int64_t len, int64_t* ids, int64_t cap) {
    int64_t n = -1;
    guard([&] {
        if (!t || !t->t) throw Error(PTTS_EINVAL, "tokenizer is nil");
        if ((!utf8 && len > 0) || len < 0) throw Error(PTTS_EINVAL, "tokenizer: nil text");
        const std::vector<int64_t> v = tokenizer_encode(*t->t, std::string(utf8 ? utf8 : "", (size_t)len));
        for (int64_t i = 0; i < (int64_t)v.size() && i < cap && ids; i++) ids[i] = v[(size_t)i];
        n = (int64_t)v.size();
    });
    return n;
}

int64_t ptts_tokenizer_encode_cb(void* user, const char* utf8, int64_t len, int64_t* ids, int64_t cap) {
    return ptts_tokenizer_encode(reinterpret_cast<const ptts_tokenizer*>(user), utf8, len, ids, cap);
}

int ptts_text_nfkc(const char* utf8, int64_t len, char* out, int64_t cap, int64_t* out_len) {
    return guard([&] {
        if ((!utf8 && len > 0) || len < 0 || !out_len) throw Error(PTTS_EINVAL, "text: nil argument");
        const std::string r = nfkc_utf8(std::string(utf8 ? utf8 : "", (size_t)len));
        *out_len = (int64_t)r.size();
        if (out && cap > 0) std::memcpy(out, r.data(), (size_t)std::min<int64_t>(cap, (int64_t)r.size()));
    });
}

int ptts_text_chunks(const char* utf8, int64_t len, ptts_encode_fn encode, void* user, int32_t max_tokens, double frame_rate, ptts_chunks** out) {
    return guard([&] {
        if (!encode && user) encode = ptts_tokenizer_encode_cb;   // default encoder: `user` is a ptts_tokenizer
        if ((!utf8 && len > 0) || len < 0 || !encode || !out) throw Error(PTTS_EINVAL, "text: nil argument");
        TextEncodeFn enc = [&](const std::string& t) {
            std::vector<int64_t> ids(64);
            int64_t n = encode(user, t.data(), (int64_t)t.size(), ids.data(), (int64_t)ids.size());
            if (n > (int64_t)ids.size()) {
                ids.resize((size_t)n);
                n = encode(user, t.data(), (int64_t)t.size(), ids.data(), (int64_t)ids.size());
            }
            if (n < 0) throw Error(PTTS_EINVAL, "encode \"" + t + "\": tokenizer error");
            ids.resize((size_t)n);
            return ids;
        };
        std::unique_ptr<ptts_chunks> c(new ptts_chunks());
        c->v = text_chunks(std::string(utf8 ? utf8 : "", (size_t)len), enc, max_tokens, frame_rate);
        *out = c.release();
    });
}

int32_t ptts_chunks_count(const ptts_chunks* c) { return c ? (int32_t)c->v.size() : 0; }

int ptts_chunks_get(const ptts_chunks* c, int32_t i, ptts_chunk_info* out) {
    return guard([&] {
        if (!c || !out || i < 0 || i >= (int32_t)c->v.size()) throw Error(PTTS_EINVAL, "text: chunk index out of range");
        const TextChunk& t = c->v[(size_t)i];
        std::memset(out, 0, sizeof *out);
        out->text = t.text.data(); out->text_len = (int64_t)t.text.size();
        out->token_ids = t.token_ids.data(); out->n_tokens = (int64_t)t.token_ids.size();
        out->num_words = t.num_words; out->max_frames = t.max_frames; out->frames_after_eos = t.frames_after_eos;
    });
}

void ptts_chunks_free(ptts_chunks* c) { delete c; }

struct ptts_dispatcher { Dispatcher* d; };

int ptts_dispatcher_create(ptts_model* const* models, int32_t n_models, const ptts_dispatch_opts* o, ptts_dispatcher** out) {
    return guard([&] {
        if (!models || n_models <= 0 || !out) throw Error(PTTS_EINVAL, "dispatcher: at least one model is required");
        std::vector<Model*> ms;
        for (int i = 0; i < n_models; i++) {
            if (!models[i] || !models[i]->m) throw Error(PTTS_EINVAL, "dispatcher: nil model");
            ms.push_back(models[i]->m);
        }
        DispatchCont dc;
        if (o) { dc.on = o->continuous; dc.kv_capacity = o->cont_kv_capacity; dc.max_steps = o->cont_max_steps; dc.steps_per_group = o->cont_steps_per_group; }
        *out = new ptts_dispatcher{dispatcher_create(ms.data(), n_models, nullptr, nullptr, 0, o ? o->max_batch : 0, o ? o->window_us : 2000, o ? o->queue_cap : 0, &dc)};
    });
}

int ptts_dispatcher_create_custom(ptts_dispatch_exec exec, void* user, int32_t n_workers, const ptts_dispatch_opts* o, ptts_dispatcher** out) {
    return guard([&] {
        if (!exec || !out) throw Error(PTTS_EINVAL, "dispatcher: nil executor");
        *out = new ptts_dispatcher{dispatcher_create(nullptr, 0, exec, user, n_workers, o ? o->max_batch : 0, o ? o->window_us : 2000, o ? o->queue_cap : 0)};
    });
}

int ptts_dispatch_generate(ptts_dispatcher* d, const ptts_request* req, ptts_result* result) {
    return guard([&] {
        if (!d || !d->d || !req || !result) throw Error(PTTS_EINVAL, "dispatcher: nil argument");
        std::string err;
        const int rc = dispatcher_generate(d->d, req, result, &err);
        if (rc != PTTS_OK) throw Error(rc, err.empty() ? "generate: request failed" : err);
    });
}

void ptts_dispatcher_stats(ptts_dispatcher* d, ptts_dispatch_stats* out) {
    if (d && d->d && out) dispatcher_stats(d->d, out);
}

void ptts_dispatcher_close(ptts_dispatcher* d) {
    if (!d) return;
    dispatcher_close(d->d);
    delete d;
}

int ptts_voice_create(ptts_model* h, const float* const* caches, const int64_t* steps, const int64_t* offsets, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!caches || !steps || !offsets) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        const Locked lock(*h->m);
        *out = reinterpret_cast<ptts_voice*>(voice_create(*h->m, caches, steps, offsets));
    });
}

void ptts_voice_free(ptts_voice* v) {
    if (!v) return;
    Voice* vv = reinterpret_cast<Voice*>(v);
    (void)hipSetDevice(vv->device);
    delete vv;
}

// ---- voice files (voicefile.cpp) ----
int ptts_voice_file_open(const char* path, ptts_voice_file** out) {
    return guard([&] {
        if (!path || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        *out = reinterpret_cast<ptts_voice_file*>(voice_file_from_path(path));
    });
}

int ptts_voice_file_open_bytes(const void* data, size_t len, ptts_voice_file** out) {
    return guard([&] {
        if ((!data && len) || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        *out = reinterpret_cast<ptts_voice_file*>(voice_file_from_bytes(data, len));
    });
}

void ptts_voice_file_close(ptts_voice_file* f) { delete reinterpret_cast<VoiceFile*>(f); }

int32_t ptts_voice_file_kind(const ptts_voice_file* f) { return f ? reinterpret_cast<const VoiceFile*>(f)->kind : PTTS_VOICE_FILE_UNKNOWN; }

int ptts_voice_file_embedding(const ptts_voice_file* f, const float** data, int64_t shape[3]) {
    return guard([&] {
        if (!f || !data || !shape) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        voice_file_embedding(*reinterpret_cast<const VoiceFile*>(f), data, shape);
    });
}

int ptts_voice_file_modules(const ptts_voice_file* f, int32_t* n) {
    return guard([&] {
        if (!f || !n) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        const VoiceFile& v = *reinterpret_cast<const VoiceFile*>(f);
        voice_file_require_state(v);
        *n = (int32_t)v.modules.size();
    });
}

int ptts_voice_file_module(const ptts_voice_file* f, int32_t i, const char** name, ptts_voice_tensor* cache, ptts_voice_tensor* offset) {
    return guard([&] {
        if (!f) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        const VoiceFile& v = *reinterpret_cast<const VoiceFile*>(f);
        voice_file_require_state(v);
        if (i < 0 || (size_t)i >= v.modules.size()) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice module index %d out of range [0,%zu)", i, v.modules.size()));
        const VoiceFile::Module& m = v.modules[(size_t)i];
        if (name) *name = m.name.c_str();
        auto put = [&](const char* key, ptts_voice_tensor* o) {
            if (!o) return;
            std::memset(o, 0, sizeof *o);
            auto it = m.tensors.find(key);
            if (it == m.tensors.end()) return;
            static const float none = 0.0f;
            o->data = it->second.data.empty() ? &none : it->second.data.data();   // present but empty: data non-NULL, count 0
            o->count = (int64_t)it->second.data.size();
            o->rank = (int32_t)std::min<size_t>(it->second.shape.size(), 8);
            for (int32_t d = 0; d < o->rank; d++) o->shape[d] = it->second.shape[(size_t)d];
        };
        put("cache", cache);
        put("offset", offset);
    });
}

int ptts_voice_file_state(const ptts_voice_file* f, int32_t n_layers, int32_t heads, int32_t head_dim, const float** caches, int64_t* steps, int64_t* offsets) {
    return guard([&] {
        if (!f) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        if (n_layers < 0 || (n_layers > 0 && (!caches || !steps || !offsets))) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        voice_file_state(*reinterpret_cast<const VoiceFile*>(f), n_layers, heads, head_dim, caches, steps, offsets);
    });
}

static void voice_upload_from_file(ptts_model* h, const VoiceFile& vf, ptts_voice** out) {
    Model& m = *h->m;
    std::vector<const float*> caches((size_t)m.d.n_layers);
    std::vector<int64_t> steps((size_t)m.d.n_layers), offs((size_t)m.d.n_layers);
    voice_file_state(vf, m.d.n_layers, m.d.heads, m.d.hd, caches.data(), steps.data(), offs.data());
    const Locked lock(m);
    *out = reinterpret_cast<ptts_voice*>(voice_create(m, caches.data(), steps.data(), offs.data()));
}

int ptts_voice_open(ptts_model* h, const char* path, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!path) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<VoiceFile> vf(voice_file_from_path(path));
        voice_upload_from_file(h, *vf, out);
    });
}

int ptts_voice_open_bytes(ptts_model* h, const void* data, size_t len, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!data && len) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        std::unique_ptr<VoiceFile> vf(voice_file_from_bytes(data, len));
        voice_upload_from_file(h, *vf, out);
    });
}

int ptts_profile_enable(ptts_model* h, int32_t on) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        std::lock_guard<std::mutex> lock(h->m->mu);
        h->m->prof.on = on == 1;          // 1: per-launch events (plain launches) + phases; 2: phases only
        h->m->prof.phases_on = on != 0;
        h->m->prof.used = 0; h->m->prof.bytes = 0; h->m->prof.wbytes = 0; h->m->prof.launches = 0; h->m->prof.phases = false;
    });
}

int ptts_profile_read(ptts_model* h, ptts_profile* out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        const Locked lock(*h->m);
        profile_read(*h->m, out);
    });
}

int ptts_text_embeddings(ptts_model* h, const int64_t* ids, int64_t n, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        Model& m = *h->m;
        const Locked lock(m);
        for (int64_t i = 0; i < n; i++)
            if (ids[i] < 0 || ids[i] >= m.d.n_bins) throw Error(PTTS_EINVAL, strfmt("native: token id %lld (%lld) out of range [0,%d)", (long long)i, (long long)ids[i], m.d.n_bins));
        if (n == 0) return;
        staged_text_embeddings(m, ids, n, out);
    });
}

int ptts_batch_new(ptts_model* h, int32_t n_slots, int32_t kv_capacity, ptts_batch** out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        std::lock_guard<std::mutex> lock(h->m->mu);
        std::unique_ptr<ptts_batch> b(new ptts_batch());
        b->m = h->m;
        b->b = batch_new(*h->m, n_slots, kv_capacity, 1);
        PTTS_HIP(hipStreamSynchronize(h->m->stream));
        *out = b.release();
    });
}

void ptts_batch_free(ptts_batch* b) {
    if (!b) return;
    if (b->b) {
        (void)hipSetDevice(b->m->device);
        (void)hipStreamSynchronize(b->m->stream);
        delete b->b;
    }
    delete b;
}

int ptts_batch_reset(ptts_batch* b) {
    return guard([&] {
        if (!b || !b->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        const Locked lock(*b->m);
        batch_reset(*b->b);
        PTTS_HIP(hipStreamSynchronize(b->m->stream));
    });
}

int ptts_batch_set_voice_state(ptts_batch* b, int32_t slot, const float* const* caches, const int64_t* steps, const int64_t* offsets) {
    return guard([&] {
        if (!b || !b->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        if (!caches || !steps || !offsets) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        const Locked lock(*b->m);
        batch_set_voice(*b->b, slot, caches, steps, offsets);
    });
}

int ptts_batch_prompt(ptts_batch* b, const float* emb, const int64_t* row_offsets) {
    return guard([&] {
        if (!b || !b->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        if (!row_offsets) throw Error(PTTS_EINVAL, "native: prompt text embeddings are nil");
        Model& m = *b->m;
        const Locked lock(m);
        if (row_offsets[b->b->B] > 0 && !emb) throw Error(PTTS_EINVAL, "native: prompt text embeddings are nil");
        staged_prompt(*b->b, emb, row_offsets);
    });
}

int ptts_batch_step(ptts_batch* hb, const float* frames_in, int32_t lsd_steps, const float* noise, float* frames_out,
                    float* eos_logits, float* last_hidden) {
    return guard([&] {
        if (!hb || !hb->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        if (lsd_steps <= 0) throw Error(PTTS_EINVAL, "native: lsd decode steps must be >0");
        if (!frames_in) throw Error(PTTS_EINVAL, "native: replaceNaNWithVector requires non-nil tensors");
        Model& m = *hb->m;
        Batch& b = *hb->b;
        const Locked lock(m);
        for (int i = 0; i < b.B; i++)
            if (b.kv_len_host[i] + 1 > b.cap) throw Error(PTTS_EINVAL, "ptts-hip: KV capacity exhausted");
        staged_step(b, frames_in, lsd_steps, noise, frames_out, eos_logits, last_hidden);
    });
}

int ptts_batch_offsets(ptts_batch* b, int64_t* out) {
    return guard([&] {
        if (!b || !b->b || !out) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        for (int i = 0; i < b->b->B; i++) out[i] = b->b->kv_len_host[i];
    });
}

int ptts_batch_read_kv(ptts_batch* hb, int32_t slot, int32_t layer, float* k, float* v) {
    return guard([&] {
        if (!hb || !hb->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        Model& m = *hb->m;
        Batch& b = *hb->b;
        if (slot < 0 || slot >= b.B || layer < 0 || layer >= m.d.n_layers) throw Error(PTTS_EINVAL, "ptts-hip: slot/layer out of range");
        const Locked lock(m);
        staged_read_kv(b, slot, layer, k, v);
    });
}

int ptts_decode_latents(ptts_model* h, const float* latents, int32_t n_utt, int32_t frames, float* pcm, float* mimi_latent) {
    return ptts::capi::decode_stages(h, latents, n_utt, frames, pcm, mimi_latent, nullptr);
}

}  // extern "C"

// the Mimi encoder with the staged observation points of tests (stages; capi_hooks.cpp ptts_debug_encode_stages)
int ptts::capi::encode_stages(ptts_model* h, const float* const* pcm, const int64_t* n_samples, int32_t n_clips, float* const* latent_out, float* const* stages,
                              const int32_t* rates) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        Model& m = *h->m;
        require_encoder(m.d);
        const Locked lock(m);
        mimi_encode(m, pcm, n_samples, n_clips, latent_out, stages, rates);
    });
}

// LatentToMimi + MimiDecode with the staged observation point of tests (transformer_out; capi_hooks.cpp ptts_decode_stages)
int ptts::capi::decode_stages(ptts_model* h, const float* latents, int32_t n_utt, int32_t frames, float* pcm, float* mimi_latent, float* transformer_out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model is not fully initialized");
        if (!latents) throw Error(PTTS_EINVAL, "native: latent tensor is nil");
        if (n_utt <= 0 || frames <= 0) throw Error(PTTS_EINVAL, strfmt("native: latent shape must be positive, got [%d %d 32]", n_utt, frames));
        Model& m = *h->m;
        const Locked lock(m);
        staged_decode(m, latents, n_utt, frames, pcm, mimi_latent, transformer_out);
    });
}

// encoder + speaker projection (EncodeVoice, onnx/voice_encode.go:23-158): PTTS_EFORMAT naming what the checkpoint lacks
static void require_voice_encoder(const Desc& d) {
    require_encoder(d);
    const Lin& l = d.speaker_proj;
    if (l.w == NONE) throw Error(PTTS_EFORMAT, "load speaker_proj_weight: tensor not found in the model weights");
    if (l.in != d.mimi_dim) throw Error(PTTS_EFORMAT, strfmt("speaker_proj_weight takes %d-wide latents, the encoder makes %d", l.in, d.mimi_dim));
}

static void voices_out(std::vector<std::unique_ptr<Voice>>& vs, ptts_voice** out) {
    for (size_t i = 0; i < vs.size(); i++) out[i] = reinterpret_cast<ptts_voice*>(vs[i].release());
}

static void bytes_out(const std::vector<uint8_t>& b, uint8_t** data, size_t* len) {
    uint8_t* p = (uint8_t*)malloc(std::max<size_t>(b.size(), 1));
    if (!p) throw std::bad_alloc();
    std::memcpy(p, b.data(), b.size());
    *data = p;
    *len = b.size();
}

// a device voice as a model-state file, under its engine's lock
static std::vector<uint8_t> voice_file_bytes(const ptts_voice* hv) {
    if (!hv) throw Error(PTTS_EINVAL, "native: voice model state is nil");
    const Voice& v = *reinterpret_cast<const Voice*>(hv);
    const Locked lock(*v.m);
    return voice_state_bytes(v);
}

extern "C" {

int ptts_speaker_project(ptts_model* h, const float* latent, int64_t frames, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        Model& m = *h->m;
        const Lin& l = m.d.speaker_proj;
        if (l.w == NONE) throw Error(PTTS_EFORMAT, "load speaker_proj_weight: tensor not found in the model weights");
        if (!latent || !out || frames <= 0) throw Error(PTTS_EINVAL, strfmt("latent shape must be [1,T,%d], got [1 %lld %d]", l.in, (long long)frames, l.in));
        const Locked lock(m);
        staged_speaker_project(m, latent, frames, out);
    });
}

int ptts_mimi_encode(ptts_model* h, const float* const* pcm, const int64_t* n_samples, int32_t n_clips, float* const* latent_out) {
    return encode_stages(h, pcm, n_samples, n_clips, latent_out, nullptr);
}

int64_t ptts_mimi_encode_frames(int64_t n_samples) {
    if (n_samples < 0) return -PTTS_EINVAL;
    return (n_samples + 1919) / 1920;   // (every checkpoint this build loads has the decoder's 16 x 6 x 5 x 4 = 1920-sample frame; the encoder's hop must match)
}

int ptts_voice_encode_audio(ptts_model* h, const float* pcm, int64_t n_samples, float* embedding_out, int64_t* frames) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        Model& m = *h->m;
        require_voice_encoder(m.d);
        if (!embedding_out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        const Locked lock(m);
        const int64_t f = voice_embedding_device(m, pcm, n_samples, embedding_out);
        if (frames) *frames = f;
    });
}

int ptts_voice_from_embeddings(ptts_model* h, const float* const* emb, const int64_t* frames, int64_t width, int32_t n, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!out) throw Error(PTTS_EINVAL, "ptts-hip: voice build: null output array");
        Model& m = *h->m;
        const Locked lock(m);
        auto vs = voice_build(m, emb, frames, width, n);
        voices_out(vs, out);
    });
}

static void voice_from_audio(ptts_model* h, const float* const* pcm, const int64_t* n_samples, const int32_t* rates, int32_t n, ptts_voice** out) {
    if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
    Model& m = *h->m;
    require_voice_encoder(m.d);
    if (n <= 0) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice build needs at least one clip, got %d", n));
    if (!pcm || !n_samples || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
    const int64_t hop = m.d.enc.hop, D = m.d.d_model;
    const Locked lock(m);
    std::vector<std::vector<float>> embs((size_t)n);
    std::vector<const float*> ptrs((size_t)n);
    std::vector<int64_t> frames((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!pcm[i]) throw Error(PTTS_EINVAL, strfmt("ptts-hip: clip %d is null", i));
        const int rate = rates ? rates[i] : kNativeRate;
        const int64_t n24 = mimi_encode_samples(std::max<int64_t>(n_samples[i], 0), rate);
        embs[(size_t)i].resize((size_t)std::max<int64_t>((n24 + hop - 1) / hop, 1) * D);
        frames[(size_t)i] = voice_embedding_device(m, pcm[i], n_samples[i], embs[(size_t)i].data(), rate);
        ptrs[(size_t)i] = embs[(size_t)i].data();
    }
    auto vs = voice_build(m, ptrs.data(), frames.data(), D, n);
    voices_out(vs, out);
}

int ptts_voice_from_audio(ptts_model* h, const float* const* pcm, const int64_t* n_samples, int32_t n, ptts_voice** out) {
    return guard([&] { voice_from_audio(h, pcm, n_samples, nullptr, n, out); });
}

int ptts_voice_from_audio_rates(ptts_model* h, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates, int32_t n, ptts_voice** out) {
    return guard([&] { voice_from_audio(h, pcm, n_samples, sample_rates, n, out); });
}

int ptts_mimi_encode_rates(ptts_model* h, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates, int32_t n_clips, float* const* latent_out) {
    return encode_stages(h, pcm, n_samples, n_clips, latent_out, nullptr, sample_rates);
}

int ptts_voice_offset(const ptts_voice* v, int64_t* offset) {
    return guard([&] {
        if (!v || !offset) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        *offset = reinterpret_cast<const Voice*>(v)->offset;
    });
}

int ptts_voice_read_state(const ptts_voice* hv, int32_t layer, float* cache) {
    return guard([&] {
        if (!hv || !cache) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        const Voice& v = *reinterpret_cast<const Voice*>(hv);
        const Locked lock(*v.m);
        voice_read_state(v, layer, cache);
    });
}

int ptts_voice_write(const ptts_voice* v, const char* path) {
    return guard([&] {
        if (!path) throw Error(PTTS_EINVAL, "ptts-hip: null path");
        write_file(path, voice_file_bytes(v));
    });
}

int ptts_voice_write_bytes(const ptts_voice* v, uint8_t** data, size_t* len) {
    return guard([&] {
        if (!data || !len) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        bytes_out(voice_file_bytes(v), data, len);
    });
}

int ptts_voice_state_write_bytes(const float* const* caches, int64_t offset, int32_t n_layers, int32_t heads, int32_t head_dim, uint8_t** data, size_t* len) {
    return guard([&] {
        if (!data || !len) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        bytes_out(voice_state_file(caches, offset, n_layers, heads, head_dim), data, len);
    });
}

int ptts_voice_embedding_write(const float* emb, int64_t frames, int64_t dim, const char* path) {
    return guard([&] {
        if (!path) throw Error(PTTS_EINVAL, "ptts-hip: null path");
        write_file(path, voice_embedding_file(emb, frames, dim));
    });
}

void ptts_free_bytes(uint8_t* data) { free(data); }

int ptts_noise_rows(ptts_model* h, uint64_t seed, float temperature, int32_t rows, float* out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        if (rows <= 0) throw Error(PTTS_EINVAL, "native: invalid gaussian noise shape");
        Model& m = *h->m;
        const Locked lock(m);
        if (m.d.ldim % 4) throw Error(PTTS_EINVAL, "ptts-hip: the device noise draw needs a latent width that is a multiple of 4");
        staged_noise_rows(m, seed, temperature, rows, out);
    });
}

int ptts_flow_direction(ptts_model* h, const float* c, float sv, float tv, const float* x, int32_t n, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: flow_lm flow net unavailable");
        Model& m = *h->m;
        const Locked lock(m);
        staged_flow_direction(m, c, sv, tv, x, n, out);
    });
}

// Service.Synthesize's chunks as one utterance (service.go:107-153), finished on the device: generate_joined (generate.cpp)
int ptts_generate_joined(ptts_model* h, const ptts_request* reqs, int32_t n, const ptts_join_opts* o, ptts_result* out, ptts_join_part* parts) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        if (!reqs || !out || n <= 0) throw Error(PTTS_EINVAL, "ptts-hip: no requests");
        if (!o) throw Error(PTTS_EINVAL, "ptts-hip: join: null options");
        set_last_error("");
        generate_joined(*h->m, reqs, n, *o, nullptr, out, parts);
    });
}

// ... handed over group by group (generate.cpp JoinStream).  The stream options are checked first: their refusals need no model
int ptts_generate_joined_streamed(ptts_model* h, const ptts_request* reqs, int32_t n, const ptts_join_opts* o, const ptts_join_stream_opts* so, ptts_result* out,
                                  ptts_join_part* parts) {
    return guard([&] {
        const std::string e = join_stream_opts_error(so);
        if (!e.empty()) {   // *out and parts as generate_joined leaves them on a refusal
            if (out) { std::memset(out, 0, sizeof *out); out->eos_step = -1; out->status = PTTS_EINVAL; }
            for (int i = 0; parts && i < n && n <= kJoinMaxRows; i++) { std::memset(&parts[i], 0, sizeof parts[i]); parts[i].eos_step = -1; }
            throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        }
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        if (!reqs || !out || n <= 0) throw Error(PTTS_EINVAL, "ptts-hip: no requests");
        if (!o) throw Error(PTTS_EINVAL, "ptts-hip: join: null options");
        set_last_error("");
        ptts_join_stream_opts known{};   // (a newer caller's struct: the bytes this library knows)
        std::memcpy(&known, so, std::min<size_t>(so->size, sizeof known));
        generate_joined(*h->m, reqs, n, *o, &known, out, parts);
    });
}

// ... with one ptts_part_opts per part (generate.cpp JoinSink's per-part stages, seams and volumes).  so NULL: not streamed
int ptts_generate_joined_parts(ptts_model* h, const ptts_request* reqs, int32_t n, const ptts_join_opts* o, const ptts_part_opts* po, const ptts_join_stream_opts* so,
                               ptts_result* out, ptts_join_part* parts, float* gains) {
    return guard([&] {
        const std::string e = so ? join_stream_opts_error(so) : std::string();
        if (!e.empty() || !po) {   // *out and parts as generate_joined leaves them on a refusal
            if (out) { std::memset(out, 0, sizeof *out); out->eos_step = -1; out->status = PTTS_EINVAL; }
            for (int i = 0; parts && i < n && n <= kJoinMaxRows; i++) { std::memset(&parts[i], 0, sizeof parts[i]); parts[i].eos_step = -1; }
            throw Error(PTTS_EINVAL, "ptts-hip: " + (e.empty() ? std::string("join: parts: null list") : e));
        }
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        if (!reqs || !out || n <= 0) throw Error(PTTS_EINVAL, "ptts-hip: no requests");
        if (!o) throw Error(PTTS_EINVAL, "ptts-hip: join: null options");
        set_last_error("");
        ptts_join_stream_opts known{};   // (a newer caller's struct: the bytes this library knows)
        if (so) std::memcpy(&known, so, std::min<size_t>(so->size, sizeof known));
        const JoinPartsList list{po, gains};
        generate_joined(*h->m, reqs, n, *o, so ? &known : nullptr, out, parts, &list);
    });
}

}  // extern "C"
