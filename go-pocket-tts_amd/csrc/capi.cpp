// capi.cpp -- extern "C" surface of libptts_hip.so (include/ptts.h).
#include <cmath>
#include <map>

#include "runtime.h"

#include "capi_internal.h"
#include "eq.h"
#include "opts_check.h"

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

void ptts_wav_header_streaming(uint8_t out[44]) {   // internal/audio/wav_stream.go:15-41
    static const uint8_t hdr[44] = {'R', 'I', 'F', 'F', 0xFF, 0xFF, 0xFF, 0xFF, 'W', 'A', 'V', 'E', 'f', 'm', 't', ' ', 16, 0, 0, 0, 1, 0, 1, 0,
                                    0xC0, 0x5D, 0, 0 /* 24000 */, 0x80, 0xBB, 0, 0 /* 48000 B/s */, 2, 0, 16, 0, 'd', 'a', 't', 'a', 0xFF, 0xFF, 0xFF, 0xFF};
    memcpy(out, hdr, 44);
}

int ptts_voice_create(ptts_model* h, const float* const* caches, const int64_t* steps, const int64_t* offsets, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m || !out) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!caches || !steps || !offsets) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        std::lock_guard<std::mutex> lock(h->m->mu);
        h->m->use_device();
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
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
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
        Model& m = *h->m;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        PTTS_HIP(hipStreamSynchronize(m.stream));
        std::memset(out, 0, sizeof *out);
        double ms = 0;
        for (size_t i = 0; i + 1 < m.prof.used; i += 2) {
            float t = 0;
            PTTS_HIP(hipEventElapsedTime(&t, m.prof.ev[i], m.prof.ev[i + 1]));
            ms += t;
        }
        out->launches = m.prof.launches;
        out->total_ms = ms;
        out->algorithmic_bytes = m.prof.bytes;
        out->weight_bytes = m.prof.wbytes;
        if (m.prof.phases) {
            PTTS_HIP(hipStreamSynchronize(m.stream2));
            float t = 0;
            PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[0], m.prof.phase[1])); out->prefill_ms = t;
            PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[1], m.prof.phase[2])); out->ar_loop_ms = t;
            PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[3], m.prof.phase[4])); out->mimi_ms = t;
        }
        snprintf(out->kernel, sizeof out->kernel, "%s", "k_skinny");
        m.prof.used = 0; m.prof.bytes = 0; m.prof.wbytes = 0; m.prof.launches = 0; m.prof.phases = false;
    });
}

int ptts_text_embeddings(ptts_model* h, const int64_t* ids, int64_t n, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        Model& m = *h->m;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        for (int64_t i = 0; i < n; i++)
            if (ids[i] < 0 || ids[i] >= m.d.n_bins) throw Error(PTTS_EINVAL, strfmt("native: token id %lld (%lld) out of range [0,%d)", (long long)i, (long long)ids[i], m.d.n_bins));
        if (n == 0) return;
        DevBuf& dids = m.work(6, (size_t)n * sizeof(int64_t));
        DevBuf& rows = m.work(5, (size_t)n * m.d.d_model * sizeof(float));
        PTTS_HIP(hipMemcpyAsync(dids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, m.stream));
        launch_embed_gather(m.at<float>(m.d.embed), dids.as<int64_t>(), (int)n, m.d.d_model, rows.as<float>(), m.stream);
        PTTS_HIP(hipMemcpyAsync(out, rows.p, (size_t)n * m.d.d_model * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
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
        std::lock_guard<std::mutex> lock(b->m->mu);
        b->m->use_device();
        batch_reset(*b->b);
        PTTS_HIP(hipStreamSynchronize(b->m->stream));
    });
}

int ptts_batch_set_voice_state(ptts_batch* b, int32_t slot, const float* const* caches, const int64_t* steps, const int64_t* offsets) {
    return guard([&] {
        if (!b || !b->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        if (!caches || !steps || !offsets) throw Error(PTTS_EINVAL, "native: voice model state is nil");
        std::lock_guard<std::mutex> lock(b->m->mu);
        b->m->use_device();
        batch_set_voice(*b->b, slot, caches, steps, offsets);
    });
}

int ptts_batch_prompt(ptts_batch* b, const float* emb, const int64_t* row_offsets) {
    return guard([&] {
        if (!b || !b->b) throw Error(PTTS_EINVAL, "native: flow_lm state unavailable");
        if (!row_offsets) throw Error(PTTS_EINVAL, "native: prompt text embeddings are nil");
        Model& m = *b->m;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        int64_t R = row_offsets[b->b->B];
        if (R > 0 && !emb) throw Error(PTTS_EINVAL, "native: prompt text embeddings are nil");
        DevBuf& rows = m.work(5, (size_t)std::max<int64_t>(R, 1) * m.d.d_model * sizeof(float));
        if (R > 0) {
            PTTS_HIP(hipMemcpyAsync(rows.p, emb, (size_t)R * m.d.d_model * sizeof(float), hipMemcpyHostToDevice, m.stream));
            PTTS_HIP(hipStreamSynchronize(m.stream));
        }
        batch_prompt(*b->b, rows.as<float>(), row_offsets);
        PTTS_HIP(hipStreamSynchronize(m.stream));
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
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        hipStream_t s = m.stream;
        const int B = b.B, ld = m.d.ldim;
        for (int i = 0; i < B; i++)
            if (b.kv_len_host[i] + 1 > b.cap) throw Error(PTTS_EINVAL, "ptts-hip: KV capacity exhausted");
        m.tcomb_for(lsd_steps);
        PTTS_HIP(hipMemcpyAsync(b.in_raw.p, frames_in, (size_t)B * ld * sizeof(float), hipMemcpyHostToDevice, s));
        launch_replace_nan(b.in_raw.as<float>(), m.at<float>(m.d.bos), B, ld, b.in32.as<float>(), s);
        if (noise) PTTS_HIP(hipMemcpyAsync(b.cur.p, noise, (size_t)B * ld * sizeof(float), hipMemcpyHostToDevice, s));
        else PTTS_HIP(hipMemsetAsync(b.cur.p, 0, (size_t)B * ld * sizeof(float), s));
        // (the Euler state as the step found it: if a hand-off inside k_flow_cluster times out, the flow part of THIS step is re-issued from it as launches)
        if (b.fc_ok) PTTS_HIP(hipMemcpyAsync(b.cur2.p, b.cur.p, (size_t)B * ld * sizeof(float), hipMemcpyDeviceToDevice, s));
        const bool clustered = b.fc_ok;
        step_core(b, lsd_steps);
        if (clustered) {
            unsigned fault = 0;
            PTTS_HIP(hipMemcpyAsync(&fault, b.fc_fault(), sizeof fault, hipMemcpyDeviceToHost, s));
            PTTS_HIP(hipStreamSynchronize(s));
            if (fault) {   // transformer state (keys, values, `last`, the EOS logit) is untouched by the cluster: only the frame is redone
                flow_cluster_recover(b);
                PTTS_HIP(hipMemcpyAsync(b.cur.p, b.cur2.p, (size_t)B * ld * sizeof(float), hipMemcpyDeviceToDevice, s));
                step_flow_again(b, lsd_steps);
            }
        }
        for (int i = 0; i < B; i++) b.kv_len_host[i] += 1;
        PTTS_HIP(hipMemcpyAsync(b.st.kv_len, b.kv_len_host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (frames_out) PTTS_HIP(hipMemcpyAsync(frames_out, b.cur.p, (size_t)B * ld * sizeof(float), hipMemcpyDeviceToHost, s));
        if (eos_logits) PTTS_HIP(hipMemcpyAsync(eos_logits, b.eos.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
        if (last_hidden) PTTS_HIP(hipMemcpyAsync(last_hidden, b.last.p, (size_t)B * m.d.d_model * sizeof(float), hipMemcpyDeviceToHost, s));
        PTTS_HIP(hipStreamSynchronize(s));
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
        const Desc& d = m.d;
        if (slot < 0 || slot >= b.B || layer < 0 || layer >= d.n_layers) throw Error(PTTS_EINVAL, "ptts-hip: slot/layer out of range");
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const int n = b.kv_len_host[slot];
        const size_t es = b.kv_elem();
        std::vector<uint8_t> tmp((size_t)n * d.hd * es);
        for (int which = 0; which < 2; which++) {
            const char* base = (const char*)(which ? b.vc(layer) : b.kc(layer));
            float* dst = which ? v : k;
            for (int h = 0; h < d.heads; h++) {
                const char* src = base + (((size_t)slot * d.heads + h) * b.cap) * d.hd * es;
                PTTS_HIP(hipMemcpy(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost));
                float* o = dst + (size_t)h * n * d.hd;
                if (es == 4) std::memcpy(o, tmp.data(), tmp.size());
                else for (size_t i = 0; i < (size_t)n * d.hd; i++) { uint16_t bb; std::memcpy(&bb, tmp.data() + 2 * i, 2); o[i] = bf16_to_f32(bb); }
            }
        }
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
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
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
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const Desc& d = m.d;
        size_t nl = (size_t)n_utt * frames * d.ldim, np = (size_t)n_utt * frames * d.samples_per_frame, nm = (size_t)n_utt * d.mimi_dim * frames;
        size_t nx = transformer_out ? (size_t)n_utt * frames * d.up_stride * d.mimi_dim : 0;
        DevBuf& io = m.work(8, (nl + np + nm + nx) * sizeof(float));
        float* dl = io.as<float>();
        float* dp = dl + nl;
        float* dm = dp + np;
        float* dx = dm + nm;
        PTTS_HIP(hipMemcpyAsync(dl, latents, nl * sizeof(float), hipMemcpyHostToDevice, m.stream));
        mimi_decode(m, dl, (int64_t)frames * d.ldim, n_utt, frames, dp, mimi_latent ? dm : nullptr, transformer_out ? dx : nullptr);
        if (pcm) PTTS_HIP(hipMemcpyAsync(pcm, dp, np * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        if (mimi_latent) PTTS_HIP(hipMemcpyAsync(mimi_latent, dm, nm * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        if (transformer_out) PTTS_HIP(hipMemcpyAsync(transformer_out, dx, nx * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
    });
}

// encoder + speaker projection (EncodeVoice, onnx/voice_encode.go:23-158): PTTS_EFORMAT naming what the checkpoint lacks
static void require_voice_encoder(const Desc& d) {
    require_encoder(d);
    const Lin& l = d.speaker_proj;
    if (l.w == NONE) throw Error(PTTS_EFORMAT, "load speaker_proj_weight: tensor not found in the model weights");
    if (l.in != d.mimi_dim) throw Error(PTTS_EFORMAT, strfmt("speaker_proj_weight takes %d-wide latents, the encoder makes %d", l.in, d.mimi_dim));
}

// one clip -> its voice embedding in out (host, [ceil(n / hop)][d_model]); returns the frame count.  The caller holds m.mu.
static int64_t encode_embedding(Model& m, const float* pcm, int64_t n_samples, float* out, int rate = kNativeRate) {
    const Lin& l = m.d.speaker_proj;
    const int64_t n24 = mimi_encode_samples(std::max<int64_t>(n_samples, 0), rate);
    const int64_t nf = n24 > 0 ? (n24 + m.d.enc.hop - 1) / m.d.enc.hop : 0;
    DevBuf& io = m.work(17, (size_t)std::max<int64_t>(nf, 1) * (l.in + l.out) * sizeof(float));
    float* lat = io.as<float>();
    const int64_t f = mimi_encode_clip(m, pcm, n_samples, lat, nullptr, rate);
    float* dout = lat + (size_t)f * l.in;
    GemmArgs g;   // the product ptts_speaker_project runs, on the latents where the encoder left them
    g.A = lat; g.amap = RowMap{l.in, 0, 0};
    g.W = m.arena + l.w; g.w_bf16 = 0; g.ldw = l.in;
    g.C = dout; g.cmap = RowMap{l.out, 0, 0};
    g.M = (int)f; g.N = l.out; g.K = l.in;
    launch_gemm(g, m.stream);
    PTTS_HIP(hipMemcpyAsync(out, dout, (size_t)f * l.out * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
    return f;
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

// a device voice as a model-state file (the caller holds nothing; the voice's engine is locked here)
static std::vector<uint8_t> voice_file_bytes(const ptts_voice* hv) {
    if (!hv) throw Error(PTTS_EINVAL, "native: voice model state is nil");
    const Voice& v = *reinterpret_cast<const Voice*>(hv);
    Model& m = *v.m;
    const Desc& d = m.d;
    const size_t per = (size_t)2 * v.offset * d.heads * d.hd;
    std::vector<float> all(per * d.n_layers);
    {
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        voice_export(v, 0, d.n_layers, all.data());
    }
    std::vector<const float*> caches((size_t)d.n_layers);
    for (int l = 0; l < d.n_layers; l++) caches[(size_t)l] = all.data() + per * l;
    return voice_state_file(caches.data(), v.offset, d.n_layers, d.heads, d.hd);
}

extern "C" {

int ptts_speaker_project(ptts_model* h, const float* latent, int64_t frames, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        Model& m = *h->m;
        const Lin& l = m.d.speaker_proj;
        if (l.w == NONE) throw Error(PTTS_EFORMAT, "load speaker_proj_weight: tensor not found in the model weights");
        if (!latent || !out || frames <= 0) throw Error(PTTS_EINVAL, strfmt("latent shape must be [1,T,%d], got [1 %lld %d]", l.in, (long long)frames, l.in));
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const size_t ni = (size_t)frames * l.in, no = (size_t)frames * l.out;
        DevBuf& io = m.work(8, (ni + no) * sizeof(float));
        float* di = io.as<float>();
        float* dout = di + ni;
        PTTS_HIP(hipMemcpyAsync(di, latent, ni * sizeof(float), hipMemcpyHostToDevice, m.stream));
        GemmArgs g;
        g.A = di; g.amap = RowMap{l.in, 0, 0};
        g.W = m.arena + l.w; g.w_bf16 = 0; g.ldw = l.in;
        g.C = dout; g.cmap = RowMap{l.out, 0, 0};
        g.M = (int)frames; g.N = l.out; g.K = l.in;
        launch_gemm(g, m.stream);
        PTTS_HIP(hipMemcpyAsync(out, dout, no * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
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
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const int64_t f = encode_embedding(m, pcm, n_samples, embedding_out);
        if (frames) *frames = f;
    });
}

int ptts_voice_from_embeddings(ptts_model* h, const float* const* emb, const int64_t* frames, int64_t width, int32_t n, ptts_voice** out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model flow_lm unavailable");
        if (!out) throw Error(PTTS_EINVAL, "ptts-hip: voice build: null output array");
        Model& m = *h->m;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
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
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    std::vector<std::vector<float>> embs((size_t)n);
    std::vector<const float*> ptrs((size_t)n);
    std::vector<int64_t> frames((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!pcm[i]) throw Error(PTTS_EINVAL, strfmt("ptts-hip: clip %d is null", i));
        const int rate = rates ? rates[i] : kNativeRate;
        const int64_t n24 = mimi_encode_samples(std::max<int64_t>(n_samples[i], 0), rate);
        embs[(size_t)i].resize((size_t)std::max<int64_t>((n24 + hop - 1) / hop, 1) * D);
        frames[(size_t)i] = encode_embedding(m, pcm[i], n_samples[i], embs[(size_t)i].data(), rate);
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
        std::lock_guard<std::mutex> lock(v.m->mu);
        v.m->use_device();
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
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const int ld = m.d.ldim;
        if (ld % 4) throw Error(PTTS_EINVAL, "ptts-hip: the device noise draw needs a latent width that is a multiple of 4");
        NoiseSpec sp{seed, temperature > 0.0f ? std::sqrt(temperature) : 0.0f, rows};
        DevBuf& sb = m.work(12, sizeof sp);
        DevBuf& ob = m.work(8, (size_t)rows * ld * sizeof(float));
        PTTS_HIP(hipMemcpyAsync(sb.p, &sp, sizeof sp, hipMemcpyHostToDevice, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
        launch_noise_fill(sb.as<NoiseSpec>(), 1, rows, ob.as<float>(), (int64_t)rows * ld, ld, m.stream);
        PTTS_HIP(hipMemcpyAsync(out, ob.p, (size_t)rows * ld * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
    });
}

int ptts_flow_direction(ptts_model* h, const float* c, float sv, float tv, const float* x, int32_t n, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: flow_lm flow net unavailable");
        Model& m = *h->m;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        // one Euler step of size 1 starting from zero velocity accumulation: run step-core's flow part through a 1-slot-per-row batch
        const Desc& d = m.d;
        const int C = d.flow_dim, D = d.d_model, NA = d.ada_all.out, B = n;
        hipStream_t s = m.stream;
        DevBuf& wsb = m.work(9, ((size_t)B * (D + d.ldim + d.ldim + 4 * C + NA) + C) * sizeof(float));
        float* dc = wsb.as<float>();
        float* dx = dc + (size_t)B * D;
        float* dout = dx + (size_t)B * d.ldim;
        float* sy = dout + (size_t)B * d.ldim;
        float* fx = sy + (size_t)B * C;
        float* fh = fx + (size_t)B * C;
        float* fh2 = fh + (size_t)B * C;
        float* ada = fh2 + (size_t)B * C;
        float* tc = ada + (size_t)B * NA;
        PTTS_HIP(hipMemcpyAsync(dc, c, (size_t)B * D * sizeof(float), hipMemcpyHostToDevice, s));
        PTTS_HIP(hipMemcpyAsync(dx, x, (size_t)B * d.ldim * sizeof(float), hipMemcpyHostToDevice, s));
        PTTS_HIP(hipStreamSynchronize(s));
        m.compute_tcomb(sv, tv, tc);
        auto mkg = [&](const float* A, int64_t lda, const Lin& l, float* Cc, int64_t ldc) {
            GemmArgs g;
            g.A = A; g.amap = RowMap{lda, 0, 0};
            g.W = m.arena + l.w; g.w_bf16 = l.bf16; g.ldw = l.in; g.bias = m.at<float>(l.b);
            g.wt_i8 = l.wt_i8; g.wscale = m.at<float>(l.wscale);
            g.C = Cc; g.cmap = RowMap{ldc, 0, 0};
            g.M = B; g.N = l.out; g.K = l.in;
            return g;
        };
        GemmArgs gc = mkg(dc, D, d.cond_embed, sy, C);
        gc.epi = EPI_SILU; gc.addvec = tc;
        launch_gemm(gc, s);
        launch_gemm(mkg(sy, C, d.ada_all, ada, NA), s);
        launch_gemm(mkg(dx, d.ldim, d.input_proj, fx, C), s);
        for (int r = 0; r < d.flow_depth; r++) {
            const auto& rb = d.rb[r];
            LnArgs ln;
            ln.x = fx; ln.xmap = RowMap{C, 0, 0}; ln.w = m.at<float>(rb.ln.w); ln.b = m.at<float>(rb.ln.b); ln.eps = rb.ln.eps;
            ln.y = fh; ln.ldy = C; ln.rows = B; ln.d = C;
            ln.shift = ada + (size_t)r * 3 * C; ln.scale = ln.shift + C; ln.ldmod = NA;
            launch_layernorm(ln, s);
            GemmArgs g0 = mkg(fh, C, rb.mlp0, fh2, C);
            g0.epi = EPI_SILU;
            launch_gemm(g0, s);
            GemmArgs g2 = mkg(fh2, C, rb.mlp2, fx, C);
            g2.R = fx; g2.epi = EPI_GATE_RESADD; g2.gate = ada + (size_t)r * 3 * C + 2 * C; g2.ldg = NA;
            launch_gemm(g2, s);
        }
        LnArgs lf;
        lf.x = fx; lf.xmap = RowMap{C, 0, 0}; lf.eps = 1e-6f; lf.y = fh; lf.ldy = C; lf.rows = B; lf.d = C;
        lf.shift = ada + (size_t)d.flow_depth * 3 * C; lf.scale = lf.shift + C; lf.ldmod = NA;
        launch_layernorm(lf, s);
        launch_gemm(mkg(fh, C, d.final_linear, dout, d.ldim), s);
        PTTS_HIP(hipMemcpyAsync(out, dout, (size_t)B * d.ldim * sizeof(float), hipMemcpyDeviceToHost, s));
        PTTS_HIP(hipStreamSynchronize(s));
    });
}

// ---- kernel-level entry points ----

int ptts_op_linear(const float* x, const float* w, const float* bias, int64_t rows, int64_t in, int64_t out, float* y) {
    return guard([&] {
        require_device();
        if (!x || !w || !y) throw Error(PTTS_EINVAL, "tensor: linear requires non-nil x and weight");
        Tmp dx((size_t)rows * in * 4), dw((size_t)out * in * 4), db((size_t)out * 4), dy((size_t)rows * out * 4);
        up(dx.p, x, (size_t)rows * in * 4); up(dw.p, w, (size_t)out * in * 4);
        if (bias) up(db.p, bias, (size_t)out * 4);
        GemmArgs g;
        g.A = dx.as<float>(); g.amap = RowMap{in, 0, 0};
        g.W = dw.p; g.ldw = in; g.bias = bias ? db.as<float>() : nullptr;
        g.C = dy.as<float>(); g.cmap = RowMap{out, 0, 0};
        g.M = (int)rows; g.N = (int)out; g.K = (int)in;
        launch_gemm(g, nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        down(y, dy.p, (size_t)rows * out * 4);
    });
}

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

// n host rows -> n host rows through one device buffer each way (runtime.h PackedRows), one k_resample launch per RowRing::kRows rows
static void device_convert(Model& m, const float* const* in, const int64_t* n_in, int32_t n, const RateFilter* f, const int64_t* n_out, int fmt,
                           void* const* out) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> ib((size_t)n), ob((size_t)n);
    for (int i = 0; i < n; i++) {
        ib[(size_t)i] = (size_t)n_in[i] * sizeof(float);
        ob[(size_t)i] = (size_t)n_out[i] * pcm_bytes(fmt);
    }
    PackedRows di(m, WORK_CONVERT_IN, std::move(ib)), dout(m, WORK_CONVERT_OUT, std::move(ob));
    std::vector<ResampleRow> rows;
    for (int i = 0; i < n; i++) {
        if (n_in[i] > 0) di.upload(i, in[i], s);
        if (n_out[i] > 0) rows.push_back(resample_row(f, (const float*)di.row(i), n_in[i], dout.row(i), 0, n_out[i], fmt));
    }
    resample_launch(m, rows, s);
    for (int i = 0; i < n; i++)
        if (n_out[i] > 0) dout.download(i, out[i], s);
    PTTS_HIP(hipStreamSynchronize(s));
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
        const RateFilter* f;
        {
            std::lock_guard<std::mutex> lock(m.mu);
            m.use_device();
            f = rate_filter(m, in_rate, out_rate, m.stream);
        }
        device_convert(m, in, n_in, n, f, n_out.data(), RS_F32, (void* const*)out);
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

// The host-rows entry points with one stage and one option per row (ptts_eq_rows, ptts_compress_rows, ptts_limit_rows): the argument checks
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
int ptts_pitch_rows(ptts_model* h, const ptts_pitch_opts* const* p, const ptts_tempo_opts* const* t, const float* const* in, const int64_t* n, int32_t rows,
                    float* const* out, int64_t* n_out) {
    std::vector<PitchScan> pitches;
    std::vector<TempoScan> tempos;
    return part_rows(h, "pitch", !p || !t || !n_out, in, n, rows, out, n_out, nullptr, [&](int i, PartStages& st) {
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
    }, pitches, tempos);
}

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
        device_convert(m, &in, &n, 1, nullptr, &n, pcm_format, &out);
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

int ptts_op_pcm16(const float* samples, int64_t n, int16_t* out) {
    return guard([&] {
        require_device();
        if (n < 0 || (n > 0 && (!samples || !out))) throw Error(PTTS_EINVAL, "audio: pcm16 requires non-nil buffers");
        if (n == 0) return;
        Tmp dx((size_t)n * 4), dy((size_t)n * 2);
        up(dx.p, samples, (size_t)n * 4);
        launch_pcm16(dx.as<float>(), dy.as<int16_t>(), n, nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        down(out, dy.p, (size_t)n * 2);
    });
}

int ptts_op_layernorm(const float* x, const float* w, const float* b, float eps, int64_t rows, int64_t d, float* y) {
    return guard([&] {
        require_device();
        if (!x || !y) throw Error(PTTS_EINVAL, "tensor: layernorm input is nil");
        if (eps <= 0) throw Error(PTTS_EINVAL, "tensor: layernorm eps must be > 0");
        if (d <= 0) throw Error(PTTS_EINVAL, "tensor: layernorm last dimension must be > 0");
        Tmp dx((size_t)rows * d * 4), dw((size_t)d * 4), db((size_t)d * 4), dy((size_t)rows * d * 4);
        up(dx.p, x, (size_t)rows * d * 4);
        if (w) up(dw.p, w, (size_t)d * 4);
        if (b) up(db.p, b, (size_t)d * 4);
        LnArgs a;
        a.x = dx.as<float>(); a.xmap = RowMap{d, 0, 0};
        a.w = w ? dw.as<float>() : nullptr; a.b = b ? db.as<float>() : nullptr; a.eps = eps;
        a.y = dy.as<float>(); a.ldy = d; a.rows = (int)rows; a.d = (int)d;
        launch_layernorm(a, nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        down(y, dy.p, (size_t)rows * d * 4);
    });
}

int ptts_op_rope(float* x, const float* cos_t, const float* sin_t, int64_t table_rows, int64_t prefix, int64_t seq, int64_t dim, int64_t pos) {
    return guard([&] {
        require_device();
        if (!x || !cos_t || !sin_t) throw Error(PTTS_EINVAL, "ops: rope requires non-nil x/cos/sin");
        if (pos < 0) throw Error(PTTS_EINVAL, "ops: rope position must be >= 0");
        if (dim % 2) throw Error(PTTS_EINVAL, strfmt("ops: rope last dimension must be even, got %lld", (long long)dim));
        if (table_rows < pos + seq) throw Error(PTTS_EINVAL, strfmt("ops: rope cos/sin sequence length too small for pos=%lld seq=%lld", (long long)pos, (long long)seq));
        size_t n = (size_t)prefix * seq * dim, tn = (size_t)table_rows * (dim / 2);
        Tmp dx(n * 4), dc(tn * 4), ds(tn * 4);
        up(dx.p, x, n * 4); up(dc.p, cos_t, tn * 4); up(ds.p, sin_t, tn * 4);
        launch_rope_rows(dx.as<float>(), RowMap{dim, 0, 0}, 0, 1, (int)dim, nullptr, (int)pos, (int)seq, (int)(prefix * seq), dc.as<float>(), ds.as<float>(), nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        down(x, dx.p, n * 4);
    });
}

int ptts_op_attention_positions(const float* q, const float* k, const float* v, int64_t b, int64_t h, int64_t tq, int64_t tk,
                                int64_t d, const int64_t* posq, const int64_t* posk, int64_t context, float* out) {
    return guard([&] {
        require_device();
        if (!q || !k || !v || !out) throw Error(PTTS_EINVAL, "ops: attention with positions requires non-nil q/k/v");
        if (b <= 0 || h <= 0 || tq <= 0 || tk <= 0 || d <= 0) throw Error(PTTS_EINVAL, "ops: attention expects positive dims");
        if (d > 64) throw Error(PTTS_EINVAL, "ptts-hip: attention kernels are built for head_dim <= 64");
        // cache-slot semantics of the reference's callers (flow_transformer.go:391-420): slot j holds position j or is invalid
        for (int64_t j = 0; j < tk; j++)
            if (posk[j] != -1 && posk[j] != j) throw Error(PTTS_EINVAL, "ptts-hip: posK must be the slot index or -1");
        for (int64_t i = 0; i < tq; i++) {
            int64_t lo = context >= 0 ? std::max<int64_t>(0, posq[i] - context + 1) : 0;
            for (int64_t j = lo; j <= std::min<int64_t>(posq[i], tk - 1); j++)
                if (posk[j] < 0) throw Error(PTTS_EINVAL, "ptts-hip: an invalid key inside a query window is not representable");
            if (posq[i] >= tk) throw Error(PTTS_EINVAL, "ptts-hip: query position beyond the key slots");
        }
        const int HD = 64;
        auto pad = [&](const float* src, int64_t rows) {  // zero-pad head_dim to 64 (dot products are unchanged)
            std::vector<float> o((size_t)rows * HD, 0.0f);
            for (int64_t r = 0; r < rows; r++) for (int64_t e = 0; e < d; e++) { float val = src[r * d + e]; o[(size_t)r * HD + e] = std::isnan(val) ? 0.0f : val; }
            return o;
        };
        // NaN in never-visible slots is allowed by the reference (masked before the dot product); padding drops it too
        std::vector<float> qp = pad(q, b * h * tq), kp = pad(k, b * h * tk), vp = pad(v, b * h * tk);
        const float fix = std::sqrt(64.0f / (float)d);  // kernel scales by 1/sqrt(64); the reference by 1/sqrt(d)
        for (auto& e : qp) e *= fix;
        std::vector<int32_t> pq((size_t)(b * h * tq)), sg((size_t)(b * h * tq));
        Tmp dq(qp.size() * 4), dk(kp.size() * 4), dv(vp.size() * 4), dout((size_t)b * h * tq * HD * 4), dpos(pq.size() * 4), dseg(sg.size() * 4);
        for (int64_t bh = 0; bh < b * h; bh++) for (int64_t i = 0; i < tq; i++) { pq[(size_t)(bh * tq + i)] = (int32_t)posq[i]; sg[(size_t)(bh * tq + i)] = (int32_t)bh; }
        up(dq.p, qp.data(), qp.size() * 4); up(dk.p, kp.data(), kp.size() * 4); up(dv.p, vp.data(), vp.size() * 4);
        up(dpos.p, pq.data(), pq.size() * 4); up(dseg.p, sg.data(), sg.size() * 4);
        AttnArgs a;
        a.q = dq.as<float>(); a.q_ld = HD; a.q_col0 = 0;
        a.k = dk.p; a.v = dv.p;
        a.k_seg_stride = tk * HD; a.k_head_stride = 0; a.k_row_stride = HD;
        a.row_seg = dseg.as<int32_t>(); a.row_pos = dpos.as<int32_t>();
        a.context = (int)context;
        a.out = dout.as<float>(); a.out_ld = HD;
        a.rows = (int)(b * h * tq); a.heads = 1; a.max_keys = (int)tk;
        // Self-attention over a whole sequence with a context window -- positions 0..T-1 on both sides, every slot valid: the
        // call shape of mimiTransformerLayer.selfAttention (mimi.go:365-441).  Implicit positions and segments, so that the
        // launch takes the Mimi decoder's own kernel (k_attn_window) and the reference's context-window tests exercise it.
        bool plain_window = context > 0 && tq == tk;
        for (int64_t i = 0; i < tq && plain_window; i++) plain_window = posq[i] == i && posk[i] == i;
        if (plain_window) {
            a.row_seg = nullptr; a.row_pos = nullptr;
            a.rows_per_seg = (int)tq;
            a.max_keys = (int)std::min<int64_t>(tk, context);
        }
        launch_attention(a, nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        std::vector<float> op((size_t)b * h * tq * HD);
        down(op.data(), dout.p, op.size() * 4);
        for (int64_t r = 0; r < b * h * tq; r++) for (int64_t e = 0; e < d; e++) out[r * d + e] = op[(size_t)r * HD + e];
    });
}

int ptts_op_conv1d_leftpad(const float* x, const float* w, const float* bias, int64_t b, int64_t cin, int64_t len, int64_t cout,
                           int64_t k, float* y) {
    return guard([&] {
        require_device();
        if (!x || !w || !y) throw Error(PTTS_EINVAL, "ops: conv1d requires non-nil input/kernel");
        if (b <= 0 || cin <= 0 || len <= 0 || cout <= 0 || k <= 0) throw Error(PTTS_EINVAL, "ops: conv1d expects positive dims");
        const int64_t P = k - 1;
        std::vector<float> wg((size_t)cout * cin * k);  // [oc][kx*Cin + ic]  (same repack as model.cpp conv_as_gemm)
        for (int64_t o = 0; o < cout; o++) for (int64_t c = 0; c < cin; c++) for (int64_t xk = 0; xk < k; xk++) wg[(size_t)(o * cin * k + xk * cin + c)] = w[(o * cin + c) * k + xk];
        Tmp dx((size_t)b * cin * len * 4), dxc((size_t)b * (P + len) * cin * 4), dw(wg.size() * 4), db((size_t)cout * 4),
            dyc((size_t)b * len * cout * 4), dy((size_t)b * cout * len * 4);
        up(dx.p, x, (size_t)b * cin * len * 4); up(dw.p, wg.data(), wg.size() * 4);
        if (bias) up(db.p, bias, (size_t)cout * 4);
        PTTS_HIP(hipMemset(dxc.p, 0, (size_t)b * (P + len) * cin * 4));
        launch_bct_to_btc(dx.as<float>(), (int)b, (int)cin, (int)len, dxc.as<float>(), (int)P, nullptr);
        GemmArgs g;
        g.A = dxc.as<float>(); g.amap = RowMap{cin, len, (P + len) * cin};
        g.W = dw.p; g.ldw = cin * k; g.bias = bias ? db.as<float>() : nullptr;
        g.C = dyc.as<float>(); g.cmap = RowMap{cout, 0, 0};
        g.M = (int)(b * len); g.N = (int)cout; g.K = (int)(cin * k);
        launch_gemm(g, nullptr);
        launch_btc_to_bct(dyc.as<float>(), 0, (int)b, (int)cout, (int)len, dy.as<float>(), nullptr);
        PTTS_HIP(hipDeviceSynchronize());
        down(y, dy.p, (size_t)b * cout * len * 4);
    });
}

int ptts_op_convtr1d_righttrim(const float* x, const float* w, const float* bias, int64_t b, int64_t cin, int64_t len,
                               int64_t opg, int64_t k, int64_t stride, int64_t groups, float* y) {
    return guard([&] {
        require_device();
        if (!x || !w || !y) throw Error(PTTS_EINVAL, "ops: convtranspose1d requires non-nil input/kernel");
        if (stride <= 0 || groups <= 0) throw Error(PTTS_EINVAL, "ops: convtranspose1d stride/dilation/groups must be > 0");
        if (k != 2 * stride) throw Error(PTTS_EINVAL, "ptts-hip: transposed convolutions are built for kernel = 2*stride");
        const int64_t lout = len * stride;
        if (groups == 1) {
            const int64_t cout = opg;
            std::vector<float> wg((size_t)stride * cout * 2 * cin), bg((size_t)stride * cout, 0.0f);
            for (int64_t r = 0; r < stride; r++) for (int64_t o = 0; o < cout; o++) {
                for (int64_t c = 0; c < cin; c++) {
                    wg[(size_t)((r * cout + o) * 2 * cin + c)] = w[(c * cout + o) * k + r + stride];
                    wg[(size_t)((r * cout + o) * 2 * cin + cin + c)] = w[(c * cout + o) * k + r];
                }
                if (bias) bg[(size_t)(r * cout + o)] = bias[o];
            }
            Tmp dx((size_t)b * cin * len * 4), dxc((size_t)b * (1 + len) * cin * 4), dw(wg.size() * 4), db(bg.size() * 4),
                dyc((size_t)b * lout * cout * 4), dy((size_t)b * cout * lout * 4);
            up(dx.p, x, (size_t)b * cin * len * 4); up(dw.p, wg.data(), wg.size() * 4); up(db.p, bg.data(), bg.size() * 4);
            PTTS_HIP(hipMemset(dxc.p, 0, (size_t)b * (1 + len) * cin * 4));
            launch_bct_to_btc(dx.as<float>(), (int)b, (int)cin, (int)len, dxc.as<float>(), 1, nullptr);
            GemmArgs g;
            g.A = dxc.as<float>(); g.amap = RowMap{cin, len, (1 + len) * cin};
            g.W = dw.p; g.ldw = 2 * cin; g.bias = db.as<float>();
            g.C = dyc.as<float>(); g.cmap = RowMap{stride * cout, 0, 0};
            g.M = (int)(b * len); g.N = (int)(stride * cout); g.K = (int)(2 * cin);
            launch_gemm(g, nullptr);
            launch_btc_to_bct(dyc.as<float>(), 0, (int)b, (int)cout, (int)lout, dy.as<float>(), nullptr);
            PTTS_HIP(hipDeviceSynchronize());
            down(y, dy.p, (size_t)b * cout * lout * 4);
            return;
        }
        if (groups == cin && opg == 1) {
            std::vector<float> w0((size_t)stride * cin), w1((size_t)stride * cin);
            for (int64_t r = 0; r < stride; r++) for (int64_t c = 0; c < cin; c++) { w0[(size_t)(r * cin + c)] = w[c * k + r + stride]; w1[(size_t)(r * cin + c)] = w[c * k + r]; }
            Tmp dx((size_t)b * cin * len * 4), dxc((size_t)b * (1 + len) * cin * 4), d0(w0.size() * 4), d1(w1.size() * 4), db((size_t)cin * 4),
                dyc((size_t)b * lout * cin * 4), dy((size_t)b * cin * lout * 4);
            up(dx.p, x, (size_t)b * cin * len * 4); up(d0.p, w0.data(), w0.size() * 4); up(d1.p, w1.data(), w1.size() * 4);
            if (bias) up(db.p, bias, (size_t)cin * 4);
            PTTS_HIP(hipMemset(dxc.p, 0, (size_t)b * (1 + len) * cin * 4));
            launch_bct_to_btc(dx.as<float>(), (int)b, (int)cin, (int)len, dxc.as<float>(), 1, nullptr);
            launch_upsample_depthwise(dxc.as<float>(), d0.as<float>(), d1.as<float>(), bias ? db.as<float>() : nullptr, (int)b, (int)len, 0, (int)len,
                                      (int)cin, (int)stride, dyc.as<float>(), 0, nullptr);
            launch_btc_to_bct(dyc.as<float>(), 0, (int)b, (int)cin, (int)lout, dy.as<float>(), nullptr);
            PTTS_HIP(hipDeviceSynchronize());
            down(y, dy.p, (size_t)b * cin * lout * 4);
            return;
        }
        throw Error(PTTS_EINVAL, "ptts-hip: transposed convolution supports groups == 1 or depthwise (groups == in_channels)");
    });
}

}  // extern "C"
