// generate.cpp -- engine: request staging and result delivery, GenerateAudio for a batch of chunks (generate), a text's chunks as one utterance
// (generate_joined).
#include "runtime.h"

#include <chrono>

#include <algorithm>
#include <cmath>

namespace ptts {

// ------------------------------------------------------------------------------------------------
// request staging and result delivery, shared by generate() and the continuous batch (continuous.cpp)
// ------------------------------------------------------------------------------------------------
void stage_prompt(Batch& b, const std::vector<SlotReq>& list, hipStream_t s, hipEvent_t before_prefill) {
    Model& m = *b.m;
    const int D = m.d.d_model;
    std::map<const Voice*, std::vector<int32_t>> by_voice;
    for (const SlotReq& q : list) {
        if (q.req->voice) by_voice[reinterpret_cast<const Voice*>(q.req->voice)].push_back(q.slot);
        else if (q.req->voice_caches) batch_set_voice(b, q.slot, q.req->voice_caches, q.req->voice_cache_steps, q.req->voice_offsets);
    }
    for (auto& kv : by_voice) batch_apply_voice(b, *kv.first, kv.second);
    // text (+ voice) embeddings packed as rows (runtime_native_safetensors.go:89-119); the slots not listed have empty segments
    std::vector<int64_t> row_off((size_t)b.B + 1, 0), ids;
    for (const SlotReq& q : list) {
        row_off[(size_t)q.slot + 1] = q.req->n_tokens + (q.req->voice_embedding ? q.req->voice_frames : 0);
        ids.insert(ids.end(), q.req->tokens, q.req->tokens + q.req->n_tokens);
    }
    for (int sl = 0; sl < b.B; sl++) row_off[(size_t)sl + 1] += row_off[(size_t)sl];
    DevBuf& rows = m.work(WORK_PROMPT_ROWS, (size_t)row_off[(size_t)b.B] * D * sizeof(float));
    DevBuf& dids = m.work(WORK_PROMPT_IDS, ids.size() * sizeof(int64_t));
    h2d(dids.p, ids.data(), ids.size() * sizeof(int64_t), s);
    // token rows of consecutive requests are contiguous unless a voice embedding sits between them: one gather per such run
    // (a batch without voice embeddings is ONE launch instead of one per request)
    int64_t id0 = 0, run_id0 = 0, run_n = 0;
    float* run_dst = rows.as<float>();
    auto flush = [&]() {
        if (run_n > 0) launch_embed_gather(m.at<float>(m.d.embed), dids.as<int64_t>() + run_id0, (int)run_n, D, run_dst, s);
        run_n = 0;
    };
    for (const SlotReq& q : list) {
        const ptts_request& r = *q.req;
        float* dst = rows.as<float>() + row_off[(size_t)q.slot] * D;
        const int64_t tv = r.voice_embedding ? r.voice_frames : 0;
        if (tv) {
            flush();
            h2d(dst, r.voice_embedding, (size_t)tv * D * sizeof(float), s);
        }
        if (run_n == 0) { run_id0 = id0; run_dst = dst + tv * D; }
        run_n += r.n_tokens;
        id0 += r.n_tokens;
    }
    flush();
    if (before_prefill) PTTS_HIP(hipEventRecord(before_prefill, s));
    batch_prompt(b, rows.as<float>(), row_off.data());
}

void stage_noise(Batch& b, const std::vector<SlotReq>& list, hipStream_t s) {
    Model& m = *b.m;
    const int ld = m.d.ldim;
    const int64_t slot_rows = (int64_t)b.max_steps * ld;
    float* noise = b.noise.as<float>();
    for (size_t i = 0; i < list.size();) {   // one memset per run of consecutive slots
        size_t j = i + 1;
        while (j < list.size() && list[j].slot == list[j - 1].slot + 1) j++;
        PTTS_HIP(hipMemsetAsync(noise + list[i].slot * slot_rows, 0, (j - i) * slot_rows * sizeof(float), s));
        i = j;
    }
    std::vector<NoiseSpec> spec((size_t)b.B, NoiseSpec{0, 0.0f, 0});
    int draw_rows = 0;
    for (const SlotReq& q : list) {
        const ptts_request& r = *q.req;
        if (r.noise) h2d(noise + q.slot * slot_rows, r.noise, (size_t)q.max_steps * ld * sizeof(float), s);
        else if (r.temperature > 0.0f) {
            if (ld % 4) throw Error(PTTS_EINVAL, "ptts-hip: the device noise draw needs a latent width that is a multiple of 4");
            spec[(size_t)q.slot] = NoiseSpec{r.noise_seed ? r.noise_seed : m.next_noise_seed(), std::sqrt(r.temperature), q.max_steps};
            draw_rows = std::max(draw_rows, q.max_steps);
        }
    }
    if (draw_rows == 0) return;
    DevBuf& sb = m.work(WORK_NOISE_SPECS, spec.size() * sizeof(NoiseSpec));
    h2d(sb.p, spec.data(), spec.size() * sizeof(NoiseSpec), s);
    launch_noise_fill(sb.as<NoiseSpec>(), b.B, draw_rows, noise, slot_rows, ld, s);
}

const PcmRow* results_alloc(const Model& m, const std::vector<Delivery>& g, PcmRow* host_rows, PcmRow* dev_rows, hipStream_t s) {
    const int64_t spf = m.d.samples_per_frame;
    bool all_pinned = true, converts = false;
    for (size_t i = 0; i < g.size(); i++) {
        if (host_rows) host_rows[i] = PcmRow{nullptr, 0, 0};
        const Delivery& u = g[i];
        if (!u.res || u.filled) continue;
        const int fmt = u.req->pcm_format;
        const bool s16 = fmt == PTTS_PCM_S16;
        const int64_t ns = egress_length(*u.req, u.samples(spf));
        void* p = result_alloc((size_t)std::max<int64_t>(1, ns) * pcm_bytes(fmt));
        set_result_buffer(*u.res, fmt, p);
        if (!p) continue;
        all_pinned = all_pinned && result_is_pinned(p);
        converts = converts || request_converts(*u.req);
        if (host_rows) host_rows[i] = PcmRow{p, (int32_t)std::min<int64_t>(ns, INT32_MAX), s16 ? 1 : 0};
    }
    // a group with rows at another rate or in G.711 is decoded into the device buffer: results_deliver converts those rows from there
    if (!host_rows || !dev_rows || !all_pinned || converts) return nullptr;
    PTTS_HIP(hipMemcpyAsync(dev_rows, host_rows, g.size() * sizeof(PcmRow), hipMemcpyHostToDevice, s));   // page-locked source: no wait needed
    return dev_rows;
}

void results_deliver(Model& m, const std::vector<Delivery>& g, bool stored, const float* pcm, int64_t pcm_stride, const float* lat, int64_t lat_stride,
                     hipStream_t s) {
    const int ld = m.d.ldim;
    const int64_t spf = m.d.samples_per_frame;
    const int64_t n = (int64_t)g.size();
    const int16_t* pcm16 = nullptr;   // PCM16 egress on the device (audio/wav_stream.go:43-54), converted for the whole group at the first request that asks for it
    std::vector<int64_t> conv;        // rows at another rate or in G.711: one k_resample launch for all of them
    if (!stored) {   // post-processing (ptts_request.dsp, .loudness): every such row of the group at once, in place in the decoder's buffer, in front of the egress
        std::vector<DspJob> jobs;
        for (int64_t i = 0; i < n; i++) {
            const Delivery& u = g[(size_t)i];
            if (u.res && !u.filled && u.samples(spf) > 0 && (u.req->dsp || u.req->loudness) && result_buffer(*u.res, u.req->pcm_format)) {
                // resolved now, not at admission: a handle freed since the request was checked ends the call with PTTS_EINVAL, nothing is launched
                // (whether the row has work is asked of the resolved spec; request_postprocesses, which counts an ext unseen, has kept every
                // such request away from the decoder's direct store, so `stored` is false for a group that holds one)
                DspJob j{const_cast<float*>(pcm) + i * pcm_stride, u.samples(spf), DspSpec()};
                const std::string e = dsp_resolve(u.req->dsp, &j.spec);
                if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
                const double target_lufs = (double)u.req->loudness / 100.0;   // 0.01 LUFS
                if (u.req->loudness) dsp_spec_loudness(j.spec, &target_lufs);
                if (j.spec.any()) jobs.push_back(j);
            }
        }
        if (!jobs.empty()) dsp_launch(m, jobs, s);
    }
    for (int64_t i = 0; i < n; i++) {
        const Delivery& u = g[(size_t)i];
        if (!u.res) continue;
        ptts_result& r = *u.res;
        const int fmt = u.req->pcm_format;
        r.n_frames = u.nf; r.eos_step = u.eos; r.n_samples = egress_length(*u.req, u.samples(spf));
        const bool s16 = fmt == PTTS_PCM_S16;
        if (!result_buffer(r, fmt)) { r.status = PTTS_ENOMEM; continue; }
        if (!stored && !u.filled && r.n_samples > 0) {   // all copies are queued back to back: the caller waits once
            if (request_converts(*u.req)) conv.push_back(i);
            else {
                if (s16 && !pcm16) {
                    DevBuf& buf = m.work(WORK_EGRESS_S16, (size_t)(n * pcm_stride) * sizeof(int16_t));
                    launch_pcm16(pcm, buf.as<int16_t>(), n * pcm_stride, s);
                    pcm16 = buf.as<int16_t>();
                }
                if (s16) PTTS_HIP(hipMemcpyAsync(r.pcm16, pcm16 + i * pcm_stride, (size_t)r.n_samples * sizeof(int16_t), hipMemcpyDeviceToHost, s));
                else PTTS_HIP(hipMemcpyAsync(r.pcm, pcm + i * pcm_stride, (size_t)r.n_samples * sizeof(float), hipMemcpyDeviceToHost, s));
            }
        }
        if (u.req->want_latents) {
            r.latents = (float*)malloc((size_t)std::max(1, u.nf) * ld * sizeof(float));
            if (!r.latents) { r.status = PTTS_ENOMEM; continue; }
            if (u.nf > 0) PTTS_HIP(hipMemcpyAsync(r.latents, lat + i * lat_stride, (size_t)u.nf * ld * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        r.status = PTTS_OK;
    }
    if (conv.empty()) return;
    // k_resample stores straight into page-locked result buffers (like the decoder's direct store); a pageable one gets a device row and a copy
    size_t scratch = 0;
    for (int64_t i : conv) {
        const ptts_result& r = *g[(size_t)i].res;
        const int fmt = g[(size_t)i].req->pcm_format;
        if (!result_is_pinned(result_buffer(r, fmt))) scratch += ((size_t)r.n_samples * pcm_bytes(fmt) + 255) & ~(size_t)255;
    }
    char* sb = scratch ? m.work(WORK_EGRESS_PAGEABLE, scratch).as<char>() : nullptr;
    std::vector<ResampleRow> rows;
    std::vector<std::pair<void*, const void*>> copies;
    std::vector<size_t> copy_bytes;
    for (int64_t i : conv) {
        const Delivery& u = g[(size_t)i];
        const ptts_result& r = *u.res;
        const int fmt = u.req->pcm_format;
        void* dst = result_buffer(r, fmt);
        if (!result_is_pinned(dst)) {
            const size_t bytes = (size_t)r.n_samples * pcm_bytes(fmt);
            copies.emplace_back(dst, sb);
            copy_bytes.push_back(bytes);
            dst = sb;
            sb += (bytes + 255) & ~(size_t)255;
        }
        rows.push_back(resample_row(rate_filter(m, kNativeRate, request_rate(*u.req), s), pcm + i * pcm_stride, u.samples(spf), dst, 0, r.n_samples, fmt));
    }
    resample_launch(m, rows, s);
    for (size_t k = 0; k < copies.size(); k++)
        PTTS_HIP(hipMemcpyAsync(copies[k].first, copies[k].second, copy_bytes[k], hipMemcpyDeviceToHost, s));
}

// ------------------------------------------------------------------------------------------------
// GenerateAudio for a batch of independent utterance chunks
// ------------------------------------------------------------------------------------------------
int resolve_max_steps(const ptts_request& r) {  // runtime_native_safetensors.go:61-67, text/prepare.go:38-48
    int ms = r.max_steps;
    if (ms <= 0) ms = r.estimated_max_steps;
    if (ms <= 0) ms = (int)std::ceil(((double)r.n_tokens / 3.0 + 2.0) * 12.5);
    return ms;
}

namespace {
// What the groups of one generate_joined call share: the text's joined row on the device (WORK_JOINED, sized for the step budgets before the
// first group runs), how far it is filled, and the parts' records.  A group's Chunk::deliver joins its rows behind what is there.
struct JoinSink {
    JoinLens lens;                // the pair of the join options
    std::vector<JoinLens> seam;   // [n], by request index: the seam BEHIND part i (a call without a list: `lens` everywhere)
    float* row = nullptr;         // the joined row (device)
    int64_t cap = 0;              // its samples
    ptts_join_part* parts;        // [n], by request index
    int64_t at = 0;               // the joined length so far
    int64_t n_prev = -1;          // samples of the last part joined (-1: none yet)
    int64_t frames = 0;
    int fail = PTTS_OK;           // the code of the first chunk, in text order, that was cancelled or ran past the decoder's reach
    std::string fail_msg;
    // What the join options' ext asks for every part in front of k_join, resolved once, before anything launches (runtime.h PartStages; parts_launch
    // runs it): a trim, whose length comes back from the device; a pitch other than 1000 (with the formants kept, where the handle says so); a tempo -- behind a pitch the pair (speed, pitch) was
    // resolved beforehand (pitch.h pitch_steps), `tmp` carries the effective speed and the step is off at 1000.  One PartStages per part, by request
    // index: a call without a list (include/ptts.h ptts_part_opts) fills them uniformly from the handle.  The designs the stages point to ([n], or [1]
    // where every part shares them):
    std::vector<PartStages> stages;
    std::vector<TrimScan> trm;
    std::vector<PitchScan> pit;
    std::vector<TempoScan> tmp;
    // a list's volumes ([n]; empty: a call without a list, whose groups go to join_launch as they always did) and where the gains go ([n], pinned;
    // null: a call without a list)
    std::vector<PartVolume> vol;
    float* gains = nullptr;
};

// One generate_chunk call: its requests and what its phases share.  The destructor is the clean-up of the normal path and of a throw
// alike: copies, decoder launches and host functions queued on the two streams may still read `cancelled`, `stream_ranges` and
// `stream_host`, so both streams are drained first, then the streaming buffers go back.
struct Chunk {
    Model& m;
    const ptts_request* reqs; const std::vector<int>& idx; ptts_result* res;   // slot i: reqs[idx[i]], answered in res[idx[i]]
    const int lsd;
    JoinSink* const join;        // generate_joined: the group's rows go into the text's joined row, nothing into res (null)
    const int B = (int)idx.size(), ld = m.d.ldim;
    const int64_t spf = m.d.samples_per_frame;
    const hipStream_t s = m.stream;
    // The decoder's RoPE table ends at ROPE_SEQ positions (mimi.go:498): like the reference, a step budget beyond that is not an
    // error by itself -- generating that many frames is (the decoder is sized for what can be decoded).
    const int t_limit = mimi_frame_limit(m.d);
    std::vector<SlotReq> list;   // slot i: reqs[idx[i]] and its step budget
    int ms_max = 0, T = 0;       // the largest step budget; the frames the decoder is sized for
    Batch* b = nullptr;
    std::vector<char> cancelled = std::vector<char>((size_t)B, 0);
    DevBuf* pcm = nullptr;       // decoded samples, [B][T * spf]
    int chunk = 1 << 30;         // frames per range decoded under the AR loop (streaming, PTTS_MIMI_CHUNK)
    bool streaming = false;
    // Streaming (pcm_callback): ranges of `chunk` frames are decoded on stream2 behind the AR loop, copied into the buffers the results
    // will own (stream_host) and announced from a host function queued on that stream (a HIP runtime thread).
    struct StreamRange {
        const Chunk* c; int f0, f1;
        int32_t* nf;   // pinned: n_frames of every slot, read after the range's last step (converting rows: then the active flags, [B, 2B))
        bool last;     // the final hand-over: every utterance is flushed
        std::vector<int64_t> ready;   // converting rows: the outputs this range delivers if the utterance goes on
    };
    std::vector<void*> stream_host = std::vector<void*>((size_t)B, nullptr);
    // streaming at another rate or in G.711 (k_resample per hand-over): outputs converted so far if the utterance goes on (the next range's o0),
    // outputs announced (host function), and the device rows the hand-overs are converted into (stream_stage, stage_row bytes apart) and copied
    // from into the result buffers, like the f32 / PCM16 hand-overs: the host function reads what the copies have landed
    bool any_conv = false;
    std::vector<int64_t> stream_next = std::vector<int64_t>((size_t)B, 0);
    mutable std::vector<int64_t> stream_sent = std::vector<int64_t>((size_t)B, 0);
    char* stream_stage = nullptr;
    size_t stage_row = 0;
    std::vector<std::unique_ptr<StreamRange>> stream_ranges;
    DevBuf* stream_s16 = nullptr;
    MimiWs mw;
    int dec_group = 0;
    int f_done = 0, f_emitted = 0, steps_run = 0;   // frames decoded, announced, generated
    size_t ev_used = 0;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();

    ~Chunk() {
        (void)hipStreamSynchronize(m.stream2);
        (void)hipStreamSynchronize(m.stream);
        for (auto& r : stream_ranges) (void)hipHostFree(r->nf);
        for (void* p : stream_host) result_free(p);   // buffers of cancelled / failed streaming requests
    }
    const ptts_request& req(int i) const { return reqs[idx[(size_t)i]]; }
    Error too_long(int frames) const {
        return Error(PTTS_EINVAL, strfmt("generate: mimi_decode: ops: rope cos/sin sequence length too small for pos=0 seq=%lld", (long long)frames * m.d.up_stride));
    }
    void mark(const char* what) {   // PTTS_TRACE=1: host wall time of the phases of one call (stderr); each mark drains the streams first
        static const bool trace = getenv("PTTS_TRACE") != nullptr;
        if (!trace) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(m.stream2);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[ptts] %-12s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
    hipEvent_t phase_event(int i) {   // measurement pass only (ptts_profile_enable): device time of the call's phases
        if (!m.prof.phases_on) return nullptr;
        if (!m.prof.phase[i]) PTTS_HIP(hipEventCreate(&m.prof.phase[i]));
        return m.prof.phase[i];
    }
    void phase(int i, hipStream_t st) { if (hipEvent_t e = phase_event(i)) PTTS_HIP(hipEventRecord(e, st)); }
    // how slot i's utterance of nf frames ends: cancelled, or PTTS_EINVAL -- it ran past the decoder's reach and fails one by one, like the
    // reference's one GenerateAudio call (too_long has the message); such slots are decoded with the others, not delivered
    int slot_status(int i, int nf) const { return cancelled[(size_t)i] ? PTTS_ECANCELLED : nf > t_limit ? PTTS_EINVAL : PTTS_OK; }
    void setup(); void decoder_setup(); void ar_loop(); void deliver();   // the phases, in order
    void deliver_joined(const int32_t* nf, const int32_t* eos);
    void decode_upto(int f1, const PcmRow* rows = nullptr, bool* rows_used = nullptr);
    void decode_rest(int f1, const PcmRow* rows = nullptr, bool* rows_used = nullptr);
    void emit_upto(int f1, bool last = false);
};

// the batch, the slots' step budgets and EOS settings, voices, prompts and sampling noise
void Chunk::setup() {
    int cap_need = 0;
    for (int i = 0; i < B; i++) {
        const ptts_request& r = req(i);
        const int ms = resolve_max_steps(r);
        const int tp = (int)r.n_tokens + (r.voice_embedding ? (int)r.voice_frames : 0);
        const int off = r.voice ? reinterpret_cast<const Voice*>(r.voice)->offset : (r.voice_caches ? (int)r.voice_offsets[0] : 0);
        list.push_back(SlotReq{i, &r, ms});
        cap_need = std::max(cap_need, off + tp + ms);
        ms_max = std::max(ms_max, ms);
    }
    int cap = (cap_need + 63) / 64 * 64;
    if (cap > ROPE_SEQ) throw Error(PTTS_EINVAL, strfmt("ops: rope cos/sin sequence length too small for pos=%d seq=1", cap_need));
    if (!m.cached_batch || m.cached_batch->B != B || m.cached_batch->cap < cap || m.cached_batch->max_steps < ms_max) {
        m.cached_batch.reset();
        m.cached_batch.reset(batch_new(m, B, cap, ms_max));
    }
    b = m.cached_batch.get();
    batch_reset(*b);
    // (a slot stops at most one frame past what the decoder's RoPE table reaches: generating that frame is what the reference reports as the
    // error, mimi.go:498 -- for that utterance alone; the other utterances of the batch are unaffected)
    std::vector<int32_t> v_ms((size_t)B), v_fae((size_t)B);
    std::vector<float> v_thr((size_t)B);
    for (int i = 0; i < B; i++) { v_ms[i] = std::min(list[i].max_steps, t_limit + 1); v_fae[i] = req(i).frames_after_eos; v_thr[i] = req(i).eos_threshold; }
    h2d(b->st.max_steps, v_ms.data(), (size_t)B * 4, s);
    h2d(b->st.frames_after_eos, v_fae.data(), (size_t)B * 4, s);
    h2d(b->st.eos_threshold, v_thr.data(), (size_t)B * 4, s);
    mark("setup");
    m.prof.phases = false;
    stage_prompt(*b, list, s, phase_event(0));
    phase(1, s);
    mark("prefill");
    b->has_noise = false;
    for (int i = 0; i < B; i++) b->has_noise |= req(i).noise != nullptr || req(i).temperature > 0.0f;
    if (!b->has_noise) return;
    b->noise.ensure((size_t)B * b->max_steps * ld * sizeof(float));
    stage_noise(*b, list, s);
}

// Mimi decode of finished frame ranges runs on a second stream while the AR loop keeps stepping: the loop is a chain of latency-bound
// launches that leaves most of the chip idle, the decoder is throughput work, and every decoder op is causal, so frames [f0, f1) can be
// decoded as soon as step f1-1 has finished.
void Chunk::decoder_setup() {
    T = std::min(ms_max, t_limit);
    pcm = &m.work(WORK_PCM, (size_t)B * T * spf * sizeof(float));
    const char* env_chunk = getenv("PTTS_MIMI_CHUNK");
    chunk = env_chunk && atoi(env_chunk) > 0 ? atoi(env_chunk) : 1 << 30;   // default: decode after the loop (measured: overlapping
                                                                            // slows the AR launches by as much as it hides)
    for (int i = 0; i < B; i++) streaming |= req(i).pcm_callback != nullptr;
    if (streaming) {
        chunk = 1 << 30;
        bool any_s16 = false;
        for (int i = 0; i < B; i++) {
            const ptts_request& r = req(i);
            if (!r.pcm_callback) continue;
            chunk = std::min(chunk, r.stream_frames > 0 ? (int)r.stream_frames : 12);
            const size_t bytes = (size_t)std::max<int64_t>(1, egress_length(r, (int64_t)list[i].max_steps * spf)) * pcm_bytes(r.pcm_format);
            stream_host[(size_t)i] = result_alloc(bytes);
            if (!stream_host[(size_t)i]) throw Error(PTTS_ENOMEM, "ptts-hip: out of host memory");
            const bool conv = request_converts(r);
            any_s16 |= r.pcm_format == PTTS_PCM_S16 && !conv;
            any_conv |= conv;
            if (conv) stage_row = std::max(stage_row, (bytes + 255) & ~(size_t)255);
        }
        if (any_s16) stream_s16 = &m.work(WORK_STREAM_S16, (size_t)B * T * spf * sizeof(int16_t));
        if (stage_row) stream_stage = m.work(WORK_STREAM_STAGE, stage_row * (size_t)B).as<char>();
    }
    // Decoder workspace (~2.7 MB of f32 activations per latent frame and utterance).  A batch of more than kMimiGroup utterances that is decoded in one go after the
    // loop (the default) goes through the decoder group after group in the SAME buffers (stream order keeps them apart); a batch whose frame ranges are decoded under
    // the loop (streaming, PTTS_MIMI_CHUNK) needs every utterance's history from range to range and keeps one workspace for all of them.
    dec_group = (B > kMimiGroup && !streaming && chunk > ms_max) ? kMimiGroup : B;
    mimi_setup(m, mw, dec_group, T);
    mimi_zero_history(m, mw, m.stream2);   // nine small launches: under the AR loop instead of between the loop and the decoder
}

void Chunk::ar_loop() {
    m.tcomb_for(lsd);
    // PTTS_GRAPH=0/1 overrides the option (A/B measurement, tools/eager_vs_graph.py)
    static const int env_graph = [] { const char* e = getenv("PTTS_GRAPH"); return e ? atoi(e) : -1; }();
    const bool use_graph = (env_graph >= 0 ? env_graph != 0 : m.opts.use_graph != 0) && !m.prof.on;
    bool may_stop = false, any_cb = false, any_cancel_flag = false;
    for (int i = 0; i < B; i++) {
        may_stop |= req(i).eos_threshold < 1e30f;
        any_cb |= req(i).step_callback != nullptr;
        any_cancel_flag |= req(i).cancel != nullptr;
    }
    std::vector<int32_t> act((size_t)B, 1);
    // graph replay without per-step host work (no step callbacks, no cancel flags, no ranges to decode on the way): several
    // steps per graph.  Slots that finish inside a graph are skipped by every kernel of the remaining steps (active flags).
    // 5 steps per graph; 25 when no request of the batch can end by EOS (threshold = +inf: every budget is known, so no replayed step can turn out to
    // have been for nothing) -- measured on the 125-step batch: 1 -> 5 steps: -0.2..-0.6 ms, 5 -> 25: -0.5 ms, 125: -0.15 (one big graph is slower again)
    static const int env_gsteps = [] { const char* e = getenv("PTTS_GRAPH_STEPS"); return e ? std::max(1, atoi(e)) : 0; }();
    const int gsteps = (use_graph && !any_cb && !any_cancel_flag && chunk > ms_max) ? (env_gsteps ? env_gsteps : (may_stop ? 5 : 25)) : 1;
    const int ms_loop = std::min(ms_max, t_limit + 1);
    for (int step = 0; step < ms_loop;) {
        int n_cancel = 0;
        for (int i = 0; i < B; i++) {  // ctx.Err() check before every step (:156-159)
            const ptts_request& r = req(i);
            if (r.cancel && *r.cancel) cancelled[i] = 1;
            n_cancel += cancelled[i];
        }
        if (n_cancel == B) break;
        const int n_now = (gsteps > 1 && step + gsteps <= ms_loop) ? gsteps : (gsteps > 5 && step + 5 <= ms_loop) ? 5 : 1;   // the tail: smaller graphs
        enqueue_step(*b, lsd, use_graph, n_now);
        step += n_now;
        steps_run = step;
        if (steps_run % chunk == 0) { decode_upto(steps_run); emit_upto(steps_run); }
        if (any_cb) {  // StepCallback runs synchronously after the step (:194-196)
            std::vector<int32_t> before = act, broke((size_t)B);
            d2h(act.data(), b->st.active, (size_t)B * 4, s);
            d2h(broke.data(), b->st.broke, (size_t)B * 4, s);
            for (int i = 0; i < B; i++) {  // not called for the iteration that leaves through `break` (:185-187)
                const ptts_request& r = req(i);
                if (r.step_callback && before[i] && !broke[i] && !cancelled[i]) r.step_callback(r.callback_user, step, list[i].max_steps);
            }
            if (std::none_of(act.begin(), act.end(), [](int32_t a) { return a != 0; })) break;
        } else if (may_stop && step / 8 != (step - n_now) / 8) {   // every eighth step (or the first graph boundary past it)
            PTTS_HIP(hipMemcpyAsync(b->n_active_pinned, b->st.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            PTTS_HIP(hipStreamSynchronize(s));
            if (*b->n_active_pinned <= 0) break;
        }
    }
    phase(2, s);
    mark("ar loop");
}

// frames [f_done, f1) of every utterance through the decoder on stream2, behind the steps queued so far; rows (whole range only): the
// decoder's direct store (results_alloc), *rows_used: whether it took it
void Chunk::decode_upto(int f1, const PcmRow* rows, bool* rows_used) {
    if (f1 <= f_done) return;
    if (f1 > T) throw too_long(f1);
    if (m.events.size() <= ev_used) { hipEvent_t e; PTTS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m.events.push_back(e); }
    hipEvent_t e = m.events[ev_used++];
    PTTS_HIP(hipEventRecord(e, s));
    PTTS_HIP(hipStreamWaitEvent(m.stream2, e, 0));
    const int64_t lstride = (int64_t)b->max_steps * ld;
    int direct = 0, groups = 0;
    for (int g0 = 0; g0 < B; g0 += dec_group, groups++) {
        const int nb = std::min(dec_group, B - g0);
        MimiWs wg;
        MimiWs* w = &mw;
        if (nb != mw.B) { mimi_setup(m, wg, nb, T); w = &wg; }   // the last, smaller group: its own layout inside the same (grow-only) buffer
        if (g0 > 0) w->zeroed = false;                           // (a group's history rows: zeroed again in front of its decode)
        bool used = false;
        mimi_range(m, *w, b->latents.as<float>() + (int64_t)g0 * lstride, lstride, f_done, f1, pcm->as<float>() + (size_t)g0 * T * spf, nullptr, m.stream2,
                   (f_done == 0 && rows) ? rows + g0 : nullptr, &used);
        direct += used ? 1 : 0;
    }
    if (direct != 0 && direct != groups) throw Error(PTTS_EINVAL, "ptts-hip: internal: the decoder's groups disagree about the direct PCM rows");
    if (rows_used) *rows_used = direct != 0;
    f_done = f1;
}

// hand frames [f_emitted, f1) to the streaming callbacks (they are decoded: f1 <= f_done).  Rows at another rate or in G.711 are converted by one
// k_resample launch: every output whose filter support lies inside the decoded input, the rest with the next hand-over -- all of it once the
// utterance has ended (its input ends there: outputs past it read zeros) or with the last hand-over.  Offsets count output samples.
void Chunk::emit_upto(int f1, bool last) {
    if (!streaming || (f1 <= f_emitted && !(last && any_conv))) return;
    const int f0 = f_emitted;
    hipStream_t s2 = m.stream2;
    if (stream_s16 && f1 > f0) launch_pcm16_rows(pcm->as<float>(), stream_s16->as<int16_t>(), B, (int64_t)T * spf, (int64_t)f0 * spf, (int64_t)(f1 - f0) * spf, s2);
    for (int i = 0; i < B; i++) {
        if (!stream_host[(size_t)i] || request_converts(req(i))) continue;
        const int fe = std::min(f1, list[i].max_steps);
        if (fe <= f0) continue;
        const bool s16 = req(i).pcm_format == PTTS_PCM_S16;
        const size_t esz = s16 ? sizeof(int16_t) : sizeof(float);
        const char* src = s16 ? (const char*)stream_s16->p : (const char*)pcm->p;
        PTTS_HIP(hipMemcpyAsync((char*)stream_host[(size_t)i] + (size_t)f0 * spf * esz, src + ((size_t)i * T * spf + (size_t)f0 * spf) * esz,
                                (size_t)(fe - f0) * spf * esz, hipMemcpyDeviceToHost, s2));
    }
    int32_t* nfp = nullptr;
    PTTS_HIP(hipHostMalloc((void**)&nfp, (size_t)2 * B * sizeof(int32_t), hipHostMallocDefault));
    stream_ranges.emplace_back(new StreamRange{this, f0, f1, nfp, last, std::vector<int64_t>((size_t)B, 0)});
    StreamRange& range = *stream_ranges.back();
    if (any_conv) {
        // one snapshot of (active, n_frames) for this range's k_resample rows AND its host function, so that both agree on which utterances
        // have ended.  The AR loop goes on meanwhile: active is copied first, so an utterance seen inactive comes with its final frame count
        DevBuf& snap = m.work(WORK_STREAM_SNAP, (size_t)2 * B * sizeof(int32_t));
        int32_t* sa = snap.as<int32_t>();
        int32_t* sn = sa + B;
        PTTS_HIP(hipMemcpyAsync(sa, b->st.active, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s2));
        PTTS_HIP(hipMemcpyAsync(sn, b->st.n_frames, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s2));
        std::vector<ResampleRow> rows;
        std::vector<std::pair<int, ResampleRow>> staged;
        for (int i = 0; i < B; i++) {
            const ptts_request& r = req(i);
            if (!stream_host[(size_t)i] || !request_converts(r)) continue;
            const RateFilter* f = rate_filter(m, kNativeRate, request_rate(r), s2);
            const int64_t n_dec = (int64_t)std::min(f1, list[i].max_steps) * spf;   // (no utterance runs past its step budget: its buffer's size)
            const int64_t o0 = stream_next[(size_t)i], o1 = std::max(o0, resample_ready(f, n_dec));
            void* dst = stream_stage + (size_t)i * stage_row;
            ResampleRow row = resample_row(f, pcm->as<float>() + (size_t)i * T * spf, n_dec, dst, o0, o1, r.pcm_format);
            row.o_cap = egress_length(r, n_dec);
            row.nf = sn + i; row.act = sa + i; row.spf = (int32_t)spf; row.fin = last ? 1 : 0;
            rows.push_back(row);
            staged.emplace_back(i, row);
            range.ready[(size_t)i] = o1;
            stream_next[(size_t)i] = o1;
        }
        resample_launch(m, rows, s2);
        for (const auto& st : staged) {   // the range's outputs [o0, o_cap); what is not final yet is copied again by a later range
            const size_t esz = pcm_bytes(st.second.fmt);
            if (st.second.o_cap > st.second.o0)
                PTTS_HIP(hipMemcpyAsync((char*)stream_host[(size_t)st.first] + st.second.o0 * esz, (const char*)st.second.dst + st.second.o0 * esz,
                                        (size_t)(st.second.o_cap - st.second.o0) * esz, hipMemcpyDeviceToHost, s2));
        }
        PTTS_HIP(hipMemcpyAsync(nfp, sn, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s2));
        PTTS_HIP(hipMemcpyAsync(nfp + B, sa, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s2));
    } else {
        PTTS_HIP(hipMemcpyAsync(nfp, b->st.n_frames, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s2));
    }
    PTTS_HIP(hipLaunchHostFunc(s2, [](void* p) {
        const StreamRange& sr = *static_cast<const StreamRange*>(p);
        const Chunk& c = *sr.c;
        for (int i = 0; i < c.B; i++) {
            const ptts_request& r = c.req(i);
            if (!r.pcm_callback || !c.stream_host[(size_t)i] || c.cancelled[(size_t)i]) continue;
            const size_t esz = pcm_bytes(r.pcm_format);
            if (request_converts(r)) {   // the same arithmetic as the range's k_resample row, on the same snapshot
                const int64_t n_dec = (int64_t)std::min(sr.f1, c.list[i].max_steps) * c.spf, e = (int64_t)sr.nf[i] * c.spf;
                const bool ended = sr.last || e < n_dec || (sr.nf[c.B + i] == 0 && e <= n_dec);
                const int64_t end = ended ? egress_length(r, std::min(n_dec, e)) : sr.ready[(size_t)i];
                const int64_t sent = c.stream_sent[(size_t)i];
                if (end <= sent) continue;
                r.pcm_callback(r.pcm_user, sent, end - sent, (const char*)c.stream_host[(size_t)i] + (size_t)sent * esz);
                c.stream_sent[(size_t)i] = end;
                continue;
            }
            const int end = std::min(sr.f1, (int)sr.nf[i]);   // frames past the utterance's end are not audio
            if (end <= sr.f0) continue;
            r.pcm_callback(r.pcm_user, (int64_t)sr.f0 * c.spf, (int64_t)(end - sr.f0) * c.spf, (const char*)c.stream_host[(size_t)i] + (size_t)sr.f0 * c.spf * esz);
        }
    }, &range));
    f_emitted = std::max(f_emitted, f1);
}

// behind the loop: the decode of what has not been decoded under it, up to frame f1 (frames past every utterance's end are never decoded), the last
// hand-over of a streaming batch (a joined group streams nothing: its requests carry no pcm_callback), the measurement pass's marks; stream2 is drained
void Chunk::decode_rest(int f1, const PcmRow* rows, bool* rows_used) {
    if (m.prof.phases_on) { PTTS_HIP(hipStreamWaitEvent(m.stream2, m.prof.phase[2], 0)); phase(3, m.stream2); }
    decode_upto(f1, rows, rows_used);
    emit_upto(f1, true);
    phase(4, m.stream2);
    m.prof.phases = m.prof.phases_on && f_done > 0;
    PTTS_HIP(hipStreamSynchronize(m.stream2));
    mark("mimi");
}

// the frame counts back; the decode of what has not been decoded under the loop; the results
void Chunk::deliver() {
    // n_frames and eos_step sit side by side in the state block: one copy into page-locked memory, one wait
    int32_t* const hp = b->n_active_pinned;
    PTTS_HIP(hipMemcpyAsync(hp + 1, b->st.n_frames, (size_t)2 * B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    hp[1 + 2 * B] = 0;
    if (b->fc_ok) PTTS_HIP(hipMemcpyAsync(hp + 1 + 2 * B, b->fc_fault(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipStreamSynchronize(s));
    if (hp[1 + 2 * B]) flow_cluster_fault(*b);
    const int32_t* nf = hp + 1;
    if (join) { deliver_joined(nf, hp + 1 + B); return; }
    int Tmax = 0;
    std::vector<Delivery> g((size_t)B);   // row i of the decode: slot i (cancelled and over-long utterances are decoded, not delivered)
    for (int i = 0; i < B; i++) {
        const int status = slot_status(i, nf[i]);
        if (status == PTTS_EINVAL) set_last_error(too_long(nf[i]).what());
        if (status != PTTS_OK) { res[idx[i]].status = status; continue; }
        g[(size_t)i] = Delivery{&req(i), &res[idx[i]], nf[i], hp[1 + B + i], stream_host[(size_t)i] != nullptr};
        Tmax = std::max(Tmax, nf[i]);
    }
    // Whole batch decoded in one go (the default): the decoder's last kernel stores the samples into the result buffers itself
    const bool try_direct = !streaming && f_done == 0;
    const PcmRow* rows = results_alloc(m, g, try_direct ? b->rows_pinned : nullptr, try_direct ? m.work(WORK_PCM_ROWS, (size_t)B * sizeof(PcmRow)).as<PcmRow>() : nullptr, s);
    bool stored = false;
    decode_rest(std::min(steps_run, Tmax), rows, &stored);
    for (int i = 0; i < B; i++) {   // streamed: the buffer already holds every sample that was announced
        if (!g[(size_t)i].filled) continue;
        set_result_buffer(res[idx[i]], req(i).pcm_format, stream_host[(size_t)i]);
        stream_host[(size_t)i] = nullptr;
    }
    results_deliver(m, g, stored, pcm->as<float>(), (int64_t)T * spf, b->latents.as<float>(), (int64_t)b->max_steps * ld, s);
    PTTS_HIP(hipStreamSynchronize(s));
    mark("results d2h");
}

// generate_joined's delivery (behind the fault check: a group that is run again has joined nothing yet): the parts' records; the decode of
// the whole group into the decoder's buffer; with a trim (trim.h), the rows' trimmed forms and their lengths; with a tempo (tempo.h), their
// time-scaled forms, and with a pitch (pitch.h) their resampled forms in front of that; one k_join table that copies the
// group's rows behind what the text's row holds.  A seam inside
// the group is computed by the row behind it, which reads its predecessor's tail in the decoder's buffer.  The group's first row has its
// predecessor in an earlier group, whose buffer is gone: that group stored the tail unfaded, and this row fades it where it lies.
void Chunk::deliver_joined(const int32_t* nf, const int32_t* eos) {
    int Tmax = 0;
    for (int i = 0; i < B; i++) {
        ptts_join_part& p = join->parts[idx[(size_t)i]];
        p.n_frames = nf[i]; p.eos_step = eos[i];
        p.status = slot_status(i, nf[i]);
        if (p.status != PTTS_OK && join->fail == PTTS_OK) {
            join->fail = p.status;
            join->fail_msg = p.status == PTTS_EINVAL ? std::string(too_long(nf[i]).what()) : strfmt("generate: context canceled (request %d of the joined call)", idx[(size_t)i]);
        }
        Tmax = std::max(Tmax, nf[i]);
    }
    if (join->fail != PTTS_OK) return;   // the call fails: nothing of this group is decoded
    decode_rest(std::min(steps_run, Tmax));
    // The parts as the join sees them: the decoder's rows through the part stages (parts_launch: the trim, the pitch, the tempo, each where the part
    // has it).  What the trim keeps lies in a buffer of the decoder buffer's row stride; the resampled and the time-scaled forms in buffers whose
    // row stride holds the longest a decoded row of the group's widest part can become.  Everything below counts in the lengths that come back
    const size_t decoded = (size_t)T * spf;
    bool any_trim = false, any_pitch = false, any_tempo = false;
    int64_t wide_p = (int64_t)decoded, wide_t = (int64_t)decoded;
    for (int i = 0; i < B; i++) {
        const PartStages& st = join->stages[(size_t)idx[(size_t)i]];
        any_trim |= st.trim != nullptr; any_pitch |= st.pitch != nullptr; any_tempo |= st.tempo != nullptr;
        const int64_t mine_p = st.pitch ? std::max<int64_t>(decoded, pitch_resample_length(decoded, st.pitch->p)) : (int64_t)decoded;
        const int64_t mine_t = st.tempo ? std::max(mine_p, tempo_length(mine_p, st.tempo->speed)) : mine_p;
        wide_p = std::max(wide_p, mine_p);
        wide_t = std::max(wide_t, mine_t);
    }
    float* const kept = any_trim ? m.work(WORK_TRIMMED, std::max<size_t>((size_t)B * decoded, 1) * sizeof(float)).as<float>() : nullptr;
    float* const shifted = any_pitch ? m.work(WORK_PITCH, std::max<size_t>((size_t)B * (size_t)wide_p, 1) * sizeof(float)).as<float>() : nullptr;
    float* const scaled = any_tempo ? m.work(WORK_TEMPO, std::max<size_t>((size_t)B * (size_t)wide_t, 1) * sizeof(float)).as<float>() : nullptr;
    std::vector<PartRow> part((size_t)B);
    for (int i = 0; i < B; i++) {
        PartRow& r = part[(size_t)i];
        r.src = pcm->as<float>() + (size_t)i * decoded; r.n = (int64_t)nf[i] * spf; r.st = join->stages[(size_t)idx[(size_t)i]];
        if (r.st.trim) r.trimmed = kept + (size_t)i * decoded;
        if (r.st.pitch) r.shifted = shifted + (size_t)i * (size_t)wide_p;
        if (r.st.tempo) r.scaled = scaled + (size_t)i * (size_t)wide_t;
    }
    parts_launch(m, part, s, [&](const char* what) { mark(what); }, "part");
    // a list's volumes, on the parts as the tempo left them: the fixed gains, and for the levels the loudness rows' measuring launches, whose gain
    // words k_join_gain reads (no host round trip, no pass that rewrites the samples)
    std::vector<PartGain> pg;
    if (!join->vol.empty()) {
        std::vector<const float*> x((size_t)B);
        std::vector<int64_t> len((size_t)B);
        std::vector<PartVolume> vol((size_t)B);
        for (int i = 0; i < B; i++) { x[(size_t)i] = part[(size_t)i].out; len[(size_t)i] = part[(size_t)i].n_out; vol[(size_t)i] = join->vol[(size_t)idx[(size_t)i]]; }
        pg = part_gains_launch(m, x, len, vol, s);
        for (int i = 0; i < B; i++) {
            float* const to = join->gains + idx[(size_t)i];
            *to = pg[(size_t)i].fixed ? pg[(size_t)i].g : 1.0f;
            if (pg[(size_t)i].word) PTTS_HIP(hipMemcpyAsync(to, pg[(size_t)i].word, sizeof(float), hipMemcpyDeviceToHost, s));   // (page-locked: nothing waits)
        }
    }
    std::vector<JoinRow> rows;
    for (int i = 0; i < B; i++) {
        ptts_join_part& p = join->parts[idx[(size_t)i]];
        const int64_t n = part[(size_t)i].n_out;
        const bool first = join->n_prev < 0;
        const JoinLens l = first ? JoinLens{} : join->seam[(size_t)idx[(size_t)i] - 1];   // the seam in front of the part
        const int64_t k = first ? 0 : join_seam(l.xfade, join->n_prev, n);
        const int64_t off = first ? 0 : join->at + l.gap - k;
        const int64_t k_next = i + 1 < B ? join_seam(join->seam[(size_t)idx[(size_t)i]].xfade, n, part[(size_t)i + 1].n_out) : 0;   // (the group's last row stores its tail whole)
        if (off + n > join->cap) throw Error(PTTS_EINVAL, "ptts-hip: internal: the joined row is smaller than the text");
        JoinRow r{};
        r.src = part[(size_t)i].out;
        r.prev = !k ? nullptr : i ? part[(size_t)i - 1].out + (join->n_prev - k) : join->row + off;
        r.dst = join->row;
        r.off = off; r.n = n - k_next; r.k = (int32_t)k; r.gap = first ? 0 : (int32_t)l.gap;
        rows.push_back(r);
        p.offset = off; p.n_samples = n;
        join->at = off + n; join->n_prev = n; join->frames += nf[i];
    }
    if (!join->vol.empty()) {   // the gain form where a table has a gain (join_gain_launch); the tail of an earlier group lies in the joined row, scaled
        std::vector<JoinGainRow> grows;
        for (int i = 0; i < B; i++) grows.push_back(join_gain_row(rows[(size_t)i], pg[(size_t)i], i ? &pg[(size_t)i - 1] : nullptr));
        join_gain_launch(m, grows, s);
        mark("join");
        return;
    }
    join_launch(m, rows, s);   // behind the decode (stream2 has been waited for); the next group's decode waits for s (decode_upto)
    mark("join");
}
}  // namespace

static void generate_chunk(Model& m, const ptts_request* reqs, const std::vector<int>& idx, ptts_result* res, int lsd, JoinSink* join = nullptr) {
    UploadScope upload_scope(m.upload, m.stream);
    Chunk c{m, reqs, idx, res, lsd, join};
    c.setup();
    c.decoder_setup();
    c.ar_loop();
    c.deliver();
}

std::string request_error(const Desc& d, const ptts_request& q) {   // the argument checks of GenerateAudio (runtime_native_safetensors.go:52-119)
    if (!q.tokens || q.n_tokens <= 0) return "generate: token slice must not be empty";
    if ((q.voice_embedding != nullptr) + (q.voice_caches != nullptr) + (q.voice != nullptr) > 1) return "generate: voice embedding and voice model state are mutually exclusive";
    if (q.voice_caches && (!q.voice_cache_steps || !q.voice_offsets)) return "generate: load voice model state: missing cache steps/offsets";
    if (q.noise && q.noise_rows > 0 && q.noise_rows < resolve_max_steps(q))
        return strfmt("generate: injected noise has %d rows, the step budget is %d", q.noise_rows, resolve_max_steps(q));
    if (std::isnan(q.temperature)) return "generate: temperature is NaN";
    if (q.pcm_format < PTTS_PCM_F32 || q.pcm_format > PTTS_PCM_ALAW)
        return strfmt("generate: pcm_format %d is not PTTS_PCM_F32, PTTS_PCM_S16, PTTS_PCM_ULAW or PTTS_PCM_ALAW", q.pcm_format);
    if (q.sample_rate != 0) {
        const std::string e = rate_pair_error(kNativeRate, q.sample_rate);
        if (!e.empty()) return "generate: " + e;
    }
    if (q.dsp) {
        DspSpec spec;
        std::string e = dsp_resolve(q.dsp, &spec);
        if (e.empty()) e = dsp_trim_refusal(spec);   // a request's result buffers are sized before the decode
        if (e.empty()) e = dsp_tempo_refusal(spec);
        if (e.empty()) e = dsp_pitch_refusal(spec);
        if (!e.empty()) return "generate: " + e;
        if (q.pcm_callback) {   // the peak and the end are not known when samples are handed over; the filter and the fade in are refused with it for now
            const char* f = q.dsp->normalize ? "normalize" : q.dsp->fade_out_ms > 0 ? "fade_out_ms" : q.dsp->dc_block ? "dc_block" : q.dsp->fade_in_ms > 0 ? "fade_in_ms" : q.dsp->eq ? "eq" : q.dsp->ext ? "ext" : nullptr;
            if (f) return strfmt("generate: dsp: %s cannot be combined with pcm_callback", f);
        }
    }
    if (q.loudness) {   // 0.01 LUFS; one gain slot with normalise; not known when a stream's samples are handed over
        if (q.loudness < -7000 || q.loudness > -100) return strfmt("generate: loudness %d is not 0 (off) or a target from -7000 to -100 (0.01 LUFS)", q.loudness);
        if (q.dsp && q.dsp->normalize) return "generate: loudness cannot be combined with dsp normalize (one gain)";
        if (q.pcm_callback) return "generate: loudness cannot be combined with pcm_callback";
    }
    for (int64_t t = 0; t < q.n_tokens; t++)
        if (q.tokens[t] < 0 || q.tokens[t] >= d.n_bins)
            return strfmt("generate: text embeddings: native: token id %lld (%lld) out of range [0,%d)", (long long)t, (long long)q.tokens[t], d.n_bins);
    return std::string();
}

// one group, and once more after a hand-off inside k_flow_cluster timed out somewhere in its AR loop (found when the loop's counters were read
// back).  The group's inputs are the requests themselves: it runs again on the 2 x depth launches, which compute the same bits (the batch has
// been switched over: flow_cluster_recover).  Only a group that has already spoken to its caller -- step callbacks, streamed samples -- cannot
// be re-run.  res null: a group of generate_joined, which has delivered nothing when the fault is found
static void result_clear(ptts_result& r) { std::memset(&r, 0, sizeof r); r.eos_step = -1; }   // an empty result: no frame has ended the utterance
static void generate_group(Model& m, const ptts_request* reqs, const std::vector<int>& idx, ptts_result* res, int lsd, JoinSink* join = nullptr) {
    try {
        generate_chunk(m, reqs, idx, res, lsd, join);
    } catch (const FlowClusterFault&) {
        bool spoke = false;
        for (int i : idx) spoke |= reqs[i].step_callback != nullptr || reqs[i].pcm_callback != nullptr;
        if (spoke) throw;
        if (res) for (int i : idx) { ptts_free_result(&res[i]); result_clear(res[i]); }
        generate_chunk(m, reqs, idx, res, lsd, join);
    }
}

void generate(Model& m, const ptts_request* reqs, int n, ptts_result* res) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    const Desc& d = m.d;
    std::map<int, std::vector<int>> groups;  // lsd_steps -> request indices
    std::string first_err;
    for (int i = 0; i < n; i++) {
        ptts_result& r = res[i];
        result_clear(r);
        const ptts_request& q = reqs[i];
        std::string err = request_error(d, q);
        if (!err.empty()) {
            r.status = PTTS_EINVAL;
            if (first_err.empty()) first_err = err;
            continue;
        }
        groups[request_lsd(q)].push_back(i);
    }
    const int mb = std::max(1, m.opts.max_batch);
    for (auto& kv : groups) {
        const std::vector<int>& all = kv.second;
        for (size_t o = 0; o < all.size(); o += (size_t)mb) {
            std::vector<int> idx(all.begin() + (long)o, all.begin() + (long)std::min(all.size(), o + (size_t)mb));
            try {
                generate_group(m, reqs, idx, res, kv.first);
            } catch (const Error& e) {
                for (int i : idx) { ptts_free_result(&res[i]); res[i].status = e.code; res[i].eos_step = -1; }
                if (first_err.empty()) first_err = e.what();
            }
        }
    }
    if (!first_err.empty()) set_last_error(first_err);
}

// ------------------------------------------------------------------------------------------------
// Joined synthesis: a text's chunks as one utterance (include/ptts.h ptts_generate_joined; join.h)
// ------------------------------------------------------------------------------------------------
// the egress and the chain of the join options, as request_error checks a request's: empty, or the message naming the field
static std::string join_egress_error(const ptts_join_opts& o) {
    if (o.pcm_format < PTTS_PCM_F32 || o.pcm_format > PTTS_PCM_ALAW)
        return strfmt("join: pcm_format %d is not PTTS_PCM_F32, PTTS_PCM_S16, PTTS_PCM_ULAW or PTTS_PCM_ALAW", o.pcm_format);
    if (o.sample_rate != 0) {
        const std::string e = rate_pair_error(kNativeRate, o.sample_rate);
        if (!e.empty()) return "join: sample_rate: " + e;
    }
    if (o.dsp) {
        const std::string e = dsp_opts_error(*o.dsp);
        if (!e.empty()) return "join: " + e;
    }
    if (o.loudness) {
        if (o.loudness < -7000 || o.loudness > -100) return strfmt("join: loudness %d is not 0 (off) or a target from -7000 to -100 (0.01 LUFS)", o.loudness);
        if (o.dsp && o.dsp->normalize) return "join: loudness cannot be combined with dsp normalize (one gain)";
    }
    return std::string();
}

namespace {
// A streamed joined call (include/ptts.h ptts_generate_joined_streamed): what its hand-overs share.  Behind each group's k_join the chain runs over
// the window [done, P) of the joined row with the carried states (dsp_launch's windowed jobs), the egress converts or copies the outputs
// [sent, o) into the buffer the result will own, and a host function on stream2 -- where a slow callback holds up a decode at the most, never
// the next group's steps -- announces them.
struct JoinStream {
    Model& m;
    const ptts_join_stream_opts& so;
    const ptts_request& eg;          // the join options' chain and egress, as a request states its own
    DspSpec spec;                    // the chain, resolved before anything launched
    int64_t fade_in = 0;             // the fade in's samples, not clamped
    void* host = nullptr;            // the result's buffer, allocated for the step budgets' bound
    char* stage = nullptr;           // where the egress stores when it cannot store into `host` itself (device, indexed like `host`)
    double* carry = nullptr;         // the chain's carried states (device, [kCarryDoubles])
    int64_t done = 0, sent = 0;      // 24 kHz samples the chain has finished; outputs handed over
    hipEvent_t ev = nullptr;
    struct HandOver { const JoinStream* js; int64_t off, count; };
    std::vector<std::unique_ptr<HandOver>> handed;   // read by the host functions: kept until both streams are drained

    JoinStream(Model& m_, const ptts_join_stream_opts& so_, const ptts_request& eg_) : m(m_), so(so_), eg(eg_) {}
    ~JoinStream() {
        (void)hipStreamSynchronize(m.stream);
        (void)hipStreamSynchronize(m.stream2);
        if (ev) (void)hipEventDestroy(ev);
        result_free(host);
    }
    void setup(int64_t bound, hipStream_t s) {
        fade_in = spec.fade_in_ms > 0 ? (int64_t)(spec.fade_in_ms / 1000.0 * (double)kNativeRate) : 0;
        const size_t bytes = (size_t)std::max<int64_t>(1, egress_length(eg, bound)) * pcm_bytes(eg.pcm_format);
        host = result_alloc(bytes);
        if (!host) throw Error(PTTS_ENOMEM, "ptts-hip: out of host memory");
        // k_resample stores into page-locked memory itself; f32 at 24 kHz without a chain is copied out of the joined row
        if (request_converts(eg) ? !result_is_pinned(host) : eg.pcm_format == PTTS_PCM_S16) stage = m.work(WORK_JOIN_STAGE, bytes).as<char>();
        carry = m.work(WORK_JOIN_CARRY, kCarryDoubles * sizeof(double)).as<double>();
        PTTS_HIP(hipMemsetAsync(carry, 0, kCarryDoubles * sizeof(double), s));
        PTTS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    // behind a group's k_join: `at` samples are joined; last: no part follows; hold: max(K, Fo), K the crossfade of the seam behind the group
    void window(float* row, int64_t at, bool last, int64_t hold, hipStream_t s) {
        int64_t P = last ? at : std::max(done, join_stream_ready(at, hold));
        if (!last && at < fade_in) P = done;   // the fade in is clamped by the final length: not known to exceed it yet
        if (P > done || last) {
            if (spec.any()) {
                std::vector<DspJob> jobs(1, DspJob{row, P, spec});
                jobs[0].t0 = done / kDspTile; jobs[0].open = !last; jobs[0].carry = carry;
                dsp_launch(m, jobs, s);
            }
            done = P;
        }
        // the egress of what is final: outputs [sent, o1)
        const int fmt = eg.pcm_format;
        const size_t esz = pcm_bytes(fmt);
        const bool conv = request_converts(eg);
        const RateFilter* f = conv ? rate_filter(m, kNativeRate, request_rate(eg), s) : nullptr;
        const int64_t o1 = last ? egress_length(eg, at) : std::max(sent, resample_ready(f, done));
        if (o1 <= sent) return;
        const char* from = nullptr;   // (null: the launch stored into `host` itself)
        if (conv) {
            std::vector<ResampleRow> rows(1, resample_row(f, row, done, stage ? (void*)stage : host, sent, o1, fmt));
            resample_launch(m, rows, s);
            from = stage;
        } else if (fmt == PTTS_PCM_S16) {
            launch_pcm16(row + sent, reinterpret_cast<int16_t*>(stage) + sent, o1 - sent, s);
            from = stage;
        } else {
            from = reinterpret_cast<const char*>(row);
        }
        hipStream_t s2 = m.stream2;
        PTTS_HIP(hipEventRecord(ev, s));
        PTTS_HIP(hipStreamWaitEvent(s2, ev, 0));
        if (from) PTTS_HIP(hipMemcpyAsync((char*)host + (size_t)sent * esz, from + (size_t)sent * esz, (size_t)(o1 - sent) * esz, hipMemcpyDeviceToHost, s2));
        handed.emplace_back(new HandOver{this, sent, o1 - sent});
        PTTS_HIP(hipLaunchHostFunc(s2, [](void* p) {
            const HandOver& h = *static_cast<const HandOver*>(p);
            const JoinStream& js = *h.js;
            js.so.pcm_callback(js.so.pcm_user, h.off, h.count, (const char*)js.host + (size_t)h.off * pcm_bytes(js.eg.pcm_format));
        }, handed.back().get()));
        sent = o1;
    }
};
}  // namespace

void generate_joined(Model& m, const ptts_request* reqs, int n, const ptts_join_opts& o, const ptts_join_stream_opts* so, ptts_result* out, ptts_join_part* parts,
                     const JoinPartsList* list) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    const Desc& d = m.d;
    const int64_t spf = d.samples_per_frame;
    result_clear(*out);
    std::vector<ptts_join_part> own;
    if (!parts) { own.resize((size_t)std::max(n, 1)); parts = own.data(); }
    for (int i = 0; i < n; i++) { std::memset(&parts[i], 0, sizeof parts[i]); parts[i].eos_step = -1; }
    const auto refuse = [&](const std::string& e) { out->status = PTTS_EINVAL; throw Error(PTTS_EINVAL, "ptts-hip: " + e); };
    // ---- refusals: nothing is launched ----
    JoinSink sink;
    sink.parts = parts;
    std::string e = join_opts_error(&o, &sink.lens);
    if (e.empty()) e = join_egress_error(o);
    if (e.empty() && (n < 1 || n > kJoinMaxRows)) e = strfmt("join: %d requests, a text has from 1 to %d parts", n, kJoinMaxRows);
    const int mb = std::max(1, m.opts.max_batch);
    if (e.empty() && so && (so->first_group < 0 || so->first_group > mb))
        e = strfmt("join: stream: first_group %d is not 0 (max_batch) or from 1 to max_batch (%d)", so->first_group, mb);
    if (!e.empty()) refuse(e);
    for (int i = 0; list && list->gains && i < n; i++) list->gains[i] = 1.0f;
    if (list) {   // the list's seams and volumes (join.h), resolved against the pair of the join options
        JoinSeams seams;
        e = join_parts_error(list->po, n, sink.lens, &seams, &sink.vol);
        if (!e.empty()) refuse(e);
        sink.seam = std::move(seams.lens);
        sink.gains = static_cast<float*>(m.part_gains.ensure((size_t)n * sizeof(float)));
        for (int i = 0; i < n; i++) sink.gains[i] = 1.0f;
    } else {
        sink.seam.assign((size_t)n, sink.lens);
    }
    const bool streamed = so && so->pcm_callback;
    DspSpec spec;
    sink.stages.assign((size_t)n, PartStages{});
    if (o.dsp) {   // the trim and the tempo of the parts, resolved once: the chain below never sees them
        e = dsp_resolve(o.dsp, &spec);
        if (!e.empty()) refuse("join: " + e);
        if (const char* f = !list ? nullptr : spec.trim ? "trim" : spec.pitch ? "pitch" : spec.formant ? "formant" : spec.tempo ? "tempo" : nullptr)
            refuse(strfmt("join: parts: the ext handle's %s belongs in the list (ptts_part_opts) of a call with per-part options", f));
        sink.trm.assign(1, spec.trm);
        sink.pit.assign(1, spec.pit);
        sink.tmp.assign(1, spec.tmp);
        PitchSteps run{sink.tmp[0].speed, false, spec.tempo};
        if (spec.pitch) {   // the pair (speed, pitch) becomes the tempo's effective speed; either step may be the identity, and then it is not run
            e = pitch_steps(spec.pit.p, spec.tempo ? spec.tmp.speed : 1000, &run);
            if (!e.empty()) refuse("join: " + e);
            sink.tmp[0].speed = run.E;
        }
        PartStages all{spec.trim ? &sink.trm[0] : nullptr, run.resample ? &sink.pit[0] : nullptr, run.tempo ? &sink.tmp[0] : nullptr};
        if (spec.formant && run.resample) {   // keep the formants around that resample: the pair (option, pitch) is resolved here too
            e = formant_pitch_error(spec.pit.p);
            if (!e.empty()) refuse("join: " + e);
            all.formant = true;
        }
        sink.stages.assign((size_t)n, all);
    }
    if (list) {   // every part's own stages, each pair (tempo, pitch) resolved to its effective speed: as ptts_formant_rows resolves a row
        sink.trm.resize((size_t)n); sink.pit.resize((size_t)n); sink.tmp.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const ptts_part_opts po = part_opts_known(list->po, i);
            const auto part_refuse = [&](const std::string& why) { if (!why.empty()) { parts[i].status = PTTS_EINVAL; refuse(strfmt("join: parts: part %d: ", i) + why); } };
            if (po.formant && !po.pitch) part_refuse("formant is set without pitch: the option keeps the formants around the pitch's resample");
            if (po.trim) part_refuse(trim_opts_error(po.trim));
            if (po.pitch) part_refuse(pitch_opts_error(po.pitch));
            if (po.formant) part_refuse(formant_opts_error(po.formant));
            if (po.tempo) part_refuse(tempo_opts_error(po.tempo));
            PartStages& st = sink.stages[(size_t)i];
            if (po.trim) { sink.trm[(size_t)i] = trim_design(*po.trim); st.trim = &sink.trm[(size_t)i]; }
            PitchSteps run{po.tempo ? po.tempo->speed_permille : 1000, false, po.tempo != nullptr};
            if (po.pitch) {
                part_refuse(pitch_steps(po.pitch->pitch_permille, run.E, &run));
                if (run.resample) { sink.pit[(size_t)i] = pitch_design(*po.pitch); st.pitch = &sink.pit[(size_t)i]; }
            }
            sink.tmp[(size_t)i].speed = run.E;
            if (run.tempo) st.tempo = &sink.tmp[(size_t)i];
            if (po.formant && po.formant->keep && st.pitch) {
                part_refuse(formant_pitch_error(st.pitch->p));
                st.formant = true;
            }
        }
    }
    if (streamed) {   // window after window only the causal stages run
        if (o.loudness) dsp_spec_loudness(spec, nullptr);
        e = dsp_window_refusal(spec);
        if (!e.empty()) refuse("join: " + e);
    }
    const int lsd = request_lsd(reqs[0]);
    int64_t bound = 0;   // the joined length the step budgets allow
    for (int i = 0; i < n; i++) {
        const ptts_request& q = reqs[i];
        e = request_error(d, q);
        if (!e.empty()) { parts[i].status = PTTS_EINVAL; out->status = PTTS_EINVAL; throw Error(PTTS_EINVAL, e); }
        const char* f = q.dsp ? "dsp" : q.loudness ? "loudness" : q.sample_rate ? "sample_rate" : q.pcm_format ? "pcm_format" : q.pcm_callback ? "pcm_callback"
                        : q.want_latents ? "want_latents" : nullptr;
        if (f) { parts[i].status = PTTS_EINVAL; refuse(strfmt("join: request %d sets %s, which belongs in the join options (ptts_join_opts) of a joined call", i, f)); }
        const int l = request_lsd(q);
        if (l != lsd) { parts[i].status = PTTS_EINVAL; refuse(strfmt("join: request %d has lsd_steps %d and request 0 has %d: the groups would leave text order", i, l, lsd)); }
        // (the trim only shortens; pitch_resample_length and tempo_length are monotone)
        const int64_t budget = (int64_t)std::min(resolve_max_steps(q), mimi_frame_limit(d)) * spf;
        const PartStages& st = sink.stages[(size_t)i];
        const int64_t shifted = st.pitch ? pitch_resample_length(budget, st.pitch->p) : budget;
        const int64_t scaled = st.tempo ? tempo_length(shifted, st.tempo->speed) : shifted;
        bound += std::max(budget, std::max(shifted, scaled)) + (i ? sink.seam[(size_t)i - 1].gap : 0);
    }
    if (bound >= kJoinMaxSamples) refuse(strfmt("join: the step budgets allow %lld samples, the joined length must stay below 2^31", (long long)bound));
    ptts_request eg{};   // the chain and the egress of the joined row, as a request states its own: results_deliver serves it like one
    eg.sample_rate = o.sample_rate; eg.pcm_format = o.pcm_format; eg.dsp = o.dsp; eg.loudness = o.loudness;
    hipStream_t s = m.stream;
    std::unique_ptr<JoinStream> js;   // (its destructor drains both streams before the hand-overs' records and the buffer go)
    try {
        sink.cap = std::max<int64_t>(bound, 1);
        sink.row = m.work(WORK_JOINED, (size_t)sink.cap * sizeof(float)).as<float>();
        if (streamed) {
            js.reset(new JoinStream(m, *so, eg));
            js->spec = spec;
            js->setup(bound, s);
        }
        // ---- the groups, as generate() cuts them; a streamed call's first group may be smaller ----
        for (int o0 = 0, size = so && so->first_group ? so->first_group : mb; o0 < n && sink.fail == PTTS_OK; o0 += size, size = mb) {
            std::vector<int> idx;
            for (int i = o0; i < std::min(n, o0 + size); i++) idx.push_back(i);
            try {
                generate_group(m, reqs, idx, nullptr, lsd, &sink);
            } catch (const Error& err) {
                for (int i : idx) if (parts[i].status == PTTS_OK) parts[i].status = err.code;
                throw;
            }
            // the group's hand-over, queued behind its k_join and in front of the next group's prefill; nothing waits for it here
            if (js && sink.fail == PTTS_OK) js->window(sink.row, sink.at, o0 + size >= n, join_stream_hold(o, sink.seam[(size_t)idx.back()]), s);
        }
        if (sink.fail != PTTS_OK) throw Error(sink.fail, sink.fail_msg);
        if (js) {   // every sample has been handed over from the buffer the result now owns
            PTTS_HIP(hipStreamSynchronize(s));
            PTTS_HIP(hipStreamSynchronize(m.stream2));
            out->n_frames = (int)std::min<int64_t>(sink.frames, INT32_MAX); out->eos_step = -1;
            out->n_samples = egress_length(eg, sink.at);
            set_result_buffer(*out, eg.pcm_format, js->host);
            js->host = nullptr;
            out->status = PTTS_OK;
            for (int i = 0; list && list->gains && i < n; i++) list->gains[i] = sink.gains[i];
            return;
        }
        // ---- the chain, once over the joined audio; the egress of one row ----
        std::vector<Delivery> g(1);
        g[0] = Delivery{&eg, out, (int)std::min<int64_t>(sink.frames, INT32_MAX), -1, false};
        g[0].n24 = sink.at;
        results_alloc(m, g, nullptr, nullptr, s);
        results_deliver(m, g, false, sink.row, sink.at, nullptr, 0, s);
        PTTS_HIP(hipStreamSynchronize(s));
        if (out->status != PTTS_OK) throw Error(out->status, "ptts-hip: out of host memory");
        for (int i = 0; list && list->gains && i < n; i++) list->gains[i] = sink.gains[i];
    } catch (const Error& err) {
        (void)hipStreamSynchronize(s);   // nothing queued still writes the buffer that goes back
        js.reset();                      // (a streamed call: both streams drained, then its buffer freed)
        ptts_free_result(out);
        result_clear(*out);
        out->status = err.code;
        throw;
    }
}

}  // namespace ptts
