// batch.cpp -- engine: the batch of FlowLM states (KV caches, step workspace), its voices, and the prompt prefill.
#include "launch_args.h"

#include <algorithm>
#include <cmath>

namespace ptts {

Batch::~Batch() {
    if (fc_stamps.p) {   // (PTTS_FC_STAMPS=<file>: the timestamps of the batch's LAST k_flow_cluster launch, one line per workgroup)
        constexpr int kWg = 8 * kFlowClusterMaxTiles;
        std::vector<unsigned long long> h((size_t)kWg * 64);
        if (const char* path = getenv("PTTS_FC_STAMPS"))
            if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), fc_stamps.p, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
                if (FILE* f = fopen(path, "a")) {
                    for (int blk = 0; blk < kWg; blk++) {
                        if (!h[(size_t)blk * 64]) continue;
                        fprintf(f, "wg %d:", blk);
                        for (int i = 0; i < 64; i++) fprintf(f, " %llu", h[(size_t)blk * 64 + i]);
                        fprintf(f, "\n");
                    }
                    fprintf(f, "\n");
                    fclose(f);
                }
    }
    drop_graphs();
    if (n_active_pinned) (void)hipHostFree(n_active_pinned);
    if (rows_pinned) (void)hipHostFree(rows_pinned);
}

void Batch::drop_graphs() {
    for (auto& set : graphs) for (auto& row : set) for (hipGraphExec_t& g : row) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto& gs : graph_steps) gs[0] = gs[1] = 0;
}

Batch* batch_new(Model& m, int n_slots, int cap, int max_steps) {
    if (n_slots <= 0) throw Error(PTTS_EINVAL, "ptts-hip: batch needs at least one slot");
    if (n_slots > kStepMaxRows) throw Error(PTTS_EINVAL, strfmt("ptts-hip: a batch takes at most %d slots (the AR step's kernels), asked for %d", kStepMaxRows, n_slots));
    if (cap <= 0 || cap > ROPE_SEQ) throw Error(PTTS_EINVAL, strfmt("ptts-hip: kv capacity %d outside (0, %d] (RoPE table rows, flow_transformer.go:505)", cap, ROPE_SEQ));
    m.use_device();
    const Desc& d = m.d;
    std::unique_ptr<Batch> b(new Batch());
    b->m = &m;
    b->B = n_slots;
    b->cap = cap;
    b->max_steps = std::max(1, max_steps);
    const size_t B = (size_t)n_slots;
    size_t kvbytes = (size_t)d.n_layers * B * d.heads * cap * d.hd * b->kv_elem();
    b->kcache.ensure(kvbytes);
    b->vcache.ensure(kvbytes);
    // the step attention re-reads a valid row for key slots past the end (zero weight): every row must hold finite data
    PTTS_HIP(hipMemsetAsync(b->kcache.p, 0, kvbytes, m.stream));
    PTTS_HIP(hipMemsetAsync(b->vcache.p, 0, kvbytes, m.stream));
    b->state_i32.ensure((9 * B + 1) * sizeof(int32_t));
    b->state_f32.ensure(B * sizeof(float));
    int32_t* s = b->state_i32.as<int32_t>();
    b->st.kv_len = s; b->st.active = s + B; b->st.step = s + 2 * B; b->st.countdown = s + 3 * B;
    b->st.n_frames = s + 4 * B; b->st.eos_step = s + 5 * B; b->st.max_steps = s + 6 * B;
    b->st.frames_after_eos = s + 7 * B; b->st.broke = s + 8 * B; b->st.n_active = s + 9 * B;
    b->st.eos_threshold = b->state_f32.as<float>();
    b->kv_len_host.assign(B, 0);
    b->pre_k.ensure((size_t)B * sizeof(void*)); b->pre_v.ensure((size_t)B * sizeof(void*)); b->pre_len.ensure((size_t)B * sizeof(int32_t));
    b->pre_k_host.assign(B, nullptr); b->pre_v_host.assign(B, nullptr); b->pre_len_host.assign(B, 0);
    const size_t f = sizeof(float);
    const int NA = d.ada_all.out;
    b->in_raw.ensure(B * d.ldim * f); b->in32.ensure(B * d.ldim * f);
    b->x.ensure(B * d.d_model * f); b->xn.ensure(B * std::max(d.d_model, d.flow_dim) * f);
    b->qkv.ensure(B * 3 * d.d_model * f); b->attn.ensure(B * d.d_model * f);
    b->ff.ensure(B * d.ffn * f); b->last.ensure(B * d.d_model * f); b->eos.ensure(B * f);
    b->sy.ensure(B * d.flow_dim * f); b->ada.ensure(B * NA * f);
    b->fx.ensure(B * d.flow_dim * f); b->fh.ensure(B * d.flow_dim * f); b->fh2.ensure(B * d.flow_dim * f);
    b->cur.ensure(B * d.ldim * f);
    b->partial.ensure((size_t)16 * B * std::max(d.d_model, d.flow_dim) * f);
    b->latents.ensure(B * b->max_steps * d.ldim * f);
    {
        StepFinish sf{b->st, b->eos.as<float>(), b->latents.as<float>(), (int64_t)b->max_steps * d.ldim, (int32_t)d.ldim, StepChain{}};
        StepOpenLinears lin;
        b->chain_ok = open_linears(*b, lin) && step_open_mfma_ok(lin, d.ldim) && ((int64_t)b->max_steps * d.ldim) % 2 == 0 &&
                      (lin.w_bf16 != 0) == (d.final_linear.bf16 != 0 || d.final_linear.wt_i8 != 0);   // the chained form takes the 32-deep linears' type from the step kernel's weight type
        // two copies: a step that reads fx / cur (par 0) opens the next one in fx2 / cur2, and the other way round
        b->fx2.ensure(B * d.flow_dim * f); b->cur2.ensure(B * d.ldim * f);
        StepFinish sf2[2] = {sf, sf};
        sf2[0].ch = StepChain{lin.w_in, lin.b_in, lin.x, lin.d_in, lin.w_pj, lin.b_pj, b->fx2.as<float>(), lin.d_pj, m.at<float>(d.bos), b->cur2.as<float>(), lin.w_bf16, b->chain_ok ? 1 : 0};
        sf2[1].ch = StepChain{lin.w_in, lin.b_in, lin.x, lin.d_in, lin.w_pj, lin.b_pj, b->fx.as<float>(), lin.d_pj, m.at<float>(d.bos), b->cur.as<float>(), lin.w_bf16, b->chain_ok ? 1 : 0};
        b->fin_dev.ensure(sizeof sf2);
        h2d(b->fin_dev.p, sf2, sizeof sf2, m.stream);
    }
    {   // flow_cluster.hip: bf16 step copies of every residual block's linears, the width it is built for
        const char* sw = getenv("PTTS_FLOW_CLUSTER");   // A/B switch, read per batch: 0 = the 2 x depth launches (tests compare the two forms bit for bit)
        const bool off = sw && sw[0] == '0';
        bool ok = !off && !m.fc_disabled.load() && d.flow_dim == 512 && d.flow_depth > 0 && d.flow_depth <= FC_MAX_DEPTH && n_slots <= kStepMaxRows &&
                  flow_cluster_fits(n_slots, m.device);   // (every workgroup of the grid resident at once: its hand-offs spin on its peers)
        for (int r = 0; ok && r < d.flow_depth; r++) {
            const auto& rb = d.rb[r];
            for (const Lin* l : {&rb.mlp0, &rb.mlp2}) ok = ok && l->in == 512 && l->out == 512 && l->bf16 && !l->wt_i8 && l->wt != NONE && l->b != NONE;
            ok = ok && rb.ln.w != NONE && rb.ln.b != NONE && rb.ln.d == 512;
        }
        b->fc_ok = ok;
        if (ok) {
            b->fc_xbuf.ensure(flow_cluster_xbuf_bytes(n_slots)); b->fc_sync.ensure(kFlowClusterSyncBytes);
            PTTS_HIP(hipMemsetAsync(b->fc_xbuf.p, 0, flow_cluster_xbuf_bytes(n_slots), m.stream));
            PTTS_HIP(hipMemsetAsync(b->fc_sync.p, 0, kFlowClusterSyncBytes, m.stream));
            if (getenv("PTTS_FC_STAMPS")) { b->fc_stamps.ensure((size_t)8 * kFlowClusterMaxTiles * 64 * 8); PTTS_HIP(hipMemsetAsync(b->fc_stamps.p, 0, (size_t)8 * kFlowClusterMaxTiles * 64 * 8, m.stream)); }
        }
    }
    {   // tall.hip: from kTallMinRows rows the layer's in_proj / linear1 / linear2 run as 64 x 64-tile products on bf16 row planes
        const char* sw = getenv("PTTS_TALL");   // A/B switch, read per batch: 0 = k_skinny for every row count
        bool ok = !(sw && sw[0] == '0') && n_slots >= kTallMinRows && (d.d_model == 512 || d.d_model == 1024) && d.ffn % 128 == 0;
        for (int l = 0; ok && l < d.n_layers; l++) {
            const auto& L = d.layers[l];
            for (const Lin* li : {&L.in_proj, &L.l1, &L.l2}) ok = ok && li->bf16 && !li->wt_i8 && li->wt != NONE && li->out % 4 == 0;
            ok = ok && L.in_proj.in == d.d_model && L.l1.in == d.d_model && L.l1.out == d.ffn && L.l2.in == d.ffn && L.l2.out == d.d_model;
            ok = ok && L.n1.w != NONE && L.n1.b != NONE && L.n2.w != NONE && L.n2.b != NONE;
        }
        b->tall_ok = ok;
        if (ok) { b->tp_a.ensure(2 * B * d.d_model * sizeof(uint16_t)); b->tp_f.ensure(2 * B * d.ffn * sizeof(uint16_t)); }
    }
    PTTS_HIP(hipHostMalloc((void**)&b->n_active_pinned, sizeof(int32_t) * (size_t)(2 + 2 * B), hipHostMallocDefault));
    PTTS_HIP(hipHostMalloc((void**)&b->rows_pinned, sizeof(PcmRow) * std::max<size_t>((size_t)B, 1), hipHostMallocDefault));
    batch_reset(*b);
    return b.release();
}

void batch_reset(Batch& b) {
    b.opened = false;
    hipStream_t s = b.m->stream;
    const int B = b.B;
    launch_fill_i32(b.st.kv_len, 0, B, s);
    b.kv_bound = 0;
    // the decoder runs every utterance of a batch over the longest one's frames, and its window attention gives the keys of later frames weight zero,
    // not a skip (attn_window.hip: a 32-query tile spans two frames): frames no step of THIS run writes must hold finite data -- not fresh memory, not
    // the NaN frames an earlier tenant of the slot may have left -- or 0 * NaN reaches the utterance's last frame
    PTTS_HIP(hipMemsetAsync(b.latents.p, 0, (size_t)B * b.max_steps * b.m->d.ldim * sizeof(float), s));
    launch_fill_i32(b.st.active, 1, B, s);
    launch_fill_i32(b.st.step, 0, B, s);
    launch_fill_i32(b.st.countdown, -1, B, s);
    launch_fill_i32(b.st.n_frames, 0, B, s);
    launch_fill_i32(b.st.eos_step, -1, B, s);
    launch_fill_i32(b.st.max_steps, 0x7fffffff, B, s);
    launch_fill_i32(b.st.frames_after_eos, 0, B, s);
    launch_fill_i32(b.st.broke, 0, B, s);
    launch_fill_i32(b.st.n_active, B, 1, s);
    std::vector<float> thr((size_t)B, INFINITY);
    h2d(b.st.eos_threshold, thr.data(), thr.size() * sizeof(float), s);
    std::fill(b.kv_len_host.begin(), b.kv_len_host.end(), 0);
    std::fill(b.pre_len_host.begin(), b.pre_len_host.end(), 0);
    launch_fill_i32(b.pre_len.as<int32_t>(), 0, B, s);
    b.has_noise = false;
}

static void check_voice(const Desc& d, const float* const* caches, const int64_t* steps, const int64_t* offsets, int64_t cap) {
    for (int l = 0; l < d.n_layers; l++) {  // flow_transformer.go:538-549
        if (!caches[l]) throw Error(PTTS_EINVAL, strfmt("native: voice model state module \"transformer.layers.%d.self_attn\" missing cache", l));
        if (offsets[l] < 0) throw Error(PTTS_EINVAL, strfmt("native: voice model state module \"transformer.layers.%d.self_attn\" has negative offset %lld", l, (long long)offsets[l]));
        if (offsets[l] > steps[l]) throw Error(PTTS_EINVAL, strfmt("native: voice model state module \"transformer.layers.%d.self_attn\" offset %lld exceeds cache length %lld", l, (long long)offsets[l], (long long)steps[l]));
        if (offsets[l] != offsets[0]) throw Error(PTTS_EINVAL, "ptts-hip: per-layer voice offsets differ; one offset per utterance is supported");
        if (offsets[l] > cap) throw Error(PTTS_EINVAL, "ptts-hip: voice state longer than the KV capacity");
    }
}

Voice* voice_create(Model& m, const float* const* caches, const int64_t* steps, const int64_t* offsets) {
    const Desc& d = m.d;
    check_voice(d, caches, steps, offsets, ROPE_SEQ);
    std::unique_ptr<Voice> v(new Voice());
    v->m = &m;
    v->device = m.device;
    v->offset = (int)offsets[0];
    const size_t lb = v->layer_bytes();
    v->k.ensure(std::max<size_t>(lb * d.n_layers, 256));
    v->v.ensure(std::max<size_t>(lb * d.n_layers, 256));
    for (int l = 0; l < d.n_layers; l++) {
        size_t n = (size_t)2 * steps[l] * d.heads * d.hd;
        DevBuf& raw = m.work(WORK_VOICE_RAW, n * sizeof(float));
        h2d(raw.p, caches[l], n * sizeof(float), m.stream);
        launch_voice_scatter(raw.as<float>(), (int)steps[l], d.heads, d.hd, v->offset, 0, (char*)v->k.p + lb * l, (char*)v->v.p + lb * l,
                             m.opts.kv == PTTS_KV_BF16, v->offset, m.stream);
        PTTS_HIP(hipStreamSynchronize(m.stream));
    }
    return v.release();
}

// a voice is device memory in the cache layout: every engine on the same GPU with the same cache geometry can read it
bool voice_usable_by(const Voice& v, const Model& m) {
    return v.m == &m || (v.m && v.m->device == m.device && v.m->opts.kv == m.opts.kv && v.m->d.n_layers == m.d.n_layers && v.m->d.heads == m.d.heads &&
                         v.m->d.hd == m.d.hd);
}

void batch_apply_voice(Batch& b, const Voice& v, const std::vector<int32_t>& slots) {
    Model& m = *b.m;
    hipStream_t io = b.io_stream ? b.io_stream : m.stream;
    const Desc& d = m.d;
    if (!voice_usable_by(v, m)) throw Error(PTTS_EINVAL, "ptts-hip: voice belongs to another model");
    if (v.offset > b.cap) throw Error(PTTS_EINVAL, "ptts-hip: voice state longer than the KV capacity");
    DevBuf& ds = m.work(WORK_VOICE_SLOTS, slots.size() * sizeof(int32_t));
    h2d(ds.p, slots.data(), slots.size() * sizeof(int32_t), io);
    const size_t lb = v.layer_bytes();
    for (int l = 0; l < d.n_layers; l++)
        launch_voice_apply((const char*)v.k.p + lb * l, (const char*)v.v.p + lb * l, v.offset, d.heads, d.hd, ds.as<int32_t>(), (int)slots.size(),
                           b.kc(l), b.vc(l), (int)b.kv_elem(), b.cap, io);
    for (int32_t sl : slots) {
        b.kv_len_host[sl] = v.offset;
        b.kv_bound = std::max(b.kv_bound, (int)v.offset);
        b.pre_k_host[sl] = v.k.p; b.pre_v_host[sl] = v.v.p; b.pre_len_host[sl] = v.offset;
    }
    if (b.slot_local) return;   // continuous batch: the admit kernel writes these entries for the slots it fills; the others are live
    h2d(b.st.kv_len, b.kv_len_host.data(), (size_t)b.B * sizeof(int32_t), io);
    h2d(b.pre_k.p, b.pre_k_host.data(), (size_t)b.B * sizeof(void*), io);
    h2d(b.pre_v.p, b.pre_v_host.data(), (size_t)b.B * sizeof(void*), io);
    h2d(b.pre_len.p, b.pre_len_host.data(), (size_t)b.B * sizeof(int32_t), io);
}

void batch_set_voice(Batch& b, int slot, const float* const* caches, const int64_t* steps, const int64_t* offsets) {
    Model& m = *b.m;
    hipStream_t io = b.io_stream ? b.io_stream : m.stream;
    const Desc& d = m.d;
    if (slot < 0 || slot >= b.B) throw Error(PTTS_EINVAL, "ptts-hip: voice state slot out of range");
    check_voice(d, caches, steps, offsets, b.cap);
    for (int l = 0; l < d.n_layers; l++) {
        size_t n = (size_t)2 * steps[l] * d.heads * d.hd;
        DevBuf& raw = m.work(WORK_VOICE_RAW, n * sizeof(float));
        h2d(raw.p, caches[l], n * sizeof(float), io);
        launch_voice_scatter(raw.as<float>(), (int)steps[l], d.heads, d.hd, (int)offsets[l], slot, b.kc(l), b.vc(l),
                             m.opts.kv == PTTS_KV_BF16, b.cap, io);
        PTTS_HIP(hipStreamSynchronize(io));
    }
    b.kv_len_host[slot] = (int32_t)offsets[0];
    b.kv_bound = std::max(b.kv_bound, (int)offsets[0]);
    b.pre_len_host[slot] = 0;
    if (b.slot_local) return;
    h2d(b.st.kv_len + slot, &b.kv_len_host[slot], sizeof(int32_t), io);
    h2d(b.pre_len.as<int32_t>() + slot, &b.pre_len_host[slot], sizeof(int32_t), io);
}

// FlowLM.PromptText -> flowTransformer.prefill (flow_lm.go:155-187, flow_transformer.go:749-771), all slots at once,
// ragged prompts packed as rows.  The hidden output is discarded by the reference, so the last layer stops after
// its keys/values are in the cache.
void batch_prompt(Batch& b, const float* rows_dev, const int64_t* row_offsets) {
    Model& m = *b.m;
    const Desc& d = m.d;
    hipStream_t s = b.io_stream ? b.io_stream : m.stream;
    const int B = b.B, D = d.d_model;
    const int64_t R64 = row_offsets[B];
    if (R64 == 0) return;
    if (R64 < 0 || R64 > (1 << 24)) throw Error(PTTS_EINVAL, "ptts-hip: prompt row count out of range");
    const int R = (int)R64;
    std::vector<int32_t> off((size_t)B + 1);
    for (int sl = 0; sl < B; sl++) {
        int64_t t = row_offsets[sl + 1] - row_offsets[sl];
        if (t < 0) throw Error(PTTS_EINVAL, "ptts-hip: prompt row offsets must be non-decreasing");
        if (b.kv_len_host[sl] + t > b.cap) throw Error(PTTS_EINVAL, strfmt("ptts-hip: prompt of %lld rows does not fit KV capacity %d (offset %d)", (long long)t, b.cap, b.kv_len_host[sl]));
        off[(size_t)sl] = (int32_t)row_offsets[sl];
    }
    off[(size_t)B] = R;
    const size_t f = sizeof(float);
    // one upload: row -> slot, row -> position, and per slot the first row / first position (the ragged-segment view of the same)
    const RaggedMeta meta = ragged_meta(off.data(), b.kv_len_host.data(), B);
    int32_t* d_meta = m.work(WORK_PROMPT_META, meta.table.size() * sizeof(int32_t)).as<int32_t>();
    const int32_t* d_slot = meta.row_seg(d_meta);
    const int32_t* d_pos = meta.row_pos(d_meta);
    h2d(d_meta, meta.table.data(), meta.table.size() * sizeof(int32_t), s);
    DevBuf& wsb = m.work(WORK_PROMPT_ACT, ((size_t)R * (size_t)(D + D + 3 * D + D + d.ffn)) * f);
    float* px = wsb.as<float>();
    float* pxn = px + (size_t)R * D;
    float* pqkv = pxn + (size_t)R * D;
    float* pattn = pqkv + (size_t)R * 3 * D;
    float* pff = pattn + (size_t)R * D;
    PTTS_HIP(hipMemcpyAsync(px, rows_dev, (size_t)R * D * f, hipMemcpyDeviceToDevice, s));
    const bool kvb = m.opts.kv == PTTS_KV_BF16;
    // a short prompt at a small batch (R <= 64 rows): linear2 (K = 4 x d_model) runs as the step's split-K kernel and its
    // partial sums are added by the next layer's LayerNorm launch, like in the AR step; otherwise it is one tile GEMM
    PendingSum pend;   // (its planes: [S][R][D])
    for (int l = 0; l < d.n_layers; l++) {
        const auto& L = d.layers[l];
        {
            LnArgs ln = mkln(m, px, flat(D), L.n1, pxn, D, R);
            ln.pend = pend;
            launch_layernorm(ln, s);
            pend = PendingSum{};
        }
        {
            GemmArgs gq = mk(m, pxn, flat(D), L.in_proj, pqkv, flat(3 * D), R);
            gq.rope_cos = m.at<float>(d.rope_cos); gq.rope_sin = m.at<float>(d.rope_sin);   // q and k are rotated in the epilogue
            gq.rope_cols = 2 * D; gq.rope_hd = d.hd; gq.rope_row_pos = d_pos;
            if (!launch_gemm_rope(gq, s)) {
                gq.rope_cos = gq.rope_sin = nullptr; gq.rope_row_pos = nullptr;
                launch_gemm(gq, s);
                launch_rope_rows(pqkv, flat(3 * D), 0, d.heads, d.hd, d_pos, 0, 0, R, m.at<float>(d.rope_cos), m.at<float>(d.rope_sin), s);
                launch_rope_rows(pqkv, flat(3 * D), D, d.heads, d.hd, d_pos, 0, 0, R, m.at<float>(d.rope_cos), m.at<float>(d.rope_sin), s);
            }
        }
        launch_kv_append(pqkv, 3 * D, D, d.heads, d.hd, d_slot, d_pos, R, b.kc(l), b.vc(l), kvb, b.cap, s);
        if (l == d.n_layers - 1) break;
        launch_attention(attn_ragged_args(kv_layer(b, l), meta, d_meta, pqkv, 3 * D, -1, pattn, D), s);
        GemmArgs go = mk(m, pattn, flat(D), L.out_proj, px, flat(D), R);
        go.R = px; go.epi = EPI_RESADD;
        launch_gemm(go, s);
        launch_layernorm(mkln(m, px, flat(D), L.n2, pxn, D, R), s);
        GemmArgs g1 = mk(m, pxn, flat(D), L.l1, pff, flat(d.ffn), R);
        g1.epi = EPI_GELU;
        launch_gemm(g1, s);
        GemmArgs g2 = mk(m, pff, flat(d.ffn), L.l2, px, flat(D), R);
        const int S = R <= kSkinnyChunkRows ? pick_split(std::min(R, 64), D, d.ffn) : 1;
        GemmArgs g2c = g2;
        g2c.M = std::min(R, 64);
        if (S > 1 && skinny_supported(g2c, S)) {   // (64-row chunks of the split step kernel; the planes of all chunks form one [S][R][D] operand)
            DevBuf& pb = m.work(WORK_PREFILL_PLANES, (size_t)S * R * D * f);
            for (int r0 = 0; r0 < R; r0 += 64) {
                g2c = g2;
                g2c.M = std::min(64, R - r0);
                g2c.A = g2.A + (int64_t)r0 * d.ffn;
                g2c.zstride = (int64_t)R * D;
                launch_skinny(g2c, SkinnyFuse{}, S, pb.as<float>() + (size_t)r0 * D, s);
            }
            pend = PendingSum{pb.as<float>(), S, (int64_t)R * D, m.at<float>(L.l2.b)};
        } else {
            // many rows, few row panels: a 4 d_model-deep product on ~100-200 blocks leaves one wave per SIMD waiting on its own
            // loads -- cut K in four (four times the blocks) and let the next layer's LayerNorm launch add the planes
            GemmArgs gs = g2;
            gs.bias = nullptr; gs.kslice = 1024; gs.zstride = (int64_t)R * D;
            const int Sg = (d.ffn + gs.kslice - 1) / gs.kslice;
            if (R < 16384 && Sg > 1 && Sg <= 8) {
                DevBuf& pb = m.work(WORK_PREFILL_PLANES, (size_t)Sg * R * D * f);
                gs.C = pb.as<float>(); gs.cmap = flat(D);
                if (gemm5_supported(gs) || gemm3_supported(gs)) {
                    if (gemm5_supported(gs)) launch_gemm5(gs, s);   // (bf16 weights from 1024 rows; the same k order within a slice: the same planes)
                    else launch_gemm3(gs, s);
                    pend = PendingSum{pb.as<float>(), Sg, (int64_t)R * D, m.at<float>(L.l2.b)};
                    continue;
                }
            }
            g2.R = px; g2.epi = EPI_RESADD;
            launch_gemm(g2, s);
        }
    }
    for (int sl = 0; sl < B; sl++) {
        b.kv_len_host[sl] += (int32_t)(row_offsets[sl + 1] - row_offsets[sl]);
        b.kv_bound = std::max(b.kv_bound, (int)b.kv_len_host[sl]);
    }
    if (!b.slot_local) h2d(b.st.kv_len, b.kv_len_host.data(), (size_t)B * sizeof(int32_t), s);
}

}  // namespace ptts
