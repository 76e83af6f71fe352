// staged.cpp -- engine: the device side of the staged entry points (the pieces of the pipeline callable one at a time: text embeddings, prompt, one AR
// step, the KV read-back, the decoder, noise rows, the flow direction, the speaker projection, host rows through k_resample).  The extern "C" functions
// (capi.cpp, capi_rows.cpp) check the arguments and word the refusals; they take Model::mu and select the device, then call in here.  Every function
// runs on Model::stream and returns with that stream drained, so its work buffers (runtime.h WorkSlot) are free again when the lock goes.
#include "launch_args.h"

#include <cmath>
#include <cstring>

namespace ptts {

void staged_text_embeddings(Model& m, const int64_t* ids, int64_t n, float* out) {
    DevBuf& dids = m.work(WORK_TEXT_IDS, (size_t)n * sizeof(int64_t));
    DevBuf& rows = m.work(WORK_TEXT_ROWS, (size_t)n * m.d.d_model * sizeof(float));
    PTTS_HIP(hipMemcpyAsync(dids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, m.stream));
    launch_embed_gather(m.at<float>(m.d.embed), dids.as<int64_t>(), (int)n, m.d.d_model, rows.as<float>(), m.stream);
    PTTS_HIP(hipMemcpyAsync(out, rows.p, (size_t)n * m.d.d_model * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
}

void staged_prompt(Batch& b, const float* emb, const int64_t* row_offsets) {
    Model& m = *b.m;
    const int64_t R = row_offsets[b.B];
    DevBuf& rows = m.work(WORK_PROMPT_UPLOAD, (size_t)std::max<int64_t>(R, 1) * m.d.d_model * sizeof(float));
    if (R > 0) {
        PTTS_HIP(hipMemcpyAsync(rows.p, emb, (size_t)R * m.d.d_model * sizeof(float), hipMemcpyHostToDevice, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
    }
    batch_prompt(b, rows.as<float>(), row_offsets);
    PTTS_HIP(hipStreamSynchronize(m.stream));
}

void staged_step(Batch& b, const float* frames_in, int lsd_steps, const float* noise, float* frames_out, float* eos_logits, float* last_hidden) {
    Model& m = *b.m;
    hipStream_t s = m.stream;
    const int B = b.B, ld = m.d.ldim;
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
}

void staged_read_kv(const Batch& b, int slot, int layer, float* k, float* v) {
    const Desc& d = b.m->d;
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
}

void staged_decode(Model& m, const float* latents, int n_utt, int frames, float* pcm, float* mimi_latent, float* transformer_out) {
    const Desc& d = m.d;
    size_t nl = (size_t)n_utt * frames * d.ldim, np = (size_t)n_utt * frames * d.samples_per_frame, nm = (size_t)n_utt * d.mimi_dim * frames;
    size_t nx = transformer_out ? (size_t)n_utt * frames * d.up_stride * d.mimi_dim : 0;
    DevBuf& io = m.work(WORK_DECODE_IO, (nl + np + nm + nx) * sizeof(float));
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
}

void staged_noise_rows(Model& m, uint64_t seed, float temperature, int rows, float* out) {
    const int ld = m.d.ldim;
    NoiseSpec sp{seed, temperature > 0.0f ? std::sqrt(temperature) : 0.0f, rows};
    DevBuf& sb = m.work(WORK_NOISE_ROWS_SPEC, sizeof sp);
    DevBuf& ob = m.work(WORK_NOISE_ROWS, (size_t)rows * ld * sizeof(float));
    PTTS_HIP(hipMemcpyAsync(sb.p, &sp, sizeof sp, hipMemcpyHostToDevice, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
    launch_noise_fill(sb.as<NoiseSpec>(), 1, rows, ob.as<float>(), (int64_t)rows * ld, ld, m.stream);
    PTTS_HIP(hipMemcpyAsync(out, ob.p, (size_t)rows * ld * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
}

// one Euler step of size 1 starting from zero velocity accumulation: step_core's flow part on B rows, through the many-row kernels (mk_rows) and one
// launch per residual-block piece -- neither k_skinny nor k_flow_cluster, so that it checks them independently
void staged_flow_direction(Model& m, const float* c, float sv, float tv, const float* x, int B, float* out) {
    const Desc& d = m.d;
    const int C = d.flow_dim, D = d.d_model, NA = d.ada_all.out;
    hipStream_t s = m.stream;
    DevBuf& wsb = m.work(WORK_FLOW_DIRECTION, ((size_t)B * (D + d.ldim + d.ldim + 4 * C + NA) + C) * sizeof(float));
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
    GemmArgs gc = mk_rows(m, dc, flat(D), d.cond_embed, sy, flat(C), B);
    gc.epi = EPI_SILU; gc.addvec = tc;
    launch_gemm(gc, s);
    launch_gemm(mk_rows(m, sy, flat(C), d.ada_all, ada, flat(NA), B), s);
    launch_gemm(mk_rows(m, dx, flat(d.ldim), d.input_proj, fx, flat(C), B), s);
    for (int r = 0; r < d.flow_depth; r++) {
        const auto& rb = d.rb[r];
        LnArgs ln = mkln(m, fx, flat(C), rb.ln, fh, C, B);
        ln.shift = ada + (size_t)r * 3 * C; ln.scale = ln.shift + C; ln.ldmod = NA;
        launch_layernorm(ln, s);
        GemmArgs g0 = mk_rows(m, fh, flat(C), rb.mlp0, fh2, flat(C), B);
        g0.epi = EPI_SILU;
        launch_gemm(g0, s);
        GemmArgs g2 = mk_rows(m, fh2, flat(C), rb.mlp2, fx, flat(C), B);
        g2.R = fx; g2.epi = EPI_GATE_RESADD; g2.gate = ada + (size_t)r * 3 * C + 2 * C; g2.ldg = NA;
        launch_gemm(g2, s);
    }
    LnArgs lf;   // the final layer's norm has no affine part
    lf.x = fx; lf.xmap = flat(C); lf.eps = 1e-6f; lf.y = fh; lf.ldy = C; lf.rows = B; lf.d = C;
    lf.shift = ada + (size_t)d.flow_depth * 3 * C; lf.scale = lf.shift + C; lf.ldmod = NA;
    launch_layernorm(lf, s);
    launch_gemm(mk_rows(m, fh, flat(C), d.final_linear, dout, flat(d.ldim), B), s);
    PTTS_HIP(hipMemcpyAsync(out, dout, (size_t)B * d.ldim * sizeof(float), hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipStreamSynchronize(s));
}

void staged_convert(Model& m, const float* const* in, const int64_t* n_in, int32_t n, const RateFilter* f, const int64_t* n_out, int fmt, void* const* out) {
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

// the speaker projection (EncodeVoice, onnx/voice_encode.go:23-158): an f32 weight, no bias, on the many-row kernels whatever the frame count
void speaker_project_device(Model& m, const float* lat, int64_t frames, float* out) {
    const Lin& l = m.d.speaker_proj;
    GemmArgs g = mk_rows(m, lat, flat(l.in), l, out, flat(l.out), (int)frames);
    g.w_bf16 = 0; g.bias = nullptr;
    launch_gemm(g, m.stream);
}

void staged_speaker_project(Model& m, const float* latent, int64_t frames, float* out) {
    const Lin& l = m.d.speaker_proj;
    const size_t ni = (size_t)frames * l.in, no = (size_t)frames * l.out;
    DevBuf& io = m.work(WORK_SPEAKER_IO, (ni + no) * sizeof(float));
    float* di = io.as<float>();
    float* dout = di + ni;
    PTTS_HIP(hipMemcpyAsync(di, latent, ni * sizeof(float), hipMemcpyHostToDevice, m.stream));
    speaker_project_device(m, di, frames, dout);
    PTTS_HIP(hipMemcpyAsync(out, dout, no * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
}

int64_t voice_embedding_device(Model& m, const float* pcm, int64_t n_samples, float* out, int rate) {
    const Lin& l = m.d.speaker_proj;
    const int64_t n24 = mimi_encode_samples(std::max<int64_t>(n_samples, 0), rate);
    const int64_t nf = n24 > 0 ? (n24 + m.d.enc.hop - 1) / m.d.enc.hop : 0;
    DevBuf& io = m.work(WORK_EMBEDDING_IO, (size_t)std::max<int64_t>(nf, 1) * (l.in + l.out) * sizeof(float));
    float* lat = io.as<float>();
    const int64_t f = mimi_encode_clip(m, pcm, n_samples, lat, nullptr, rate);
    float* dout = lat + (size_t)f * l.in;
    speaker_project_device(m, lat, f, dout);   // on the latents where the encoder left them
    PTTS_HIP(hipMemcpyAsync(out, dout, (size_t)f * l.out * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    PTTS_HIP(hipStreamSynchronize(m.stream));
    return f;
}

}  // namespace ptts
