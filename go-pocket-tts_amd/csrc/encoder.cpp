// encoder.cpp -- the Mimi encoder: 24 kHz mono PCM -> [frames, mimi_dim] latents (mimi.encode_to_latent, onnx/voice_encode.go:23-158), the first
// half of voice cloning; ptts_speaker_project is the second.
//
// PARITY UNPINNED: inferred architecture, no reference fixture.  The reference has no native encoder (mimi.go:14,791-794 returns
// ErrMimiEncoderNotImplemented); its semantics exist only inside the exported ONNX graph.  The chain below mirrors the decoder that mimi.go:546-637
// loads, as Mimi's SEANet encoder mirrors its decoder:
//   head conv (1 -> f, stride 1) -> 3 x [residual block, ELU, causal conv with stride k/2] -> ELU -> tail conv (8f -> mimi_dim, stride 1)
//   -> transformer (the decoder transformer's layer, positions from 0 per clip) -> downsample conv (stride k/2, no bias) = the raw latent
// Every convolution is causal with zero history (k - s zero rows in front of a stride-s conv), and a clip is padded with zeros to a whole number of
// frames.  Channels-last activations; a stride-s convolution is a product whose A rows are the overlapping windows s * Cin apart (RowMap::ld).
#include "launch_args.h"

#include <algorithm>
#include <cstring>

namespace ptts {

namespace {

GemmArgs conv_gemm(const Model& m, const float* A, int64_t lda, const Lin& l, float* C, int64_t ldc, int M) {
    GemmArgs g;
    g.A = A; g.amap = flat(lda);
    g.W = m.arena + l.w; g.w_bf16 = l.bf16; g.ldw = l.in;
    g.bias = m.at<float>(l.b);
    g.C = C; g.cmap = flat(ldc);
    g.M = M; g.N = l.out; g.K = l.in;
    return g;
}

// one clip's activations inside the encoder workspace: every buffer holds `pad` zero history rows in front of its L rows
struct EncWs {
    int64_t L[4] = {0, 0, 0, 0};   // rows at the head's rate and after each down conv (the last is the transformer's rate)
    int64_t frames = 0;
    int P[3] = {0, 0, 0}, Ph[3] = {0, 0, 0}, P3 = 0, Px = 0, Pp = 0;
    float *pcm = nullptr, *u[3] = {nullptr, nullptr, nullptr}, *uo[3] = {nullptr, nullptr, nullptr}, *h[3] = {nullptr, nullptr, nullptr};
    float *u3 = nullptr, *x = nullptr, *qkv = nullptr, *n1 = nullptr, *attn = nullptr, *ff = nullptr, *partial = nullptr;
    size_t floats = 0;
};

// the layout for a clip of `frames` frames; base == nullptr only measures (sizes grow with frames, so the longest clip's layout bounds all)
EncWs enc_layout(const Desc& d, int64_t frames, float* base) {
    const auto& e = d.enc;
    EncWs w;
    w.frames = frames;
    w.L[3] = frames * e.ds_s;
    w.L[2] = w.L[3] * e.down_s[2];
    w.L[1] = w.L[2] * e.down_s[1];
    w.L[0] = w.L[1] * e.down_s[0];
    w.Pp = e.head_k - 1;
    for (int j = 0; j < 3; j++) {
        w.P[j] = std::max({2, e.rb_k1[j] - 1, e.down_k[j] - e.down_s[j]});   // (k_resblock reads two rows of history)
        w.Ph[j] = e.rb_k2[j] - 1;
    }
    w.P3 = e.tail_k - 1;
    w.Px = e.ds_k - e.ds_s;
    const int C = d.mimi_dim;
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) & ~(size_t)63; return p; };
    w.pcm = take((size_t)(w.Pp + w.L[0]));
    for (int j = 0; j < 3; j++) {
        const size_t rows = (size_t)(w.P[j] + w.L[j]);
        w.u[j] = take(rows * e.ch[j]);
        w.uo[j] = take(rows * e.ch[j]);
        w.h[j] = take((size_t)(w.Ph[j] + w.L[j]) * e.hidden[j]);
    }
    w.u3 = take((size_t)(w.P3 + w.L[3]) * e.ch[3]);
    w.x = take((size_t)(w.Px + w.L[3]) * C);
    w.qkv = take((size_t)w.L[3] * 3 * C);
    w.n1 = take((size_t)w.L[3] * C);
    w.attn = take((size_t)w.L[3] * C);
    w.ff = take((size_t)w.L[3] * d.mimi_ffn);
    w.partial = take((size_t)enc_ds_splits((int)frames, C, e.ds.in) * frames * C);
    w.floats = off;
    return w;
}

void zero(float* p, size_t n, hipStream_t s) { if (n) PTTS_HIP(hipMemsetAsync(p, 0, n * sizeof(float), s)); }

// rows [pad, pad + rows) of a channels-last buffer -> host [rows][c] (stage observation)
void stage_out(float* host, const float* buf, int pad, int64_t rows, int c, hipStream_t s) {
    if (host) PTTS_HIP(hipMemcpyAsync(host, buf + (size_t)pad * c, (size_t)rows * c * sizeof(float), hipMemcpyDeviceToHost, s));
}

// x + c1(elu(c3(elu(x)))) at width C over rows [0, L) of u; uo receives elu of the sum (its only readers, the down convs, apply ELU first)
void enc_resblock(Model& m, const EncWs& w, int j, hipStream_t s) {
    const Desc& d = m.d;
    const auto& e = d.enc;
    const int C = e.ch[j], H = e.hidden[j];
    const int64_t L = w.L[j];
    ResArgs ra;
    ra.u = w.u[j]; ra.u_bs = (int64_t)(w.P[j] + L) * C; ra.pad = w.P[j]; ra.uo = w.uo[j];
    ra.w1 = m.at<uint8_t>(e.rb1[j].wf); ra.w1_lo = m.at<uint8_t>(e.rb1[j].wf_lo); ra.b1 = m.at<float>(e.rb1[j].b);
    ra.w2 = m.at<uint8_t>(e.rb2[j].wf); ra.w2_lo = m.at<uint8_t>(e.rb2[j].wf_lo); ra.b2 = m.at<float>(e.rb2[j].b);
    ra.B = 1; ra.L = (int)L; ra.t0 = 0; ra.t1 = (int)L;
    ra.C = C; ra.H = H; ra.k1 = e.rb_k1[j]; ra.k2 = e.rb_k2[j]; ra.w_bf16 = e.rb1[j].bf16;
    if (e.rb1[j].wf != NONE && e.rb2[j].wf != NONE && e.rb1[j].bf16 == e.rb2[j].bf16 && resblock_supported(ra)) {
        launch_resblock(ra, s);
        return;
    }
    // two products (the decoder's form for the widths k_resblock does not take)
    GemmArgs g1 = conv_gemm(m, w.u[j] + (size_t)(w.P[j] - (e.rb_k1[j] - 1)) * C, C, e.rb1[j], w.h[j] + (size_t)w.Ph[j] * H, H, (int)L);
    g1.aop = AOP_ELU; g1.epi = EPI_ELU;
    if (C % 64 == 0 && e.rb1[j].in == e.rb_k1[j] * C) { g1.win_taps = e.rb_k1[j]; g1.win_c = C; }
    launch_gemm(g1, s);
    GemmArgs g2 = conv_gemm(m, w.h[j], H, e.rb2[j], w.uo[j] + (size_t)w.P[j] * C, C, (int)L);
    g2.R = w.u[j] + (size_t)w.P[j] * C; g2.epi = EPI_RESADD_ELU;
    launch_gemm(g2, s);
}

}  // namespace

int64_t mimi_encode_max_frames(const Desc& d) { return d.enc.ds_s > 0 ? ROPE_SEQ / d.enc.ds_s : 0; }

void require_encoder(const Desc& d) {
    if (!d.enc.present) throw Error(PTTS_EFORMAT, "load mimi encoder: tensor \"mimi.encoder.model.0.conv.weight\" not found in the model weights");
}

void mimi_encode_stage_shapes(const Desc& d, int64_t n_samples, int64_t* shapes) {
    const auto& e = d.enc;
    const EncWs w = enc_layout(d, n_samples > 0 ? (n_samples + e.hop - 1) / e.hop : 0, nullptr);
    const int64_t sh[kEncStages][2] = {{w.L[0], e.ch[0]}, {w.L[0], e.ch[0]}, {w.L[1], e.ch[1]}, {w.L[1], e.ch[1]}, {w.L[2], e.ch[2]},
                                       {w.L[2], e.ch[2]}, {w.L[3], e.ch[3]}, {w.L[3], d.mimi_dim}, {w.L[3], d.mimi_dim}, {w.frames, d.mimi_dim}};
    std::memcpy(shapes, sh, sizeof sh);
}

int64_t mimi_encode_samples(int64_t n_samples, int rate) {
    if (rate == kNativeRate) return n_samples;
    const std::string err = rate_pair_error(rate, kNativeRate);
    if (!err.empty()) throw Error(PTTS_EINVAL, "voice encode: " + err);
    return resample_length(n_samples, rate, kNativeRate);
}

// the frames of a clip of n_samples at `rate` (resampled to 24 kHz); PTTS_EINVAL naming the resampled length beyond the cap
static int64_t clip_frames(const Desc& d, int64_t n_samples, int rate) {
    const int64_t n24 = mimi_encode_samples(n_samples, rate);
    const int64_t frames = (n24 + d.enc.hop - 1) / d.enc.hop;
    if (frames > mimi_encode_max_frames(d)) {
        if (rate != kNativeRate)
            throw Error(PTTS_EINVAL, strfmt("voice encode: %lld samples at %d Hz resample to %lld samples at 24000 Hz (%lld frames), more than the %lld frames one "
                                            "clip may have", (long long)n_samples, rate, (long long)n24, (long long)frames, (long long)mimi_encode_max_frames(d)));
        throw Error(PTTS_EINVAL, strfmt("voice encode: %lld samples (%lld frames) exceed the %lld frames one clip may have", (long long)n_samples,
                                        (long long)frames, (long long)mimi_encode_max_frames(d)));
    }
    return frames;
}

int64_t mimi_encode_clip(Model& m, const float* pcm, int64_t n_samples, float* lat_dev, float* const* stages, int rate) {
    const Desc& d = m.d;
    const auto& e = d.enc;
    require_encoder(d);
    if (!pcm || n_samples <= 0) throw Error(PTTS_EINVAL, "voice encode: audio is empty");
    const int64_t n24 = mimi_encode_samples(n_samples, rate);
    const int64_t frames = clip_frames(d, n_samples, rate);
    hipStream_t s = m.stream;
    const int C = d.mimi_dim;
    EncWs w = enc_layout(d, frames, nullptr);
    DevBuf& wsb = m.work(WORK_ENCODER, w.floats * sizeof(float));
    w = enc_layout(d, frames, wsb.as<float>());
    float* const* st = stages;
    // zero history in front of every buffer, zero samples after the clip's end
    zero(w.pcm, (size_t)(w.Pp + w.L[0]), s);
    if (rate == kNativeRate) PTTS_HIP(hipMemcpyAsync(w.pcm + w.Pp, pcm, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, s));
    else {   // the clip at its own rate, resampled by k_resample straight into the encoder's input (no host round trip)
        DevBuf& src = m.work(WORK_ENCODER_CLIP, (size_t)n_samples * sizeof(float));
        PTTS_HIP(hipMemcpyAsync(src.p, pcm, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, s));
        resample_launch(m, {resample_row(rate_filter(m, rate, kNativeRate, s), src.as<float>(), n_samples, w.pcm + w.Pp, 0, n24, RS_F32)}, s);
    }
    for (int j = 0; j < 3; j++) {
        zero(w.u[j], (size_t)w.P[j] * e.ch[j], s);
        zero(w.uo[j], (size_t)w.P[j] * e.ch[j], s);
        zero(w.h[j], (size_t)w.Ph[j] * e.hidden[j], s);
    }
    zero(w.u3, (size_t)w.P3 * e.ch[3], s);
    zero(w.x, (size_t)w.Px * C, s);
    // head: 1 -> f channels, stride 1 (encoder.hip k_enc_head)
    launch_enc_head(w.pcm, m.arena + e.head.w, e.head.bf16, m.at<float>(e.head.b), w.L[0], e.ch[0], e.head_k, w.u[0] + (size_t)w.P[0] * e.ch[0], e.ch[0], s);
    if (st) stage_out(st[0], w.u[0], w.P[0], w.L[0], e.ch[0], s);
    for (int j = 0; j < 3; j++) {
        enc_resblock(m, w, j, s);
        if (st) stage_out(st[1 + 2 * j], w.uo[j], w.P[j], w.L[j], e.ch[j], s);
        // ELU (already applied: uo) -> causal conv with stride k/2: output row t reads input rows [t s - (k - s), t s + s)
        const int cin = e.ch[j], cout = e.ch[j + 1], k = e.down_k[j], sd = e.down_s[j];
        float* out = j < 2 ? w.u[j + 1] + (size_t)w.P[j + 1] * cout : w.u3 + (size_t)w.P3 * cout;
        GemmArgs g = conv_gemm(m, w.uo[j] + (size_t)(w.P[j] - (k - sd)) * cin, (int64_t)sd * cin, e.down[j], out, cout, (int)w.L[j + 1]);
        if (cin % 64 == 0 && e.down[j].in == k * cin) { g.win_taps = k; g.win_c = cin; }
        launch_gemm(g, s);
        if (st) stage_out(st[2 + 2 * j], j < 2 ? w.u[j + 1] : w.u3, j < 2 ? w.P[j + 1] : w.P3, w.L[j + 1], cout, s);
    }
    // ELU -> tail conv 8f -> mimi_dim, stride 1: the transformer's input rows
    const int64_t T = w.L[3];
    float* x = w.x + (size_t)w.Px * C;
    {
        GemmArgs g = conv_gemm(m, w.u3 + (size_t)(w.P3 - (e.tail_k - 1)) * e.ch[3], e.ch[3], e.tail, x, C, (int)T);
        g.aop = AOP_ELU;
        if (e.ch[3] % 64 == 0 && e.tail.in == e.tail_k * e.ch[3] && e.tail_k >= 2) { g.win_taps = e.tail_k; g.win_c = e.ch[3]; }
        launch_gemm(g, s);
    }
    if (st) stage_out(st[7], w.x, w.Px, T, C, s);
    // transformer: the decoder transformer's layer (mimi.go:245-441) at the encoder's rate, positions from 0, window mimi_ctx
    const RowMap xm = RowMap{C, T, T * C};
    const RowMap qm = RowMap{3 * C, T, T * 3 * C};
    for (int l = 0; l < e.layers; l++) {
        const auto& L = e.ml[l];
        mimi_layer_qkv(m, L, x, xm, (int)T, w.qkv, qm, 0, (int)T, w.n1, s);
        launch_attention(attn_dense_args(w.qkv, 3 * C, C, 1, (int)T, 0, (int)T, d.mimi_heads, d.mimi_hd, d.mimi_ctx, w.attn, C), s);   // one segment, one chunk
        GemmArgs go = conv_gemm(m, w.attn, C, L.out_proj, x, C, (int)T);
        go.amap = flat(C); go.cmap = xm;
        go.R = x; go.epi = L.ls1 != NONE ? EPI_SCALE_RESADD : EPI_RESADD; go.scale = m.at<float>(L.ls1);
        launch_gemm(go, s);
        mimi_layer_ffn(m, L, x, xm, (int)T, w.n1, w.ff, s);
    }
    if (st) stage_out(st[8], w.x, w.Px, T, C, s);
    // downsample to the frame rate: stride ds_s, kernel ds_k over the transformer's rows, split-K (encoder.hip)
    launch_enc_downsample(w.x + (size_t)(w.Px - (e.ds_k - e.ds_s)) * C, (int64_t)e.ds_s * C, m.arena + e.ds.w, e.ds.bf16, m.at<float>(e.ds.b), (int)frames, C,
                          e.ds.in, w.partial, lat_dev, s);
    if (st && st[9]) PTTS_HIP(hipMemcpyAsync(st[9], lat_dev, (size_t)frames * C * sizeof(float), hipMemcpyDeviceToHost, s));
    return frames;
}

void mimi_encode(Model& m, const float* const* pcm, const int64_t* n_samples, int n_clips, float* const* latent_out, float* const* stages, const int32_t* rates) {
    const Desc& d = m.d;
    require_encoder(d);
    if (n_clips <= 0 || !pcm || !n_samples || !latent_out) throw Error(PTTS_EINVAL, "voice encode: no clips");
    if (stages && n_clips != 1) throw Error(PTTS_EINVAL, "ptts-hip: stage observation takes one clip");
    int64_t longest = 0;
    for (int i = 0; i < n_clips; i++) {
        if (!pcm[i] || n_samples[i] <= 0) throw Error(PTTS_EINVAL, strfmt("voice encode: audio of clip %d is empty", i));
        if (!latent_out[i]) throw Error(PTTS_EINVAL, strfmt("voice encode: no output buffer for clip %d", i));
        const int rate = rates ? rates[i] : kNativeRate;
        longest = std::max(longest, rate == kNativeRate ? (n_samples[i] + d.enc.hop - 1) / d.enc.hop : clip_frames(d, n_samples[i], rate));
    }
    if (longest > mimi_encode_max_frames(d))
        throw Error(PTTS_EINVAL, strfmt("voice encode: a clip of %lld frames exceeds the %lld frames one clip may have", (long long)longest,
                                        (long long)mimi_encode_max_frames(d)));
    // the workspace once, for the longest clip (layouts grow with the frame count)
    m.work(WORK_ENCODER, enc_layout(d, longest, nullptr).floats * sizeof(float));
    DevBuf& lat = m.work(WORK_ENCODER_LATENTS, (size_t)longest * d.mimi_dim * sizeof(float));
    for (int i = 0; i < n_clips; i++) {
        const int64_t f = mimi_encode_clip(m, pcm[i], n_samples[i], lat.as<float>(), stages, rates ? rates[i] : kNativeRate);
        PTTS_HIP(hipMemcpyAsync(latent_out[i], lat.p, (size_t)f * d.mimi_dim * sizeof(float), hipMemcpyDeviceToHost, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
    }
}

}  // namespace ptts
