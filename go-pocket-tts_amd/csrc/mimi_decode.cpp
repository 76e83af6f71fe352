// mimi_decode.cpp -- engine: the Mimi decoder, Model.LatentToMimi + MimiModel.DecodeFromLatent (model.go:141-319, mimi.go:719-789)
//
// Every op of the decoder is causal (mimi.go:69-76,116-125,418), and every intermediate lives in a per-utterance
// channels-last buffer that spans the whole utterance.  Decoding frames [f0, f1) is therefore just the same launches on
// a row sub-range of each buffer: history rows (conv taps, the transposed convs' x[t-1], the 250-step attention window)
// are read from what earlier ranges left behind.  generate() uses this to decode finished frames on a second stream
// while the (latency-bound) AR loop is still producing later ones.
#include "launch_args.h"

#include <algorithm>

namespace ptts {

void mimi_setup(Model& m, MimiWs& w, int B, int T) {
    const Desc& d = m.d;
    w.B = B; w.T = T;
    const int C = d.mimi_dim, S = d.up_stride, T1 = T * S, F = d.mimi_ffn;
    w.P0 = d.init_k - 1;
    w.Ls[0] = T1; w.Ps[0] = 1;
    for (int j = 0; j < 3; j++) {
        w.Ls[j + 1] = w.Ls[j] * d.strides[j];
        int need_next = j < 2 ? 1 : d.final_k - 1;
        w.Ps[j + 1] = std::max(d.rb_k1[j] - 1, need_next);
    }
    size_t n_xp = (size_t)B * (1 + T) * C, n_up = (size_t)B * (w.P0 + T1) * C;
    size_t n_n1 = (size_t)B * T1 * C, n_qkv = (size_t)B * T1 * 3 * C, n_ff = (size_t)B * T1 * F;
    size_t n_c[4], n_h[3];
    for (int j = 0; j < 4; j++) n_c[j] = (size_t)B * (w.Ps[j] + w.Ls[j]) * d.sea_ch[j];
    for (int j = 0; j < 3; j++) n_h[j] = (size_t)B * ((d.rb_k2[j] - 1) + w.Ls[j + 1]) * d.sea_hidden[j];
    size_t total = n_xp + n_up + n_n1 + n_qkv * d.mimi_layers + n_n1 + n_ff + n_c[0] + 2 * (n_c[1] + n_c[2] + n_c[3]) + n_h[0] + n_h[1] + n_h[2];
    DevBuf& wsb = m.work(WORK_DECODER, total * sizeof(float));
    float* p = wsb.as<float>();
    w.xp = p; p += n_xp;
    w.up = p; p += n_up;
    w.n1 = p; p += n_n1;
    for (int l = 0; l < d.mimi_layers; l++) { w.qkv[l] = p; p += n_qkv; }
    w.attn = p; p += n_n1;
    w.ff = p; p += n_ff;
    w.c0 = p; p += n_c[0];
    for (int j = 0; j < 3; j++) { w.u[j] = p; p += n_c[j + 1]; w.uo[j] = p; p += n_c[j + 1]; w.h[j] = p; p += n_h[j]; }
    w.zeroed = false;
}

void mimi_zero_history(Model& m, MimiWs& w, hipStream_t s) {
    const Desc& d = m.d;
    const int C = d.mimi_dim, T1 = w.Ls[0];
    launch_zero_rows(w.xp, (int64_t)(1 + w.T) * C, w.B, C, s);
    launch_zero_rows(w.up, (int64_t)(w.P0 + T1) * C, w.B, (int64_t)w.P0 * C, s);
    launch_zero_rows(w.c0, (int64_t)(w.Ps[0] + w.Ls[0]) * d.sea_ch[0], w.B, (int64_t)w.Ps[0] * d.sea_ch[0], s);
    for (int j = 0; j < 3; j++) {
        const int cout = d.sea_ch[j + 1], hid = d.sea_hidden[j], Ph = d.rb_k2[j] - 1;
        launch_zero_rows(w.u[j], (int64_t)(w.Ps[j + 1] + w.Ls[j + 1]) * cout, w.B, (int64_t)w.Ps[j + 1] * cout, s);
        launch_zero_rows(w.uo[j], (int64_t)(w.Ps[j + 1] + w.Ls[j + 1]) * cout, w.B, (int64_t)w.Ps[j + 1] * cout, s);
        if (Ph > 0) launch_zero_rows(w.h[j], (int64_t)(Ph + w.Ls[j + 1]) * hid, w.B, (int64_t)Ph * hid, s);
    }
    w.zeroed = true;
}

// Two pieces of a decoder-transformer layer (mimi.go:245-441) as the decoder launches them; also reachable on their own through
// ptts_mimi_layer_piece (staged parity checks).
// norm1 -> in_proj (no bias) -> RoPE of q and k at positions pos0 + (row % rows_per_seg): x rows [R][C] -> qkv rows [R][3C].  n1: [R][C] scratch.
void mimi_layer_qkv(Model& m, int l, const float* x, RowMap xmap, int R, float* qkv, RowMap qmap, int pos0, int rows_per_seg, float* n1, hipStream_t s) {
    mimi_layer_qkv(m, m.d.ml[l], x, xmap, R, qkv, qmap, pos0, rows_per_seg, n1, s);
}
void mimi_layer_qkv(Model& m, const Desc::ML& L, const float* x, RowMap xmap, int R, float* qkv, RowMap qmap, int pos0, int rows_per_seg, float* n1, hipStream_t s) {
    const Desc& d = m.d;
    const int C = d.mimi_dim;
    if (L.qkv_img != NONE && d.mimi_hd == 64) {   // one kernel (ffn_fused.hip k_mimi_rowlin)
        RowLinArgs ra;
        ra.x = x; ra.xmap = xmap;
        ra.ln_w = m.at<float>(L.n1.w); ra.ln_b = m.at<float>(L.n1.b); ra.eps = L.n1.eps;
        ra.img = m.at<uint8_t>(L.qkv_img);
        ra.y = qkv; ra.ymap = qmap;
        ra.rope_cos = m.at<float>(d.rope_cos); ra.rope_sin = m.at<float>(d.rope_sin); ra.rope_cols = 2 * C; ra.rope_pos0 = pos0; ra.rope_rows_per_seg = rows_per_seg;
        ra.M = R; ra.N = 3 * C; ra.K = C;
        if (mimi_rowlin_supported(ra)) { launch_mimi_rowlin(ra, s); return; }
    }
    launch_layernorm(mkln(m, x, xmap, L.n1, n1, C, R), s);
    GemmArgs gq = mk(m, n1, flat(C), L.in_proj, qkv, qmap, R);
    gq.rope_cos = m.at<float>(d.rope_cos); gq.rope_sin = m.at<float>(d.rope_sin);   // q and k are rotated in the epilogue
    gq.rope_cols = 2 * C; gq.rope_hd = d.mimi_hd; gq.rope_pos0 = pos0; gq.rope_rows_per_seg = rows_per_seg;
    if (!launch_gemm_rope(gq, s)) {
        gq.rope_cos = gq.rope_sin = nullptr;
        launch_gemm(gq, s);
        launch_rope_rows(qkv, qmap, 0, d.mimi_heads, d.mimi_hd, nullptr, pos0, rows_per_seg, R, m.at<float>(d.rope_cos), m.at<float>(d.rope_sin), s);
        launch_rope_rows(qkv, qmap, C, d.mimi_heads, d.mimi_hd, nullptr, pos0, rows_per_seg, R, m.at<float>(d.rope_cos), m.at<float>(d.rope_sin), s);
    }
}

// x += layer_scale_2 * linear2(gelu(linear1(norm2(x)))) on rows [R][C], in place.  n1: [R][C], ffb: [R][F] scratch (unused by the fused kernel).
void mimi_layer_ffn(Model& m, int l, float* x, RowMap xmap, int R, float* n1, float* ffb, hipStream_t s) {
    mimi_layer_ffn(m, m.d.ml[l], x, xmap, R, n1, ffb, s);
}
void mimi_layer_ffn(Model& m, const Desc::ML& L, float* x, RowMap xmap, int R, float* n1, float* ffb, hipStream_t s) {
    const Desc& d = m.d;
    const int C = d.mimi_dim, F = d.mimi_ffn;
    if (L.ffn_img != NONE) {   // one kernel (ffn_fused.hip k_mimi_ffn)
        FfnArgs fa;
        fa.x = x; fa.xmap = xmap;
        fa.ln_w = m.at<float>(L.n2.w); fa.ln_b = m.at<float>(L.n2.b); fa.eps = L.n2.eps;
        fa.img = m.at<uint8_t>(L.ffn_img);
        fa.ls = m.at<float>(L.ls2);
        fa.M = R; fa.D = C; fa.F = F;
        if (mimi_ffn_supported(fa)) { launch_mimi_ffn(fa, s); return; }
    }
    launch_layernorm(mkln(m, x, xmap, L.n2, n1, C, R), s);
    GemmArgs g1 = mk(m, n1, flat(C), L.l1, ffb, flat(F), R);
    g1.epi = EPI_GELU;
    launch_gemm(g1, s);
    GemmArgs g2 = mk(m, ffb, flat(F), L.l2, x, xmap, R);
    g2.R = x; g2.epi = L.ls2 != NONE ? EPI_SCALE_RESADD : EPI_RESADD; g2.scale = m.at<float>(L.ls2);
    launch_gemm(g2, s);
}

// frames [f0, f1) of every utterance; lat: device [B][*][ldim] with lat_bstride elements between utterances;
// pcm: device [B][T * samples_per_frame]; mimi_latent (optional): [B][C][T] (whole range only)
void mimi_range(Model& m, MimiWs& w, const float* lat, int64_t lat_bstride, int f0, int f1, float* pcm, float* mimi_latent, hipStream_t s,
                const PcmRow* pcm_rows, bool* rows_used, float* xformer_out) {
    if (rows_used) *rows_used = false;
    const Desc& d = m.d;
    const int B = w.B, T = w.T, C = d.mimi_dim, S = d.up_stride, T1 = T * S, P0 = w.P0;
    if (f1 <= f0) return;
    if (!w.zeroed) mimi_zero_history(m, w, s);
    const int nf = f1 - f0;
    // K13: latent -> mimi projection rows 1+f0 .. 1+f1 of xp
    launch_projector(lat, lat_bstride, m.at<float>(d.proj_w), m.at<float>(d.proj_b), B, T, f0, f1, d.ldim, C, w.xp, s);
    if (mimi_latent) launch_btc_to_bct(w.xp, 1, B, C, T, mimi_latent, s);
    // K14: depthwise upsample -> rows [f0*S, f1*S) of up
    launch_upsample_depthwise(w.xp, m.at<float>(d.up_w0), m.at<float>(d.up_w1), nullptr, B, T, f0, f1, C, S, w.up, P0, s);
    // decoder transformer (mimi.go:245-441, 506-525): positions restart at 0 for every utterance, window `context`
    const int t0 = f0 * S, CT = nf * S, R = B * CT;
    const int64_t up_bs = (int64_t)(P0 + T1) * C;
    float* upx = w.up + (size_t)(P0 + t0) * C;            // chunk rows of the residual stream
    const RowMap upm = seg(C, CT, up_bs);
    float* n1 = w.n1;                                       // [R][C] scratch (chunk-local)
    float* attn = w.attn;
    float* ffb = w.ff;
    for (int l = 0; l < d.mimi_layers; l++) {
        const auto& L = d.ml[l];
        float* qkv = w.qkv[l];                              // [B][T1][3C], persists across ranges (keys/values of earlier frames)
        float* qkvx = qkv + (size_t)t0 * 3 * C;
        const RowMap qm = seg(3 * C, CT, (int64_t)T1 * 3 * C);
        mimi_layer_qkv(m, l, upx, upm, R, qkvx, qm, t0, CT, n1, s);
        launch_attention(attn_dense_args(qkv, 3 * C, C, B, T1, t0, CT, d.mimi_heads, d.mimi_hd, d.mimi_ctx, attn, C), s);
        GemmArgs go = mk(m, attn, flat(C), L.out_proj, upx, upm, R);
        go.R = upx; go.epi = L.ls1 != NONE ? EPI_SCALE_RESADD : EPI_RESADD; go.scale = m.at<float>(L.ls1);
        launch_gemm(go, s);
        mimi_layer_ffn(m, l, upx, upm, R, n1, ffb, s);
    }
    if (xformer_out)   // staged parity check: the residual stream after the last layer, [B][T1][C] (rows of this range)
        PTTS_HIP(hipMemcpy2DAsync(xformer_out + (size_t)t0 * C, (size_t)T1 * C * sizeof(float), upx, (size_t)up_bs * sizeof(float), (size_t)CT * C * sizeof(float),
                                  (size_t)B, hipMemcpyDeviceToDevice, s));
    // SEANet decoder (mimi.go:740-788): causal convs as GEMMs over contiguous channels-last windows
    int r0 = t0, rn = CT;   // row range at the current rate
    {
        const int ch = d.sea_ch[0];
        GemmArgs g = mk(m, w.up + (size_t)r0 * C, seg(C, rn, up_bs), d.init_conv, w.c0 + (size_t)(w.Ps[0] + r0) * ch,
                        seg(ch, rn, (int64_t)(w.Ps[0] + w.Ls[0]) * ch), B * rn);
        g.epi = EPI_ELU;  // x = elu(initConv(x))
        if (C % 64 == 0 && d.init_conv.in == d.init_k * C) { g.win_taps = d.init_k; g.win_c = C; }   // (k walked channel-block-major: gemm5.hip)
        launch_gemm(g, s);
    }
    bool final_done = false;
    for (int j = 0; j < 3; j++) {
        const int cin = d.sea_ch[j], cout = d.sea_ch[j + 1], st = d.strides[j], hid = d.sea_hidden[j];
        const int Lin_ = w.Ls[j], Lout = w.Ls[j + 1], Pin = w.Ps[j], Pout = w.Ps[j + 1], Ph = d.rb_k2[j] - 1;
        const float* in = j == 0 ? w.c0 : w.uo[j - 1];
        float* u = w.u[j];
        float* uo = w.uo[j];
        float* hb = w.h[j];
        const int64_t in_bs = (int64_t)(Pin + Lin_) * cin, u_bs = (int64_t)(Pout + Lout) * cout, h_bs = (int64_t)(Ph + Lout) * hid;
        // transposed conv: window [x[t-1], x[t]] starts one row before t
        GemmArgs gu = mk(m, in + (size_t)(Pin - 1 + r0) * cin, seg(cin, rn, in_bs), d.up[j],
                         u + (size_t)(Pout + (int64_t)r0 * st) * cout, seg((int64_t)st * cout, rn, u_bs), B * rn);
        // elu(x) precedes every transposed conv: c0 was activated in the initConv epilogue, uo[j-1] in its residual epilogue
        if (j == 2 && d.rb1[j].wf != NONE && d.rb2[j].wf != NONE && d.rb1[j].bf16 && d.rb2[j].bf16 && d.up[j].wf != NONE) {
            // the last stage as ONE kernel: transposed convolution + residual block + final convolution (resblock_up.hip); u[2] is never written
            ResArgs rr;
            rr.u = u; rr.u_bs = u_bs; rr.pad = Pout; rr.uo = uo;
            rr.w1 = m.at<uint8_t>(d.rb1[j].wf); rr.b1 = m.at<float>(d.rb1[j].b);
            rr.w2 = m.at<uint8_t>(d.rb2[j].wf); rr.b2 = m.at<float>(d.rb2[j].b);
            rr.B = B; rr.L = Lout; rr.t0 = r0 * st; rr.t1 = (r0 + rn) * st;
            rr.C = cout; rr.H = hid; rr.k1 = d.rb_k1[j]; rr.k2 = d.rb_k2[j]; rr.w_bf16 = 1;
            rr.final_conv = 1; rr.kf = d.final_k; rr.wf_hi = m.at<uint8_t>(d.final_wf); rr.wf_lo = m.at<uint8_t>(d.final_wf_lo); rr.bf = m.at<float>(d.final_b);
            rr.pcm = pcm; rr.pcm_bs = w.Ls[3]; rr.pcm_rows = pcm_rows;
            rr.fuse_up = 1; rr.xin = in; rr.x_bs = in_bs; rr.x_pad = Pin; rr.x_L = Lin_; rr.CI = cin; rr.up_stride = st;
            rr.wup = m.at<uint8_t>(d.up[j].wf); rr.bup = m.at<float>(d.up[j].b);
            if (resblock_up_supported(rr)) {
                launch_resblock_up(rr, s);
                if (rows_used && pcm_rows) *rows_used = true;
                final_done = true;
                r0 *= st; rn *= st;
                continue;
            }
        }
        launch_gemm(gu, s);
        r0 *= st; rn *= st;
        // residual block: x + conv_k1(elu(conv_k3(elu(x))))  (mimi.go:146-164); x stays in u, elu(sum) goes to uo -- the
        // only readers of the sum are the next transposed conv and the final conv, both behind an ELU (mimi.go:752-783).
        // The two narrow blocks run as one launch each (resblock.hip); the last one also applies the final conv.
        {
            ResArgs ra;
            ra.u = u; ra.u_bs = u_bs; ra.pad = Pout; ra.uo = uo;
            ra.w1 = m.at<uint8_t>(d.rb1[j].wf); ra.w1_lo = m.at<uint8_t>(d.rb1[j].wf_lo); ra.b1 = m.at<float>(d.rb1[j].b);
            ra.w2 = m.at<uint8_t>(d.rb2[j].wf); ra.w2_lo = m.at<uint8_t>(d.rb2[j].wf_lo); ra.b2 = m.at<float>(d.rb2[j].b);
            ra.B = B; ra.L = Lout; ra.t0 = r0; ra.t1 = r0 + rn;
            ra.C = cout; ra.H = hid; ra.k1 = d.rb_k1[j]; ra.k2 = d.rb_k2[j]; ra.w_bf16 = d.rb1[j].bf16;
            if (j == 2) {
                ra.final_conv = 1; ra.kf = d.final_k; ra.wf_hi = m.at<uint8_t>(d.final_wf); ra.wf_lo = m.at<uint8_t>(d.final_wf_lo); ra.bf = m.at<float>(d.final_b);
                ra.pcm = pcm; ra.pcm_bs = w.Ls[3];
            }
            if (j == 2 && pcm_rows && d.rb1[j].wf != NONE && d.rb2[j].wf != NONE && d.rb1[j].bf16 == d.rb2[j].bf16) {
                ResArgs rr = ra;
                rr.pcm_rows = pcm_rows;
                if (resblock_supported(rr)) {
                    launch_resblock(rr, s);
                    if (rows_used) *rows_used = true;
                    final_done = true;
                    continue;
                }
            }
            if (d.rb1[j].wf != NONE && d.rb2[j].wf != NONE && d.rb1[j].bf16 == d.rb2[j].bf16 && resblock_supported(ra)) {
                launch_resblock(ra, s);
                if (j == 2) final_done = true;
                continue;
            }
        }
        GemmArgs g1 = mk(m, u + (size_t)(Pout - (d.rb_k1[j] - 1) + r0) * cout, seg(cout, rn, u_bs), d.rb1[j],
                         hb + (size_t)(Ph + r0) * hid, seg(hid, rn, h_bs), B * rn);
        g1.aop = AOP_ELU; g1.epi = EPI_ELU;
        if (cout % 64 == 0 && d.rb1[j].in == d.rb_k1[j] * cout) { g1.win_taps = d.rb_k1[j]; g1.win_c = cout; }
        launch_gemm(g1, s);
        GemmArgs g2 = mk(m, hb + (size_t)r0 * hid, seg(hid, rn, h_bs), d.rb2[j], uo + (size_t)(Pout + r0) * cout, seg(cout, rn, u_bs), B * rn);
        g2.R = u + (size_t)(Pout + r0) * cout; g2.epi = EPI_RESADD_ELU;
        launch_gemm(g2, s);
    }
    if (!final_done)
    launch_conv_final(w.uo[2], w.Ps[3], m.at<float>(d.final_w), m.at<float>(d.final_b), B, w.Ls[3], r0, r0 + rn, d.sea_ch[3], d.final_k, 0, pcm, s);
}

void mimi_decode(Model& m, const float* lat, int64_t lat_bstride, int B, int T, float* pcm, float* mimi_latent, float* xformer_out) {
    if (B <= 0 || T <= 0) return;
    if ((int64_t)T * m.d.up_stride > ROPE_SEQ) throw Error(PTTS_EINVAL, strfmt("ops: rope cos/sin sequence length too small for pos=0 seq=%lld", (long long)T * m.d.up_stride));
    // bound the workspace: ~2.7 MB of f32 activations per latent frame at the reference shapes
    const Desc& d = m.d;
    double per_frame = 4.0 * ((double)d.up_stride * (d.mimi_dim * (4.0 + 3.0 * d.mimi_layers) + d.mimi_ffn) +
                              (double)d.samples_per_frame * (d.sea_ch[3] * 2.6 + d.sea_ch[2] * 0.7 + d.sea_ch[1] * 0.25));
    int group = (int)std::max(1.0, std::min((double)B, 40e9 / (per_frame * T)));
    const int64_t spu = (int64_t)T * d.samples_per_frame;
    for (int b0 = 0; b0 < B; b0 += group) {
        int nb = std::min(group, B - b0);
        MimiWs w;
        mimi_setup(m, w, nb, T);
        mimi_range(m, w, lat + (int64_t)b0 * lat_bstride, lat_bstride, 0, T, pcm + (int64_t)b0 * spu,
                   mimi_latent ? mimi_latent + (int64_t)b0 * d.mimi_dim * T : nullptr, m.stream, nullptr, nullptr,
                   xformer_out ? xformer_out + (int64_t)b0 * T * d.up_stride * d.mimi_dim : nullptr);
    }
}

}  // namespace ptts
