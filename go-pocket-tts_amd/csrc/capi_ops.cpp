// capi_ops.cpp -- extern "C": the kernel-level entry points (ptts_op_*): one launch each on host operands, device 0, default stream, synchronous copies
// (capi_internal.h Tmp / up / down).
#include "capi_internal.h"

using namespace ptts;
using namespace ptts::capi;

// The shape ptts_op_conv1d_leftpad and the dense ptts_op_convtr1d_righttrim share: channels-first x [b][cin][len] to channels-last rows behind `pad`
// zero rows per batch, one product of every window (row t: K floats from input row t on) with wg [N][K] (+ bias [N], host, or null), and the
// [b][lout][cout] rows (N = (lout / len) * cout) back to channels-first y
static void windows_gemm(const float* x, int64_t b, int64_t cin, int64_t len, int64_t pad, const std::vector<float>& wg, const float* bias, int64_t N, int64_t K,
                         int64_t cout, int64_t lout, float* y) {
    Tmp dx((size_t)b * cin * len * 4), dxc((size_t)b * (pad + len) * cin * 4), dw(wg.size() * 4), db((size_t)N * 4), dyc((size_t)b * len * N * 4),
        dy((size_t)b * cout * lout * 4);
    up(dx.p, x, (size_t)b * cin * len * 4); up(dw.p, wg.data(), wg.size() * 4);
    if (bias) up(db.p, bias, (size_t)N * 4);
    PTTS_HIP(hipMemset(dxc.p, 0, (size_t)b * (pad + len) * cin * 4));
    launch_bct_to_btc(dx.as<float>(), (int)b, (int)cin, (int)len, dxc.as<float>(), (int)pad, nullptr);
    GemmArgs g;
    g.A = dxc.as<float>(); g.amap = RowMap{cin, len, (pad + len) * cin};
    g.W = dw.p; g.ldw = K; g.bias = bias ? db.as<float>() : nullptr;
    g.C = dyc.as<float>(); g.cmap = RowMap{N, 0, 0};
    g.M = (int)(b * len); g.N = (int)N; g.K = (int)K;
    launch_gemm(g, nullptr);
    launch_btc_to_bct(dyc.as<float>(), 0, (int)b, (int)cout, (int)lout, dy.as<float>(), nullptr);
    PTTS_HIP(hipDeviceSynchronize());
    down(y, dy.p, (size_t)b * cout * lout * 4);
}

extern "C" {

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
        std::vector<float> wg((size_t)cout * cin * k);  // [oc][kx*Cin + ic]  (same repack as model.cpp conv_as_gemm)
        for (int64_t o = 0; o < cout; o++) for (int64_t c = 0; c < cin; c++) for (int64_t xk = 0; xk < k; xk++) wg[(size_t)(o * cin * k + xk * cin + c)] = w[(o * cin + c) * k + xk];
        windows_gemm(x, b, cin, len, k - 1, wg, bias, cout, cin * k, cout, len, y);
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
            windows_gemm(x, b, cin, len, 1, wg, bg.data(), stride * cout, 2 * cin, cout, lout, y);
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