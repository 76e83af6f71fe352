// step.cpp -- engine: one AR step on device state (the step linears, the flow part, the flow-net cluster's recovery) and its graphs.
#include "launch_args.h"

#include <algorithm>

namespace ptts {

// every linear of the AR step goes through here so that bench.py can time the dominant kernel with HIP events
static void step_gemm(Model& m, const GemmArgs& g, const SkinnyFuse& fu = SkinnyFuse{}, int splitk = 1, float* partial = nullptr, hipStream_t st = nullptr) {
    if (!st) st = m.stream;
    const bool fused = fu.pend.partial || fu.ln;
    const bool sk = fused ? skinny_fuse_supported(g, fu) : skinny_supported(g, splitk);
    if (!sk && (splitk > 1 || fused)) throw Error(PTTS_EINVAL, "ptts-hip: internal: shape not supported by the step kernel");
    Prof& p = m.prof;
    if (p.on) {
        while (p.ev.size() < p.used + 2) { hipEvent_t e; PTTS_HIP(hipEventCreate(&e)); p.ev.push_back(e); }
        if (sk) { g_skinny_ev[0] = p.ev[p.used]; g_skinny_ev[1] = p.ev[p.used + 1]; }   // the dispatch stamps itself
        else PTTS_HIP(hipEventRecord(p.ev[p.used], st));
    }
    if (sk) launch_skinny(g, fu, splitk, partial, st);
    else launch_gemm(g, st);
    g_skinny_ev[0] = g_skinny_ev[1] = nullptr;
    if (p.on) {
        if (!sk) PTTS_HIP(hipEventRecord(p.ev[p.used + 1], st));
        p.used += 2;
        p.launches++;
        const int wbytes = (sk && g.wt_i8) ? 1 : (g.w_bf16 ? 2 : 4);
        p.bytes += (double)g.N * g.K * wbytes + (double)g.M * g.K * 4 * (1 + fu.pend.splitk) + (double)g.M * g.N * 4 * (splitk > 1 ? splitk : 1);
        p.wbytes += (double)g.N * g.K * wbytes;
    }
}

int pick_split(int M, int N, int K, bool w_bf16) {
    if (K <= 1024) return 1;   // a whole-K block is one memory burst; splitting pays only when K forces several bursts
    // a full batch on bf16 weights: 2048-deep slices (k_skinny NJ = 8, 32-column blocks): the producer's blocks fetch a third more,
    // every consumer block of the next launch re-reads half as many planes
    if (w_bf16 && M > 32 && K >= 4096 && K % 2048 == 0 && ((N + 31) / 32) * ((M + 15) / 16) * (K / 2048) >= 200) return K / 2048;
    int need = (K + 1023) / 1024;
    int blocks = ((N + 63) / 64) * ((M + 15) / 16);
    int want = (256 + blocks - 1) / blocks;
    int S = std::max(need, std::min(want, K / 512));
    // the slices are whole 128-deep super-steps: at widths that are no multiple of 512 the rounding can leave the last of many slices empty (K = 3080 over 6:
    // 5 x 640 >= K), which the step kernel does not take (skinny_supported).  `need` slices of at most 1024 never do: (need - 1) * 1024 < K
    while (S > need && (S - 1) * (((K + S - 1) / S + 127) / 128 * 128) >= K) S--;
    return S;
}

// one transformer-style block input: rows of x (with a pending residual update) -> LayerNorm -> linear
struct FusedIn {
    PendingSum pend;          // deferred "x += sum of split-K planes + bias": executed by this launch's prologue
    float* x_out = nullptr;   // where the updated residual goes when pend is set
    const Norm* norm = nullptr; bool affine = true; float eps = 1e-5f;
    const float* shift = nullptr; const float* scale = nullptr; int64_t ldmod = 0;
    float* y_out = nullptr;
    const StepFinish* finish = nullptr;   // the step's last launch: bookkeeping in the epilogue (SkinnyFuse::fin)
    bool chain = false; const float* chain_noise = nullptr; int64_t chain_noise_stride = 0;   // ... and the next step's opening (SkinnyFuse::chain)
};

// the step kernel's prologue for `in`, with its finish and without its chain (step_fused_linear tries that first)
static SkinnyFuse fused_prologue(const Model& m, const FusedIn& in) {
    SkinnyFuse fu;
    fu.pend = in.pend;
    fu.x_out = in.x_out;
    fu.ln = 1; fu.eps = in.eps;
    if (in.norm && in.affine) { fu.ln_w = m.at<float>(in.norm->w); fu.ln_b = m.at<float>(in.norm->b); }
    fu.shift = in.shift; fu.scale = in.scale; fu.ldmod = in.ldmod;
    fu.y_out = in.y_out;
    fu.fin = in.finish;
    return fu;
}

// returns whether in.finish was honoured (false: the caller launches k_step_finish itself)
static bool step_fused_linear(Batch& b, const float* x, const FusedIn& in, const Lin& l, float* C, int64_t ldc, int M, int epi,
                              const float* addvec, const float* R, float alpha, hipStream_t st = nullptr, bool* chained = nullptr) {
    Model& m = *b.m;
    GemmArgs g = mk(m, x, flat(l.in), l, C, flat(ldc), M);
    g.epi = epi; g.addvec = addvec; g.R = R; g.alpha = alpha;
    SkinnyFuse fu = fused_prologue(m, in);
    if (in.finish && in.chain) {
        fu.chain = 1; fu.chain_noise = in.chain_noise; fu.chain_noise_stride = in.chain_noise_stride;
        if (skinny_fuse_supported(g, fu)) { step_gemm(m, g, fu, 1, nullptr, st); if (chained) *chained = true; return true; }
        fu.chain = 0; fu.chain_noise = nullptr;
    }
    if (skinny_fuse_supported(g, fu)) { step_gemm(m, g, fu, 1, nullptr, st); return fu.fin != nullptr; }
    fu.fin = nullptr;
    if (skinny_fuse_supported(g, fu)) { step_gemm(m, g, fu, 1, nullptr, st); return false; }
    if (st && st != m.stream) throw Error(PTTS_EINVAL, "ptts-hip: internal: unfused step linear on a side stream");
    // shapes outside the fused kernel (never the reference checkpoint): separate LayerNorm launch, then the linear
    LnArgs ln;
    ln.x = x; ln.xmap = flat(l.in); ln.eps = in.eps; ln.rows = M; ln.d = l.in;
    if (in.norm && in.affine) { ln.w = m.at<float>(in.norm->w); ln.b = m.at<float>(in.norm->b); }
    ln.shift = in.shift; ln.scale = in.scale; ln.ldmod = in.ldmod;
    ln.pend = in.pend;
    float* y = in.y_out ? in.y_out : b.xn.as<float>();
    ln.y = y; ln.ldy = l.in;
    if (in.pend.partial) {   // the unfused reducer updates x in place; mirror it into x_out for the caller's ping-pong
        launch_layernorm(ln, m.stream);
        if (in.x_out && in.x_out != x) PTTS_HIP(hipMemcpyAsync(in.x_out, x, (size_t)M * l.in * sizeof(float), hipMemcpyDeviceToDevice, m.stream));
    } else launch_layernorm(ln, m.stream);
    g.A = y;
    step_gemm(m, g);
    return false;
}

bool open_linears(Batch& b, StepOpenLinears& lin) {
    Model& m = *b.m;
    const Desc& d = m.d;
    const int ld = d.ldim;
    if (!(ld <= 64 && ld % 4 == 0 && d.input_linear.in == ld && d.input_proj.in == ld && d.input_linear.bf16 == d.input_proj.bf16)) return false;
    lin.w_in = m.arena + d.input_linear.w; lin.b_in = m.at<float>(d.input_linear.b); lin.d_in = d.input_linear.out; lin.x = b.x.as<float>();
    lin.w_pj = m.arena + d.input_proj.w; lin.b_pj = m.at<float>(d.input_proj.b); lin.d_pj = d.input_proj.out; lin.fx = b.fx.as<float>();
    lin.w_bf16 = d.input_linear.bf16;
    return true;
}

// a hand-off inside k_flow_cluster gave up (flow_cluster.hip: bounded sweeps -- a tile's eight workgroups were not all running: another tenant on the CUs, a
// masked queue): the frames computed since are not to be trusted.  The exchange state is cleared, the batch -- and whatever batch this engine builds
// later -- goes back to the 2 x depth launches, which compute the same bits, and the event is counted (ptts_dispatch_stats.flow_cluster_fallbacks).
void flow_cluster_recover(Batch& b) {
    hipStream_t s = b.m->stream;
    (void)hipStreamSynchronize(s);
    (void)hipMemsetAsync(b.fc_xbuf.p, 0, flow_cluster_xbuf_bytes(b.B), s);
    (void)hipMemsetAsync(b.fc_sync.p, 0, kFlowClusterSyncBytes, s);
    (void)hipStreamSynchronize(s);
    b.fc_ok = false;
    // (the captured step graphs hold the cluster launch: drop them, the next replay captures the launches)
    b.drop_graphs();
    b.opened = false;
    b.m->fc_disabled.store(true);
    b.m->fc_fallbacks.fetch_add(1);
}
void flow_cluster_fault(Batch& b) {
    flow_cluster_recover(b);
    throw FlowClusterFault(PTTS_ENODEVICE, "ptts-hip: the flow net's in-launch hand-off timed out (k_flow_cluster); the steps concerned are re-issued as launches");
}

void step_open(Batch& b) {
    Model& m = *b.m;
    const Desc& d = m.d;
    const int ld = d.ldim;
    const int64_t ls = (int64_t)b.max_steps * ld;
    StepOpenLinears lin;
    const bool ok = open_linears(b, lin);
    b.opened = ok;
    b.par = 0;   // k_step_begin writes the first pair (fx, cur)
    launch_step_begin(b.st, b.latents.as<float>(), ls, m.at<float>(d.bos), b.has_noise ? b.noise.as<float>() : nullptr, ls, ld, b.B,
                      b.in32.as<float>(), b.cur.as<float>(), ok ? &lin : nullptr, m.stream);
}

// LSDDecode (flow_lm.go:311-353) with flowNet.Forward (flow_net.go:314-356) per Euler step: the flow part of a step, from `last` (out_norm's rows), `sy`
// (when the transformer's last launch produced it: Batch::tail_fused) and `cur` (x0 -> the frame)
static bool step_flow(Batch& b, int lsd, bool opened, bool fuse_finish, bool chain) {
    bool finished = false;
    Model& m = *b.m;
    const Desc& d = m.d;
    const int B = b.B, D = d.d_model, C = d.flow_dim, NA = d.ada_all.out;
    hipStream_t s = m.stream;
    const bool tail_fused = b.tail_fused;
    float* last = b.last.as<float>();
    float* sy = b.sy.as<float>();
    const float* tc = m.tcomb.at(lsd)->as<float>();
    float* ada = b.ada.as<float>();
    float* fx = b.fx_now();
    float* fh2 = b.fh2.as<float>();
    float* cur = b.cur_now();
    for (int i = 0; i < lsd; i++) {
        if (i > 0 || !tail_fused) {
            GemmArgs gc = mk(m, last, flat(D), d.cond_embed, sy, flat(C), B);  // sy = silu(0.5*(e_s+e_t) + cond_embed(c))
            gc.epi = EPI_SILU; gc.addvec = tc + (size_t)i * C;
            step_gemm(m, gc);
        }
        step_gemm(m, mk(m, sy, flat(C), d.ada_all, ada, flat(NA), B));
        if (i > 0 || !opened) step_gemm(m, mk(m, cur, flat(d.ldim), d.input_proj, fx, flat(C), B));
        bool clustered = false;
        if (b.fc_ok) {   // all residual blocks in one launch (flow_cluster.hip)
            FlowClusterArgs fa;
            fa.fx_in = fx; fa.fx_out = fx; fa.ada = ada; fa.ldmod = NA; fa.rows = B; fa.depth = d.flow_depth;
            for (int r = 0; r < d.flow_depth; r++) {
                const auto& rb = d.rb[r];
                fa.eps[r] = rb.ln.eps; fa.ln_w[r] = m.at<float>(rb.ln.w); fa.ln_b[r] = m.at<float>(rb.ln.b);
                fa.w0[r] = m.arena + rb.mlp0.wt; fa.b0[r] = m.at<float>(rb.mlp0.b);
                fa.w2[r] = m.arena + rb.mlp2.wt; fa.b2[r] = m.at<float>(rb.mlp2.b);
            }
            fa.xbuf = b.fc_xbuf.as<unsigned long long>(); fa.sync = b.fc_sync.as<unsigned>();
            if (b.fc_stamps.p) fa.stamps = b.fc_stamps.as<unsigned long long>();
            if (m.fc_inject && !b.capturing) { fa.inject = m.fc_inject; m.fc_inject = 0; }
            if (flow_cluster_supported(fa, C)) {
                // (not a launch of the step linear: the bench's per-launch events and byte counts -- Prof -- leave it out; bench.py reports it from the kernel trace)
                launch_flow_cluster(fa, s);
                clustered = true;
            }
        }
        for (int r = 0; !clustered && r < d.flow_depth; r++) {  // flowResBlock.Forward flow_net.go:116-172 (chunks: shift, scale, gate)
            const auto& rb = d.rb[r];
            FusedIn in;
            in.norm = &rb.ln; in.eps = rb.ln.eps;
            in.shift = ada + (size_t)r * 3 * C; in.scale = in.shift + C; in.ldmod = NA;
            step_fused_linear(b, fx, in, rb.mlp0, fh2, C, B, EPI_SILU, nullptr, nullptr, 1.0f);
            GemmArgs g2 = mk(m, fh2, flat(C), rb.mlp2, fx, flat(C), B);
            g2.R = fx; g2.epi = EPI_GATE_RESADD; g2.gate = ada + (size_t)r * 3 * C + 2 * C; g2.ldg = NA;
            step_gemm(m, g2);
        }
        FusedIn fin;  // flowFinalLayer.Forward flow_net.go:205-239: LayerNorm without affine, eps 1e-6, chunks: shift, scale
        fin.affine = false; fin.eps = 1e-6f;
        fin.shift = ada + (size_t)d.flow_depth * 3 * C; fin.scale = fin.shift + C; fin.ldmod = NA;
        if (fuse_finish && i == lsd - 1) {
            fin.finish = b.fin_dev.as<StepFinish>() + b.par;
            if (chain && b.chain_ok) {   // ... and the NEXT step's opening (k_step_begin's work without its launch)
                fin.chain = true;
                fin.chain_noise = b.has_noise ? b.noise.as<float>() : nullptr;
                fin.chain_noise_stride = (int64_t)b.max_steps * d.ldim;
            }
        }
        bool chained = false;
        finished = step_fused_linear(b, fx, fin, d.final_linear, cur, d.ldim, B, EPI_AXPY, nullptr, cur, 1.0f / (float)lsd, nullptr, &chained);  // current += flow / steps
        if (chained) { b.opened = true; b.par ^= 1; }
    }
    return finished;
}

// FlowLM.SampleNextLatentStateful minus the host glue (flow_lm.go:252-288): input_linear, 6 x forwardWithState(Tq=1),
// out_norm, out_eos, LSD decode through the flow net.  Everything reads device state, so the sequence is graph-capturable.
// Launch plan per transformer layer: [LN1 + in_proj] -> [RoPE + KV append + attention] -> [out_proj + residual]
// -> [LN2 + linear1 + GELU] -> [linear2, split over K]; the split-K sum and its residual add ride in the next
// layer's first launch.  The residual stream ping-pongs between two buffers so that no launch reads rows another
// block of the same launch rewrites.
bool step_core(Batch& b, int lsd, bool opened, bool fuse_finish, bool chain) {
    bool finished = false;
    b.opened = false;   // x / fx are consumed by this step; a chained last launch (below) sets it again for the next one
    if (!opened) b.par = 0;   // (the staged entry points and shapes k_step_begin does not take: the caller filled in32 / cur)
    Model& m = *b.m;
    const Desc& d = m.d;
    hipStream_t s = m.stream;
    const int B = b.B, D = d.d_model, C = d.flow_dim;
    float* x = b.x.as<float>();
    float* qkv = b.qkv.as<float>();
    float* attn = b.attn.as<float>();
    float* ff = b.ff.as<float>();
    if (!opened) step_gemm(m, mk(m, b.in32.as<float>(), flat(d.ldim), d.input_linear, x, flat(D), B));
    // A split linear2 leaves [x + (sums_0 + bias)] in plane 0 and the raw sums of the other K slices in planes 1..S-1 (k_skinny, slice 0
    // with GemmArgs::R set): the next consumer of the residual stream reads plane 0 as its rows and adds the others in order --
    // with S = 2 (a full batch on bf16 weights) two row images per block instead of three (residual, two planes) plus the bias.
    PendingSum pend;
    const float* xin = x;   // where the current residual rows are read from: x, or plane 0 while a split sum is pending
    float* const planes = b.partial.as<float>();
    // 128 rows and more (tall.hip): the prologue once per row (k_rowprep -> bf16 row planes), in_proj / linear1 / linear2 as 64 x 64-tile products (k_tall)
    const bool tall = b.tall_ok && B >= kTallMinRows;
    uint16_t* pa_h = tall ? b.tp_a.as<uint16_t>() : nullptr; uint16_t* pa_l = tall ? pa_h + (size_t)B * D : nullptr;
    uint16_t* pf_h = tall ? b.tp_f.as<uint16_t>() : nullptr; uint16_t* pf_l = tall ? pf_h + (size_t)B * d.ffn : nullptr;
    auto prep = [&](const float* rows, const PendingSum& pd, const Norm& nm, float* y_out = nullptr) {
        PrepArgs pa;
        pa.x = rows; pa.ldx = D; pa.pend = pd;
        pa.x_out = pd.partial ? x : nullptr;
        pa.ln_w = m.at<float>(nm.w); pa.ln_b = m.at<float>(nm.b); pa.eps = nm.eps;
        pa.yh = pa_h; pa.yl = pa_l; pa.ldy = D; pa.y_out = y_out; pa.M = B; pa.D = D;
        if (!rowprep_supported(pa)) throw Error(PTTS_EINVAL, "ptts-hip: internal: shape not supported by the row preparation kernel");
        launch_rowprep(pa, s);
    };
    auto tall_lin = [&](const uint16_t* ah, const uint16_t* al, const Lin& li, TallArgs t) {
        t.ah = ah; t.al = al; t.lda = li.in; t.Wt = m.arena + li.wt; t.bias = m.at<float>(li.b); t.M = B; t.N = li.out; t.K = li.in;
        if (!tall_supported(t)) throw Error(PTTS_EINVAL, "ptts-hip: internal: shape not supported by the 64-row step linear");
        launch_tall(t, s);
    };
    const StepAttnRows attn_rows{qkv, 3 * D, D, m.at<float>(d.rope_cos), m.at<float>(d.rope_sin), b.st.kv_len, b.st.active,
                                 b.pre_k.as<const void*>(), b.pre_v.as<const void*>(), b.pre_len.as<int32_t>(), B};
    for (int l = 0; l < d.n_layers; l++) {
        const auto& L = d.layers[l];
        if (tall) {
            prep(xin, pend, L.n1);
            TallArgs t; t.C = qkv; t.ldc = 3 * D;
            tall_lin(pa_h, pa_l, L.in_proj, t);
        } else {
            FusedIn in;
            in.pend = pend; in.x_out = pend.partial ? x : nullptr; in.norm = &L.n1; in.eps = L.n1.eps;
            step_fused_linear(b, xin, in, L.in_proj, qkv, 3 * D, B, EPI_NONE, nullptr, nullptr, 1.0f);
        }
        pend = PendingSum{}; xin = x;
        launch_attention(attn_step_args(kv_layer(b, l), attn_rows, l, b.capturing ? b.capture_keys : b.kv_bound + 1, attn, D), s);
        {
            GemmArgs go = mk(m, attn, flat(D), L.out_proj, x, flat(D), B);
            go.R = x; go.epi = EPI_RESADD;
            step_gemm(m, go);
        }
        int S = 1;   // linear2's K slices
        if (tall) {
            prep(x, PendingSum{}, L.n2);
            TallArgs t1; t1.ch = pf_h; t1.cl = pf_l; t1.ldp = d.ffn; t1.epi = EPI_GELU;   // gelu(linear1) leaves as the planes linear2 reads
            tall_lin(pa_h, pa_l, L.l1, t1);
            S = std::max(1, std::min(4, d.ffn / 1024));   // 1024-deep K slices: 16 x rows / 64 x S blocks of 8 chunks
            TallArgs t2; t2.R = x; t2.ldr = D;
            if (S > 1) { t2.splitk = S; t2.partial = planes; t2.zstride = (int64_t)B * D; }
            else { t2.epi = EPI_RESADD; t2.C = x; t2.ldc = D; }
            tall_lin(pf_h, pf_l, L.l2, t2);
        } else {
            FusedIn in;
            in.norm = &L.n2; in.eps = L.n2.eps;
            step_fused_linear(b, x, in, L.l1, ff, d.ffn, B, EPI_GELU, nullptr, nullptr, 1.0f);
            GemmArgs g2 = mk(m, ff, flat(d.ffn), L.l2, x, flat(D), B);
            g2.R = x;   // (split: slice 0 stores x + (sums_0 + bias))
            S = pick_split(B, D, d.ffn, g2.w_bf16 != 0 || g2.wt_i8 != 0);
            if (S > 1 && skinny_supported(g2, S)) step_gemm(m, g2, SkinnyFuse{}, S, planes);
            else {
                S = 1; g2.epi = EPI_RESADD;
                step_gemm(m, g2);
            }
        }
        if (S > 1) { xin = planes; pend = PendingSum{planes + (size_t)B * D, S - 1, (int64_t)B * D, nullptr}; }
    }
    float* last = b.last.as<float>();
    float* sy = b.sy.as<float>();
    const float* tc = m.tcomb.at(lsd)->as<float>();
    // out_norm (flow_lm.go:262) feeds out_eos and the flow net's cond_embed.  Both linears carry the norm (and the pending
    // split-K sum of the last linear2) in their prologue -- one launch fewer than a stand-alone LayerNorm (parallel graph
    // branches were tried for these two and for input_proj: the multi-branch graph ran the step 3x slower on ROCm 7.2);
    // cond_embed also writes the normalised rows
    // (`last`: later Euler steps and the staged API read them).  Shapes the fused kernel does not take keep the
    // stand-alone LayerNorm launch.
    bool tail_fused = false;
    {
        FusedIn in;
        in.pend = pend; in.norm = &d.out_norm; in.eps = d.out_norm.eps;
        GemmArgs g1 = mk(m, xin, flat(D), d.cond_embed, sy, flat(C), B), g2 = mk(m, xin, flat(D), d.out_eos, b.eos.as<float>(), flat(1), B);
        const SkinnyFuse fu = fused_prologue(m, in);
        tail_fused = skinny_fuse_supported(g1, fu) && skinny_fuse_supported(g2, fu);
        if (tall && d.cond_eos.wt != NONE) {
            // 128 rows and more: the pending sum and out_norm once per row (k_rowprep writes `last`); [cond_embed ; out_eos] then reads finished rows -- every
            // block of the fused form would redo the four-plane prologue (16.3 us at 256 rows against 4.7 + 8)
            prep(xin, pend, d.out_norm, last);
            GemmArgs g = mk(m, last, flat(D), d.cond_eos, sy, flat(C), B);
            g.epi = EPI_SILU; g.addvec = tc; g.tail = b.eos.as<float>();
            step_gemm(m, g);
            tail_fused = true;
        } else if (tail_fused) {
            in.y_out = last;
            if (d.cond_eos.wt != NONE) {   // one launch: columns 0..C-1 = cond_embed (SiLU epilogue), column C = out_eos (raw)
                GemmArgs g = mk(m, xin, flat(D), d.cond_eos, sy, flat(C), B);
                g.epi = EPI_SILU; g.addvec = tc; g.tail = b.eos.as<float>();
                SkinnyFuse f2 = fu;
                f2.y_out = last;
                step_gemm(m, g, f2);
            } else {
                in.y_out = nullptr;
                step_fused_linear(b, xin, in, d.out_eos, b.eos.as<float>(), 1, B, EPI_NONE, nullptr, nullptr, 1.0f);
                in.y_out = last;
                step_fused_linear(b, xin, in, d.cond_embed, sy, C, B, EPI_SILU, tc, nullptr, 1.0f);
            }
        } else {
            LnArgs ln = mkln(m, xin, flat(D), d.out_norm, last, D, B);
            ln.pend = pend;
            launch_layernorm(ln, s);
            step_gemm(m, mk(m, last, flat(D), d.out_eos, b.eos.as<float>(), flat(1), B));
        }
    }
    b.tail_fused = tail_fused;
    finished = step_flow(b, lsd, opened, fuse_finish, chain);
    if (!b.capturing) b.kv_bound++;   // every live slot has appended one key
    return finished;
}

void step_flow_again(Batch& b, int lsd) {
    b.opened = false; b.par = 0;
    (void)step_flow(b, lsd, false, false, false);
}

// one step as launches, into the stream or a capture: the previous step's last launch normally opened it (b.opened); whoever changes a slot between two
// steps (batch_reset, admission of a newcomer, the staged API, a graph's start) clears the flag, and k_step_begin opens the step for every row.  The
// bookkeeping rides in the step's last launch (shapes it does not take: k_step_finish); chain: that launch opens the next step as well
static void step_launches(Batch& b, int lsd, bool chain) {
    const int ld = b.m->d.ldim;
    if (!b.opened) step_open(b);
    if (!step_core(b, lsd, b.opened, true, chain))
        launch_step_finish(b.st, b.cur_now(), b.eos.as<float>(), ld, b.B, b.latents.as<float>(), (int64_t)b.max_steps * ld, b.m->stream);
}

// the graph of `nsteps` consecutive AR steps whose attention launches cover `ni` load rounds (captured on first use, kept with
// the batch).  Several steps per graph: the gap between two replays (~8 us of idle GPU) is paid once per graph.
static hipGraphExec_t step_graph(Batch& b, int lsd, int ni, int nsteps) {
    Model& m = *b.m;
    if (b.graph_lsd != lsd) {
        b.drop_graphs();
        b.graph_lsd = lsd;
    }
    // two sets (a step with sampling noise reads its noise row: other launches), three columns each: single steps, the short graphs (5 steps:
    // batches that may end by EOS, and the tail of the others), the long ones (25).  A column is re-captured only when ITS step count changes:
    // calls that alternate temperatures, or 25 / 5 / 1 steps, keep their graphs
    const int ns = b.has_noise ? 1 : 0;
    const int col = nsteps <= 1 ? 0 : nsteps <= 5 ? 1 : 2;
    if (col > 0 && b.graph_steps[ns][col - 1] != nsteps) {
        for (auto& row : b.graphs[ns]) if (row[col]) { (void)hipGraphExecDestroy(row[col]); row[col] = nullptr; }
        b.graph_steps[ns][col - 1] = nsteps;
    }
    hipGraphExec_t& slot = b.graphs[ns][ni][col];
    if (slot) return slot;
    hipGraph_t g = nullptr;
    PTTS_HIP(hipStreamBeginCapture(m.stream, hipStreamCaptureModeThreadLocal));
    b.capturing = true;
    b.capture_keys = ni * attn_step_keys_per_round(m.opts.kv == PTTS_KV_BF16);
    try {
        // a graph opens its first step with k_step_begin (slots may have changed since the last one); inside, every step's last launch opens the next
        b.opened = false;
        for (int k = 0; k < nsteps; k++) step_launches(b, lsd, k + 1 < nsteps);
        b.opened = false;
    } catch (...) {
        b.capturing = false;
        b.opened = false;
        (void)hipStreamEndCapture(m.stream, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    b.capturing = false;
    PTTS_HIP(hipStreamEndCapture(m.stream, &g));
    hipError_t e = hipGraphInstantiate(&slot, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) throw Error(PTTS_ENODEVICE, strfmt("hip: hipGraphInstantiate failed: %s", hipGetErrorString(e)));
    return slot;
}

// nsteps > 1 only with use_graph
void enqueue_step(Batch& b, int lsd, bool use_graph, int nsteps) {
    Model& m = *b.m;
    if (use_graph) {
        const int ni = attn_step_rounds(std::min(b.kv_bound + nsteps, b.cap), m.opts.kv == PTTS_KV_BF16);
        PTTS_HIP(hipGraphLaunch(step_graph(b, lsd, ni, nsteps), m.stream));
        b.kv_bound += nsteps;
        b.opened = false;   // (a graph ends unchained)
        return;
    }
    step_launches(b, lsd, true);
}

}  // namespace ptts
