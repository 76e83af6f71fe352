// launch_args.h -- the launch forms the engine's phases share, built in one place: the operand makers of the products and norms, and the three forms of
// AttnArgs (the AR step on the KV cache, the ragged prompt prefill on the same cache, the dense window over one q|k|v buffer).  The kernel test hooks
// (capi_hooks.cpp) build their launches with the same functions, so a stride changed here changes what the value-level tests check.
#pragma once

#include <algorithm>

#include "runtime.h"

namespace ptts {

inline RowMap flat(int64_t ld) { return RowMap{ld, 0, 0}; }
inline RowMap seg(int64_t ld, int64_t rows_per_batch, int64_t batch_stride) { return RowMap{ld, rows_per_batch, batch_stride}; }

inline GemmArgs mk(const Model& m, const float* A, RowMap am, const Lin& l, float* C, RowMap cm, int M) {
    GemmArgs g;
    g.A = A; g.amap = am;
    g.W = m.arena + l.w; g.w_bf16 = l.bf16; g.ldw = l.in;
    g.Wt = l.wt == NONE ? nullptr : m.arena + l.wt;
    g.wt_i8 = l.wt_i8; g.wscale = m.at<float>(l.wscale);
    g.bias = m.at<float>(l.b);
    g.C = C; g.cmap = cm;
    g.M = M; g.N = l.out; g.K = l.in;
    return g;
}
// mk without the step's fragment-ordered copy.  launch_gemm sends an M <= 64 product WITH Wt to k_skinny; the callers of this one stay on the many-row
// kernels whatever M is: the staged flow direction (the independent check of the step's flow part) and the speaker projection (staged.cpp)
inline GemmArgs mk_rows(const Model& m, const float* A, RowMap am, const Lin& l, float* C, RowMap cm, int M) {
    GemmArgs g = mk(m, A, am, l, C, cm, M);
    g.Wt = nullptr;
    return g;
}
inline LnArgs mkln(const Model& m, const float* x, RowMap xm, const Norm& n, float* y, int64_t ldy, int rows) {
    LnArgs a;
    a.x = x; a.xmap = xm;
    a.w = m.at<float>(n.w); a.b = m.at<float>(n.b);
    a.eps = n.eps;
    a.y = y; a.ldy = ldy;
    a.rows = rows; a.d = n.d;
    return a;
}

// one layer of a KV cache, [slot][head][cap][hd] in the cache dtype (kernels.h launch_kv_append writes it)
struct KvLayer { const void* k; const void* v; int bf16, heads, cap, hd; };
inline KvLayer kv_layer(const Batch& b, int layer) { return KvLayer{b.kc(layer), b.vc(layer), b.m->opts.kv == PTTS_KV_BF16 ? 1 : 0, b.m->d.heads, b.cap, b.m->d.hd}; }
inline void attn_on_cache(AttnArgs& a, const KvLayer& c) {
    a.k = c.k; a.v = c.v; a.kv_bf16 = c.bf16;
    a.k_seg_stride = (int64_t)c.heads * c.cap * c.hd; a.k_head_stride = (int64_t)c.cap * c.hd; a.k_row_stride = c.hd;
    a.heads = c.heads; a.hd = c.hd;
}

// The AR step: row r is slot r's one query at position seg_len[r]; q, k, v come from the row's qkv (q|k|v at columns 0, d_model, 2 d_model), are
// rotated and appended inside the launch; keys below pre_len[r] are read from the slot's shared voice prefix; no window; the score buffer is sized
// for the whole cache.  keys_now: AttnArgs::keys_now
struct StepAttnRows {
    const float* qkv; int64_t qkv_ld; int d_model;
    const float* cos_t; const float* sin_t;
    const int32_t* seg_len; const int32_t* active;
    const void* const* pre_k; const void* const* pre_v; const int32_t* pre_len;
    int rows;
};
inline AttnArgs attn_step_args(const KvLayer& c, const StepAttnRows& r, int layer, int keys_now, float* out, int64_t out_ld) {
    AttnArgs a;
    attn_on_cache(a, c);
    a.seg_len = r.seg_len; a.active = r.active;
    a.context = -1;
    a.out = out; a.out_ld = out_ld;
    a.rows = r.rows; a.max_keys = c.cap;
    a.keys_now = keys_now;
    a.fused_step = 1; a.qkv = r.qkv; a.qkv_ld = r.qkv_ld; a.d_model = r.d_model;
    a.cos_t = r.cos_t; a.sin_t = r.sin_t; a.cap = c.cap;
    a.pre_k = r.pre_k; a.pre_v = r.pre_v; a.pre_len = r.pre_len; a.layer = layer;
    return a;
}

// The ragged prompt prefill: the rows of segment s are the packed rows [rag_off[s], rag_off[s + 1]) at positions pos0[s] + i.  One table, one upload,
// holds the four views the launches read: row -> segment | row -> position | rag_off [segs + 1] | pos0 [segs].
struct RaggedMeta {
    std::vector<int32_t> table;
    int rows = 0, segs = 0, longest = 0, max_pos = 0;   // longest: the most rows a segment has; max_pos: the last position any row sits at
    const int32_t* row_seg(const int32_t* dev) const { return dev; }   // the first two views inside the table's device copy (the prefill's RoPE and KV append read them too)
    const int32_t* row_pos(const int32_t* dev) const { return dev + rows; }
};
inline RaggedMeta ragged_meta(const int32_t* rag_off, const int32_t* pos0, int segs) {   // (the caller has checked: rag_off ascends from 0, pos0 >= 0)
    RaggedMeta t;
    t.rows = rag_off[segs]; t.segs = segs;
    t.table.resize((size_t)2 * t.rows + 2 * segs + 1);
    int32_t* const row_seg = t.table.data();
    int32_t* const row_pos = row_seg + t.rows;
    for (int s = 0; s < segs; s++) {
        const int n = rag_off[s + 1] - rag_off[s];
        t.longest = std::max(t.longest, n);
        if (n > 0) t.max_pos = std::max(t.max_pos, pos0[s] + n - 1);
        for (int i = 0; i < n; i++) { row_seg[rag_off[s] + i] = s; row_pos[rag_off[s] + i] = pos0[s] + i; }
    }
    std::copy(rag_off, rag_off + segs + 1, row_pos + t.rows);
    std::copy(pos0, pos0 + segs, row_pos + t.rows + segs + 1);
    return t;
}
// q: the packed rows, the query of (row, head) at q + row * q_ld + head * hd; meta_dev: the device copy of t.table
inline AttnArgs attn_ragged_args(const KvLayer& c, const RaggedMeta& t, const int32_t* meta_dev, const float* q, int64_t q_ld, int context, float* out, int64_t out_ld) {
    AttnArgs a;
    attn_on_cache(a, c);
    a.q = q; a.q_ld = q_ld; a.q_col0 = 0;
    a.row_seg = t.row_seg(meta_dev); a.row_pos = t.row_pos(meta_dev);
    a.rag_off = a.row_pos + t.rows; a.rag_pos0 = a.rag_off + t.segs + 1; a.rag_segs = t.segs; a.rows_per_seg = t.longest;
    a.context = context;
    a.out = out; a.out_ld = out_ld;
    a.rows = t.rows; a.max_keys = t.max_pos + 1;
    return a;
}

// The dense window (the Mimi transformers): one f32 buffer [segs][T1][ld] with q | k | v at columns 0, D, 2 D of a row, positions from 0 in every
// segment; the queries are rows [t0, t0 + CT) of each segment (earlier rows hold the keys and values of earlier chunks), the window is `context` keys.
inline AttnArgs attn_dense_args(const float* qkv, int64_t ld, int D, int segs, int T1, int t0, int CT, int heads, int hd, int context, float* out, int64_t out_ld) {
    AttnArgs a;
    a.q = qkv + (size_t)t0 * ld; a.q_ld = ld; a.q_col0 = 0; a.q_rows_per_batch = CT; a.q_batch_stride = (int64_t)T1 * ld;
    a.k = qkv + D; a.v = qkv + 2 * D; a.kv_bf16 = 0;
    a.k_seg_stride = (int64_t)T1 * ld; a.k_head_stride = hd; a.k_row_stride = ld;
    a.rows_per_seg = CT; a.pos_base = t0;
    a.context = context;
    a.out = out; a.out_ld = out_ld;
    a.rows = segs * CT; a.heads = heads; a.hd = hd; a.max_keys = std::min(T1, context);
    return a;
}

}  // namespace ptts
