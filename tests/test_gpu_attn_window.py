"""The window attention (csrc/attn_window.hip: k_attn_window<KVBF16, RAGGED> and k_attn_window_lds<4>) stand-alone, value by value, against f64 numpy on operands
the test controls -- every launch form, with the strides, heads, segments and positions its three callers really pass.

What it replaces: mimiTransformerLayer.selfAttention (mimi.go:365-441: softmax(q K^T / 8) V over the keys p - context + 1 .. p of the query's own utterance and
head) for the Mimi decoder and encoder, and the prompt prefill's attention over a slot's cache rows 0 .. p (flow_transformer.go:749-771).  The hook
(ptts_debug_attn_window) fills AttnArgs as the callers do:
  dense  (mimi_decode.cpp mimi_range, encoder.cpp): ONE buffer [segs][T1][ld] holds q | k | v at columns 0, D, 2 D; a chunk (t0, CT) of every segment is launched with
         pos_base = t0, k_row_stride = q_ld = ld, k_head_stride = 64 -- form 0 through launch_attention (today k_attn_window_lds<4>), 1 k_attn_window<false, false>
         (dispatched in production only beyond 2^31 elements per segment: reachable through this hook alone), 2 k_attn_window_lds<4>;
  ragged (batch.cpp, the prompt prefill): packed query rows, caches [segs][heads][cap][64] in f32 or bf16, rag_off / rag_pos0 -- form 0, k_attn_window<., true>.
Geometry: 2 heads and 2 segments (dense), 3 heads and 1-5 segments (ragged), ld = 3 D + 4, out_ld = D + 4: every stride differs from every other.

Reference: f64, per row the keys max(0, p - ctx + 1) .. p of its own segment and head; a bf16 cache is decoded exactly (no cache-format term in the tolerance).

Poison: everything no query of the launch may see holds 0xff bytes (a NaN in f32 and in bf16), in a few cases canonical NaNs: dense rows >= t0 + CT and rows
< t0 - ctx + 1 (all columns), the q columns of every row outside the chunk, the pad columns; ragged cache rows > rag_pos0[s] + n_s - 1, the columns of the
packed rows behind q.  Masking happens after the first product, so a row that must not be visible must never be LOADED: 0 * NaN through the second product
is a NaN in the output.  `out` is 0xff before the launch: the pad columns must come back untouched, and a second run must give the same bits.

Tolerance, per output element e of a (row, head); u = 2^-24, b = 2^-16 (what the hi + lo split of an f32 into two bf16 leaves: each half rounds to 8 bits),
q' = q / 8 (exact), A = max over visible j of sum_e |q'_e k_je|, V_e = max_j |v_je|, W_e = max_j v_je - min_j v_je over the row's visible keys:
  score    three MFMAs per step (hi hi + lo hi + hi lo), lo lo dropped and the two split residues: 3 b per product; 12 chained MFMAs of 16 products each, f32:
           a product passes at most 16 + 12 roundings:                                                         ds <= A (3 b + 28 u)
  weight   p_j = __expf(s_j - m): the subtraction (16 u for a spread <= 16, which reference() asserts), v_exp_f32 on x log2(e) (1 ulp and the rounded argument:
           34 u), both scores (2 ds); the running rescale over at most 13 key tiles (visible keys <= 400 + 31): per tile one __expf (50 u) and one
           multiplication:                                                                                     eps <= 2 ds + 50 u + 13 * 52 u = 2 ds + 726 u
  out      a convex combination of the v_j: relative weight errors eps move it by at most eps W_e; P and V are split again (3 b V_e); the numerator passes
           16 + 6 roundings in its tile and 7 per later tile (106 u), the denominator 16 + 1 per tile (222 u), the final reciprocal and product 2 u:
           bound_e = eps W_e + V_e (3 b + 330 u), never above CEIL = 1e-4 absolute, which this kernel is already held to (test_window_kernel_random_against_the_oracle,
           ops/tolerance.go).
  A bf16 cache has no lo half (2 b instead of 3 b in both products): the f32 bound covers it.
The split terms dominate (3 b = 768 u): as a worst case -- every residue at its limit and of one sign -- the bound exceeds CEIL on nearly every element of
a row with more than a few keys, so CEIL is the working tolerance there and the derived bound holds the short rows (one key: W_e = 0, bound 6.6e-5 V_e).
test_emulation_stays_within_half_the_bound (no GPU) runs a numpy f32 emulation in the kernels' order (the tile alignment of each form, hi / lo split, three
products, streaming softmax with the rescale, the two half-wave sums of l) over every case and holds it to HALF the bound: it comes out at 0.23 of it
(largest |error| 2.3e-5), on rows of one or two keys, where nothing averages the split residue of v (about 2^-17 |v|) and the derived bound, not CEIL, is what
holds; where every row sees 160 keys and more (the chunks at 160 and 300) the error is 1.6e-6 flat / 6.1e-6 peaked.  OBSERVED on the MI355X (profiles/attn_window_parity.txt), largest error / bound per form and
family: dense forms 0, 1 and 2 alike 0.196 flat / 0.234 peaked (|error| 2.0e-5 / 2.3e-5, the emulation's own figures: on a row of one key the arithmetic
leaves no freedom), ragged f32 0.148 / 0.170, ragged bf16 0.056 / 0.099 -- every form inside half the bound, so no term is missing and the bound is used as
derived.

What makes a wrong key fail is the flat family (q scaled by 0.25: scores spread by 1-2): test_flat_cases_feel_every_key (no GPU) asserts on the f64 reference
alone that dropping a row's oldest key, admitting key p - ctx or p + 1, replacing any visible key's K and V rows by the next row's, or by the same row of the
next head or segment, moves some element of the row by at least 10 x its tolerance -- which is why every row sees at most 400 keys.  The peaked family (q at
scale 1: spread about 6) is for errors in score, max and exp."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round, split
from _parity import record

F32 = np.float32
U, B16 = 2.0 ** -24, 2.0 ** -16
CEIL = 1e-4
MAX_VISIBLE = 400
FAMILIES = ("flat", "peaked")
FORMS = (0, 1, 2)
FORM_KERNEL = {1: "k_attn_window<false,false>", 2: "k_attn_window_lds<4>"}


# ------------------------------------------------------------------------------------------------ number formats
def to_bits(a, fmt):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (u >> 16).astype(np.uint16) if fmt == "bf16" else u.copy()


def poison_bits(fmt, pad):
    """what rows and columns outside the launch hold: 0xff bytes, or the canonical NaN"""
    if pad == "ff":
        return np.uint16(0xFFFF) if fmt == "bf16" else np.uint32(0xFFFFFFFF)
    return np.uint16(0x7FC0) if fmt == "bf16" else np.uint32(0x7FC00000)


# ------------------------------------------------------------------------------------------------ cases
def dense(ctx, t0, ct, segs=2, family="flat", pad="ff"):
    return dict(kind="dense", heads=2, segs=segs, ctx=ctx, t0=t0, ct=ct, t1=t0 + ct + 3, fmt="f32", family=family, pad=pad)


def ragged(lens, pos0, fmt, ctx=-1, family="flat", pad="ff"):
    lens, pos0 = tuple(lens), tuple(pos0) if isinstance(pos0, (tuple, list)) else (pos0,) * len(lens)
    return dict(kind="ragged", heads=3, segs=len(lens), lens=lens, pos0=pos0, cap=max(p + n for p, n in zip(pos0, lens)) + 3, ctx=ctx, fmt=fmt, family=family, pad=pad)


def cid(c):
    if c["kind"] == "dense":
        s = f"dense-ctx{c['ctx']}-t{c['t0']}+{c['ct']}-s{c['segs']}"
    else:
        s = "ragged-" + c["fmt"] + "-n" + ",".join(map(str, c["lens"])) + "-p" + ",".join(map(str, c["pos0"])) + (f"-ctx{c['ctx']}" if c["ctx"] > 0 else "")
    return s + "-" + c["family"] + ("-nanpad" if c["pad"] != "ff" else "")


DENSE_SHAPES = (
    [(250, 0, ct, 2) for ct in (1, 31, 32, 33, 127, 128, 129, 250, 251, 282, 400)] +                    # whole range: tile, block and window edges
    [(250, t0, ct, 2) for t0, ct in ((16, 16), (160, 160), (249, 2), (250, 1), (300, 129), (1000, 40))] +  # streamed chunks, pos_base != 0
    [(ctx, 0, 200, 2) for ctx in (1, 2, 7, 31, 32, 33, 64, 128)] +                                      # windows shorter than a tile / a block; tile skip; maskless path
    [(ctx, 150, 70, 2) for ctx in (7, 33)] +                                                            # the same with pos_base != 0
    [(1000, 0, 300, 2)] +                                                                               # ctx >= T1: no window effect
    [(250, 0, 300, 1)])                                                                                 # the encoder's call shape: one segment, positions from 0
RAGGED_SHAPES = [
    ((70, 5, 33), (0, 0, 9), -1),              # baseline (the lengths of test_prefill_ragged_long_prompts_on_the_matrix_cores)
    ((1,), 0, -1),                             # a single row
    ((31,), 0, -1), ((32,), 0, -1), ((33,), 0, -1),   # tile edges
    ((128, 129), 0, -1),                       # two groups of four waves, the second with one live wave
    ((3,), 300, -1),                           # many key tiles, one query tile
    ((40, 0, 7), 0, -1),                       # an empty segment between live ones
    ((9, 40, 1, 33, 17), (0, 64, 31, 5, 100), -1),   # pos0 varies across five segments
    ((70,), 100, 50),                          # a window on ragged rows: the kernel supports it, production does not use it
]
DENSE_CASES = [dense(ctx, t0, ct, segs, family=f) for ctx, t0, ct, segs in DENSE_SHAPES for f in FAMILIES]
RAGGED_CASES = [ragged(lens, p0, fmt, ctx, family=f) for lens, p0, ctx in RAGGED_SHAPES for fmt in ("f32", "bf16") for f in FAMILIES]
NAN_CASES = ([dense(ctx, t0, ct, pad="nan") for ctx, t0, ct in ((250, 300, 129), (33, 150, 70), (250, 0, 33))] +
             [ragged(lens, p0, fmt, pad="nan") for lens, p0 in (((70, 5, 33), (0, 0, 9)), ((40, 0, 7), 0)) for fmt in ("f32", "bf16")])
ALL_CASES = DENSE_CASES + RAGGED_CASES + NAN_CASES
CASE_BY_ID = {cid(c): c for c in ALL_CASES}


def case_forms(c):
    return FORMS if c["kind"] == "dense" else (0,)


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _operands(key):
    """clean: finite data everywhere (what the sensitivity test borrows rows from); the launch's operands: the same with everything outside the launch poisoned."""
    c = CASE_BY_ID[key]
    H, S = c["heads"], c["segs"]
    D = H * 64
    ld = 3 * D + 4
    fmt = c["fmt"]
    rng = np.random.default_rng(zlib.crc32(key.replace("-nanpad", "").encode()))
    qs = 0.25 if c["family"] == "flat" else 1.0
    pz32 = poison_bits("f32", c["pad"])
    if c["kind"] == "dense":
        t0, ct, t1, ctx = c["t0"], c["ct"], c["t1"], c["ctx"]
        clean = rng.standard_normal((S, t1, ld)).astype(F32)
        clean[:, :, :D] *= F32(qs)
        buf = np.full((S, t1, ld), pz32, np.uint32)
        lo = max(0, t0 - ctx + 1)
        buf[:, t0:t0 + ct, :D] = clean[:, t0:t0 + ct, :D].view(np.uint32)
        buf[:, lo:t0 + ct, D:3 * D] = clean[:, lo:t0 + ct, D:3 * D].view(np.uint32)
        return dict(clean=clean, qkv=buf.view(F32), D=D, ld=ld)
    lens, pos0, cap = c["lens"], c["pos0"], c["cap"]
    R = sum(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    q = np.full((R, ld), pz32, np.uint32)
    qc = (F32(qs) * rng.standard_normal((R, D))).astype(F32)
    q[:, :D] = qc.view(np.uint32)
    kv = rng.standard_normal((2, S, H, cap, 64)).astype(F32)
    if fmt == "bf16":
        kv = bf16_round(kv)
    k, v = to_bits(kv[0], fmt), to_bits(kv[1], fmt)
    for s in range(S):
        k[s, :, pos0[s] + lens[s]:], v[s, :, pos0[s] + lens[s]:] = poison_bits(fmt, c["pad"]), poison_bits(fmt, c["pad"])
    return dict(q_clean=qc, kv_clean=kv, qkv=q.view(F32), k=k, v=v, rag_off=off, rag_pos0=np.array(pos0, np.int32), D=D, ld=ld)


def operands(c):
    return _operands(cid(c))


def units(c, dtype=np.float64):
    """the launch as independent attentions: (segment, head, out rows [n], positions [n], Q [n, 64], kv) with kv(s, h) -> (K, V) [keys, 64] of ANY segment and head,
    from the clean data (rows beyond the launch included)"""
    o = operands(c)
    H, S, D = c["heads"], c["segs"], o["D"]
    if c["kind"] == "dense":
        t0, ct = c["t0"], c["ct"]
        cl = o["clean"].astype(dtype)

        def kv(s, h):
            return cl[s, :, D + 64 * h:D + 64 * h + 64], cl[s, :, 2 * D + 64 * h:2 * D + 64 * h + 64]
        for s in range(S):
            for h in range(H):
                yield s, h, s * ct + np.arange(ct), t0 + np.arange(ct), cl[s, t0:t0 + ct, 64 * h:64 * h + 64], kv
    else:
        qc, kvc = o["q_clean"].astype(dtype), o["kv_clean"].astype(dtype)

        def kv(s, h):
            return kvc[0, s, h], kvc[1, s, h]
        for s in range(S):
            n = c["lens"][s]
            if n == 0:
                continue
            rows = o["rag_off"][s] + np.arange(n)
            for h in range(H):
                yield s, h, rows, c["pos0"][s] + np.arange(n), qc[rows, 64 * h:64 * h + 64], kv


def n_rows(c):
    return c["segs"] * c["ct"] if c["kind"] == "dense" else sum(c["lens"])


# ------------------------------------------------------------------------------------------------ the f64 reference and the bound
def blocks(pos, ctx, before=0, after=0):
    """32 rows at a time: (row slice, first key, last key) of the union of their windows, widened by `before` / `after` keys"""
    for b in range(0, len(pos), 32):
        p = pos[b:b + 32]
        lo = max(0, p[0] - ctx + 1) if ctx > 0 else 0
        yield slice(b, b + len(p)), max(0, lo - before), p[-1] + after


def visible(p, j, ctx):
    vis = j[None, :] <= p[:, None]
    return vis & (j[None, :] > p[:, None] - ctx) if ctx > 0 else vis


def attend(Q, K, V, pos, ctx):
    """(out [n, 64], bound [n, 64]) of one (segment, head) in f64"""
    out, bnd = np.empty((len(pos), 64)), np.empty((len(pos), 64))
    for rs, lo, hi in blocks(pos, ctx):
        p, j = pos[rs], np.arange(lo, hi + 1)
        k, v, q = K[lo:hi + 1], V[lo:hi + 1], Q[rs] * 0.125
        vis = visible(p, j, ctx)
        assert vis.sum(axis=1).max() <= MAX_VISIBLE
        s = np.where(vis, q @ k.T, -np.inf)
        assert (s.max(axis=1) - np.where(vis, s, np.inf).min(axis=1) <= 16.0).all()   # the spread the bound's __expf term assumes
        w = np.exp(s - s.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        out[rs] = w @ v
        A = np.where(vis, np.abs(q) @ np.abs(k).T, 0.0).max(axis=1)
        eps = 2.0 * A * (3 * B16 + 28 * U) + 726 * U
        vv = np.where(vis[:, :, None], v[None], np.nan)
        W, Vm = np.nanmax(vv, axis=1) - np.nanmin(vv, axis=1), np.nanmax(np.abs(vv), axis=1)
        bnd[rs] = np.minimum(CEIL, eps[:, None] * W + Vm * (3 * B16 + 330 * U))
    return out, bnd


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = CASE_BY_ID[key]
    D = c["heads"] * 64
    out, bnd = np.zeros((n_rows(c), D)), np.zeros((n_rows(c), D))
    for s, h, rows, pos, Q, kv in units(c):
        K, V = kv(s, h)
        out[rows, 64 * h:64 * h + 64], bnd[rows, 64 * h:64 * h + 64] = attend(Q, K, V, pos, c["ctx"])
    out.setflags(write=False)
    bnd.setflags(write=False)
    return out, bnd


def reference(c):
    """(out [rows, D], bound [rows, D]), computed once per case and shared, read-only, by every form and test"""
    return _reference(cid(c))


def test_case_ids_are_unique_and_every_listed_case_is_present():
    assert len(CASE_BY_ID) == len(ALL_CASES)
    assert len(DENSE_CASES) == 2 * (11 + 6 + 8 + 2 + 1 + 1) and len(RAGGED_CASES) == 2 * 2 * 10
    for c in ALL_CASES:
        o = operands(c)
        assert o["ld"] == 3 * o["D"] + 4 and n_rows(c) <= 4096
        ref, bnd = reference(c)
        assert np.isfinite(ref).all() and (bnd > 0).all() and (bnd <= CEIL).all()


def test_poison_covers_everything_outside_the_launch():
    """the operands the GPU sees: NaN in every element the docstring lists, finite data in every element some query of the launch reads"""
    for c in ALL_CASES:
        o = operands(c)
        D, x = o["D"], o["qkv"]
        if c["kind"] == "dense":
            t0, ct, ctx = c["t0"], c["ct"], c["ctx"]
            lo = max(0, t0 - ctx + 1)
            assert np.isnan(x[:, :, 3 * D:]).all() and np.isnan(x[:, t0 + ct:]).all() and np.isnan(x[:, :lo]).all() and x[:, t0 + ct:].shape[1] == 3
            assert np.isnan(x[:, :t0, :D]).all() and np.isfinite(x[:, t0:t0 + ct, :D]).all() and np.isfinite(x[:, lo:t0 + ct, D:3 * D]).all()
        else:
            assert np.isnan(x[:, D:]).all() and np.isfinite(x[:, :D]).all()
            for s, (n, p0) in enumerate(zip(c["lens"], c["pos0"])):
                for a in (o["k"], o["v"]):
                    f = (a[s].astype(np.uint32) << 16).view(F32) if c["fmt"] == "bf16" else a[s].view(F32)
                    assert np.isnan(f[:, p0 + n:]).all() and f[:, p0 + n:].shape[1] >= 3 and np.isfinite(f[:, :p0 + n]).all()


# ------------------------------------------------------------------------------------------------ what a wrong key would do to the reference (no GPU)
def test_flat_cases_feel_every_key():
    """for every flat case, row and head, on the f64 reference alone: each of the kernel's possible key mistakes moves some element of the row by >= 10 x that
    element's tolerance.  e_j: unnormalised weights, Z their sum, N = sum e_j v_j; a replaced key (k', v') gives (N - e_j v_j + e' v') / (Z - e_j + e')."""
    worst = {}
    for c in ALL_CASES:
        if c["family"] != "flat" or c["pad"] != "ff":
            continue
        ctx, H, S = c["ctx"], c["heads"], c["segs"]
        bnd_all = reference(c)[1]
        low = {}
        for s, h, rows, pos, Q, kv in units(c):
            K, V = kv(s, h)
            others = [("next head", kv(s, (h + 1) % H))] + ([("next segment", kv((s + 1) % S, h))] if S > 1 else [])
            for rs, lo, hi in blocks(pos, ctx, before=1, after=1):
                p, j = pos[rs], np.arange(lo, hi + 1)
                q, k, v = Q[rs] * 0.125, K[lo:hi + 1], V[lo:hi + 1]
                tol = bnd_all[rows[rs], 64 * h:64 * h + 64]              # [n, 64]
                vis = visible(p, j, ctx)
                s_all = q @ k.T
                mx = np.where(vis, s_all, -np.inf).max(axis=1, keepdims=True)
                e_all = np.exp(s_all - mx)                               # [n, keys]: also of keys that are not visible
                e = np.where(vis, e_all, 0.0)
                Z, N = e.sum(axis=1), e @ v
                out = N / Z[:, None]
                ar = np.arange(len(p))

                def moved(d):                                            # [..., 64] -> the largest move / tolerance over the row's elements
                    return (np.abs(d) / (tol if d.ndim == 2 else tol[:, None, :])).max(axis=-1)

                def note(what, r):
                    if r.size:
                        low[what] = min(low.get(what, np.inf), float(r.min()))
                many = vis.sum(axis=1) > 1
                old = vis.argmax(axis=1)                                 # the oldest visible key
                eo = e[ar, old]
                note("drop the oldest key", moved((eo / np.where(many, Z - eo, 1.0))[:, None] * (out - v[old]))[many])   # (a row of one key has none to lose)
                for what, idx in (("admit key p - ctx", p - ctx - lo if ctx > 0 else None), ("admit key p + 1", p + 1 - lo)):
                    if idx is None:
                        continue
                    ok = idx >= 0
                    ii = np.where(ok, idx, 0)
                    ex = e_all[ar, ii]
                    note(what, moved((ex / (Z + ex))[:, None] * (v[ii] - out))[ok])
                # any visible key replaced: by the next row (j + 1; column `after` keeps it inside the block), by the same row of the next head / segment
                repl = [("neighbour's rows", e_all[:, 1:], v[1:])]
                for what, (K2, V2) in others:
                    k2 = K2[lo:hi + 1]
                    repl.append((what, np.exp(q @ k2.T - mx)[:, :-1], V2[lo:hi]))
                for what, e2, v2 in repl:
                    e1, v1, vs = e[:, :-1], v[:-1], vis[:, :-1]
                    new = (N[:, None, :] - e1[:, :, None] * v1[None] + e2[:, :, None] * v2[None]) / (Z[:, None] - e1 + e2)[:, :, None]
                    note(what, moved(new - out[:, None, :])[vs])
        worst[cid(c)] = low
        assert low and min(low.values()) >= 10.0, (cid(c), low)
        assert {"admit key p + 1", "neighbour's rows", "next head"} <= set(low), (cid(c), sorted(low))
    assert len(worst) == len(DENSE_SHAPES) + 2 * len(RAGGED_SHAPES)
    for what in ("drop the oldest key", "admit key p - ctx", "admit key p + 1", "neighbour's rows", "next head", "next segment"):
        print(f"smallest move / tolerance, {what}: {min(w[what] for w in worst.values() if what in w):.1f}")


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in numpy f32 (no GPU)
# the key a score register holds: register r of half-wave g is key (r & 3) + 8 (r >> 2) + 4 g of the tile
KEY_OF = np.array([[(r & 3) + 8 * (r >> 2) + 4 * g for r in range(16)] for g in range(2)])


def emulate_unit(Q, K, V, pos, ctx, lds, kv_bf16):
    """one (segment, head) in the kernels' order, all its waves at once: tiles of 32 keys from the wave's first visible key (k_attn_window) or the block's
    (k_attn_window_lds: a tile no query of the wave sees is skipped there, which leaves every sum as it is -- as a fully masked tile does here)."""
    n, pos0 = len(pos), int(pos[0])
    nw = (n + 31) // 32
    r0 = np.arange(nw) * 32
    nq = np.minimum(32, n - r0)
    qi = r0[:, None] + np.minimum(np.arange(32)[None, :], nq[:, None] - 1)         # [nw, 32]: lanes past the end replay the last query
    my_pos = pos0 + qi
    C = ctx if ctx > 0 else 1 << 30
    p_last = pos0 + r0 + nq - 1
    if lds:
        b0 = (r0 // 128) * 128
        start, last_load = np.maximum(0, pos0 + b0 - C + 1), pos0 + np.minimum(b0 + 128, n) - 1
    else:
        start, last_load = np.maximum(0, pos0 + r0 - C + 1), p_last
    tiles = int(((p_last - start) // 32 + 1).max())
    qh, ql = split(Q[qi] * F32(0.125))                                               # [nw, 32, 64]
    m = np.full((nw, 32), -np.inf, F32)
    l = np.zeros((nw, 32, 2), F32)
    o = np.zeros((nw, 32, 64), F32)
    for t in range(tiles):
        key = start[:, None] + 32 * t + np.arange(32)[None, :]                       # [nw, 32]
        src = np.minimum(key, last_load[:, None])                                   # (keys past the last position: a valid row is read again)
        kh, kl = split(K[src])                                                      # [nw, 32 keys, 64]
        vh, vl = split(V[src])
        s = np.zeros((nw, 32, 32), F32)                                             # [wave, query, key]
        for i in range(4):
            d = slice(16 * i, 16 * i + 16)
            s = s + qh[:, :, d] @ kh[:, :, d].transpose(0, 2, 1)
            if not kv_bf16:
                s = s + qh[:, :, d] @ kl[:, :, d].transpose(0, 2, 1)
            s = s + ql[:, :, d] @ kh[:, :, d].transpose(0, 2, 1)
        ok = (key[:, None, :] <= my_pos[:, :, None]) & (key[:, None, :] > my_pos[:, :, None] - C)
        s = np.where(ok, s, F32(-np.inf))
        m_new = np.maximum(m, s.max(axis=2))
        m_use = np.where(np.isneginf(m_new), F32(0), m_new)
        alpha = np.exp(m - m_use)
        m = m_new
        l = l * alpha[:, :, None]
        o = o * alpha[:, :, None]
        p = np.exp(s - m_use[:, :, None])                                           # f32
        for r in range(16):
            l = l + p[:, :, KEY_OF[:, r]]
        ph, pl = split(p)
        for i in range(2):
            ks = KEY_OF[:, 8 * i:8 * i + 8].reshape(-1)                             # the 16 keys of step i
            o = o + ph[:, :, ks] @ vh[:, ks]
            if not kv_bf16:
                o = o + ph[:, :, ks] @ vl[:, ks]
            o = o + pl[:, :, ks] @ vh[:, ks]
    inv = F32(1.0) / (l[:, :, 0] + l[:, :, 1])
    out = np.empty((n, 64), F32)
    for w in range(nw):
        out[r0[w]:r0[w] + nq[w]] = (o[w] * inv[w][:, None])[:nq[w]]
    return out


def emulate(c, lds):
    out = np.zeros((n_rows(c), c["heads"] * 64), F32)
    for s, h, rows, pos, Q, kv in units(c, F32):
        K, V = kv(s, h)
        out[rows, 64 * h:64 * h + 64] = emulate_unit(Q, K, V, pos, c["ctx"], lds, c["fmt"] == "bf16")
    return out


def test_emulation_stays_within_half_the_bound():
    worst, worst_abs = {}, 0.0
    for c in ALL_CASES:
        want, bnd = reference(c)
        for lds in ((False, True) if c["kind"] == "dense" else (False,)):
            got = emulate(c, lds)
            err = np.abs(got - want)
            ratio = float((err / bnd).max())
            key = ("lds" if lds else "wave", c["family"])
            worst[key] = max(worst.get(key, 0.0), ratio)
            worst_abs = max(worst_abs, float(err.max()))
            assert np.isfinite(got).all() and ratio <= 0.5, (cid(c), lds, ratio)
    print("emulation: largest error / bound", worst, "largest error", worst_abs)


# ------------------------------------------------------------------------------------------------ refusals (no GPU: every check comes before the device is touched)
def test_refusals_before_any_launch(pkg):
    """every operand that could take an access outside the hook's buffers is PTTS_EINVAL with a message that names it, and the census shows no launch."""
    rt = pkg.runtime
    cd, cr = dense(250, 16, 16), ragged((70, 5, 33), (0, 0, 9), "f32")
    od, orr = operands(cd), operands(cr)
    D2, D3 = od["D"], orr["D"]

    def d(**kw):
        a = dict(qkv=od["qkv"], heads=2, context=250, form=0, t0=16, ct=16, out_ld=D2 + 4)
        a.update(kw)
        return lambda: rt.debug_attn_window(a.pop("qkv"), **a)

    def r(**kw):
        a = dict(qkv=orr["qkv"], heads=3, context=-1, form=0, k=orr["k"], v=orr["v"], rag_off=orr["rag_off"], rag_pos0=orr["rag_pos0"], out_ld=D3 + 4)
        a.update(kw)
        return lambda: rt.debug_attn_window(a.pop("qkv"), **a)

    def arr(a, i, val):
        a = a.copy()
        a[i] = val
        return a
    big = np.zeros((17, 4, 3 * 64 + 4), F32)
    bad = {
        "t0 + CT > T1": (d(t0=16, ct=20), "leaves the 35 rows"),
        "t0 < 0": (d(t0=-1, ct=4), "leaves the 35 rows"),
        "CT < 1": (d(ct=0), "leaves the 35 rows"),
        "ld not a multiple of 4": (d(qkv=od["qkv"][:, :, :3 * D2 + 2]), "16-byte alignment"),
        "out_ld not a multiple of 4": (d(out_ld=D2 + 2), "16-byte alignment"),
        "ld < 3 D": (d(qkv=od["qkv"][:, :, :3 * D2 - 4]), "below the columns"),
        "out_ld < D": (d(out_ld=D2 - 4), "below the columns"),
        "dense without a window": (d(context=-1), "needs a window"),
        "unknown form": (d(form=3), "unknown form"),
        "17 heads": (d(heads=17, qkv=np.zeros((2, 35, 3 * 17 * 64 + 4), F32), out_ld=17 * 64), "1..16"),
        "17 segments": (d(qkv=big, heads=1, t0=0, ct=4, out_ld=64), "1..16"),
        "T1 > 4096": (d(qkv=np.zeros((1, 4097, 3 * 64), F32), heads=1, t0=0, ct=4, out_ld=64), "T1 4097"),
        "rows > 4096": (d(qkv=np.zeros((2, 2100, 3 * 64), F32), heads=1, t0=0, ct=2100, out_ld=64), "the hook takes 4096"),
        "rag_pos0 + n > cap": (r(rag_pos0=arr(orr["rag_pos0"], 0, orr["k"].shape[2] - 69)), "the cache holds"),
        "rag_pos0 < 0": (r(rag_pos0=arr(orr["rag_pos0"], 1, -1)), "the cache holds"),
        "a bf16 cache in the dense layout": (d(kv_bf16=True), "the dense layout is f32"),
        "rag_off decreases": (r(rag_off=np.array([0, 60, 55, 108], np.int32)), "decreases at segment 1"),
        "rag_off does not start at 0": (r(rag_off=arr(orr["rag_off"], 0, 1)), "not from 0 to rows"),
        "rag_off does not end at rows": (r(rag_off=arr(orr["rag_off"], 3, 107)), "not from 0 to rows"),
        "ragged q_ld < D": (r(qkv=orr["qkv"][:, :D3 - 4]), "below the columns"),
        "ragged on the LDS form": (r(form=2), "dense operands only"),
        "cap > 4096": (r(k=np.zeros((3, 3, 4097, 64), F32), v=np.zeros((3, 3, 4097, 64), F32)), "outside 1..4096"),
    }
    rt.launch_counts(True)
    try:
        for what, (call, msg) in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                call()
            assert e.value.code == rt.PTTS_EINVAL and "ptts_debug_attn_window" in str(e.value) and msg in str(e.value), (what, str(e.value))
            assert rt.launch_counts(True) == {}, what
    finally:
        rt.launch_counts(False)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def run(pkg, c, form):
    o = operands(c)
    if c["kind"] == "dense":
        return pkg.runtime.debug_attn_window(o["qkv"], heads=c["heads"], context=c["ctx"], form=form, t0=c["t0"], ct=c["ct"], out_ld=o["D"] + 4)
    return pkg.runtime.debug_attn_window(o["qkv"], heads=c["heads"], context=c["ctx"], form=form, k=o["k"], v=o["v"], rag_off=o["rag_off"], rag_pos0=o["rag_pos0"],
                                         kv_bf16=c["fmt"] == "bf16", out_ld=o["D"] + 4)


def check(pkg, c, form):
    """one launch, every property: the kernel the dispatch (or the form) names and exactly one launch in the census; finite and within the bound on every owned
    element (recorded through _parity.record: profiles/attn_window_parity.txt is one run's summary); every byte outside them still 0xff; a second run with
    the same bits."""
    D = c["heads"] * 64
    name = f"k_attn_window form{form} {cid(c)}"
    census = "k_attn_window" if c["kind"] == "dense" else "k_attn_window<ragged>"
    r = run(pkg, c, form)
    assert r["kernel"] == (census if form == 0 else FORM_KERNEL[form]), (name, r["kernel"])
    assert r["launched"] == {census: 1}, (name, r["launched"])
    if form == 0:
        assert pkg.runtime.last_attention_kernel() == census
    out = r["out"]
    assert out.shape == (n_rows(c), D + 4)
    assert (out[:, D:].view(np.uint32) == 0xFFFFFFFF).all(), name + ": the padding columns of the output were written"
    want, bnd = reference(c)
    got = out[:, :D]
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} non-finite outputs, first at {np.argwhere(~np.isfinite(got))[0]}"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bnd).max())
    record(name, float(err.max()), worst, float(np.abs(want).max()), (CEIL, 0))   # (max_rel slot: error / bound)
    print(f"{name}: max abs {float(err.max()):.3e}, error / bound {worst:.3f}")
    assert worst <= 1.0, (name, float(err.max()), worst, np.unravel_index(np.argmax(err / bnd), err.shape))
    again = run(pkg, c, form)["out"]
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)), name + ": a second run gave other bits"


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", DENSE_CASES, ids=cid)
def test_dense_every_form(pkg, c, form):
    """the decoder's and the encoder's layout: through the dispatch (which must name k_attn_window), k_attn_window<false, false> and k_attn_window_lds<4>"""
    check(pkg, c, form)


@gpu
@pytest.mark.parametrize("c", RAGGED_CASES, ids=cid)
def test_ragged_through_the_dispatch(pkg, c):
    """the prompt prefill's layout in both cache formats: the dispatch must name k_attn_window<ragged>"""
    check(pkg, c, 0)


@gpu
@pytest.mark.parametrize("c", NAN_CASES, ids=cid)
def test_canonical_nan_outside_the_launch(pkg, c):
    """the same poison as canonical NaNs (what a voice state's padding holds) instead of 0xff bytes"""
    for form in case_forms(c):
        check(pkg, c, form)


@gpu
def test_forced_forms_name_their_instance(pkg):
    """form 1 on ragged operands is the instance of the cache format; the forms differ by rounding only (different tile alignment: no bit equality asked)"""
    for fmt, inst in (("f32", "k_attn_window<false,true>"), ("bf16", "k_attn_window<true,true>")):
        c = CASE_BY_ID[cid(ragged((70, 5, 33), (0, 0, 9), fmt))]
        r0, r1 = run(pkg, c, 0), run(pkg, c, 1)
        assert r1["kernel"] == inst and r1["launched"] == {"k_attn_window<ragged>": 1}
        assert np.array_equal(r0["out"].view(np.uint32), r1["out"].view(np.uint32))   # (the same instance either way)
    c = CASE_BY_ID[cid(dense(250, 300, 129))]
    a, b = run(pkg, c, 1)["out"][:, :-4], run(pkg, c, 2)["out"][:, :-4]
    bnd = reference(c)[1]
    assert (np.abs(a.astype(np.float64) - b) <= 2 * bnd).all()
