"""The two kernels of csrc/ffn_fused.hip stand-alone, value by value, against f64 numpy on host operands the test owns.

  k_mimi_ffn     x += ls * linear2(gelu(linear1(LayerNorm2(x))))        in place, x [rows][512]        (mimi.go:245-285, 351-358, 506-525)
  k_mimi_rowlin  y = rope(LayerNorm1(x) W^T)                              y [rows][N]                    (mimi.go:245-441, rope.go:81-105)

The hook (ptts_debug_mimi_fused) runs ONE launch on the caller's buffers with kernels.h' RowMaps, packs the f32 row-major weights with the loader's own image
packers (csrc/model.h pack_ffn_image / pack_w1_image), returns the whole x buffer (kind 0) or the whole y buffer, filled with 0xff bytes first (kind 1), and checks
every row of both maps and every table position against the buffers before anything is uploaded (the kernels clamp rows past M and bound nothing else).

Reference: f64 numpy -- biased-variance LayerNorm, erf GELU, interleaved-pair RoPE at 64-wide heads; weights rounded to bf16 in the test.

Bounds (TOL = 3e-5 and the floor 1e-6 of tests/test_gpu_tall.py and tests/test_gpu_many_row_gemm.py: the bf16 hi + lo split of an activation is exact to 2^-17):
  rowlin      TOL sum_k |y_k w_k|, carried through the rotation as test_gpu_many_row_gemm.py carries it (|cos| b_x + |sin| b_y + 2^-23 (|x cos| + |y sin|)), + 1e-6
  FFN hidden  b_h = 1.2 TOL sum_k |y_k w1_jk| + G                                   (|gelu'| <= 1.13)
  FFN output  |ls| (TOL sum_j |g_j w2_oj| + sum_j b_h[j] |w2_oj|) + 2^-23 |want| + 1e-6
G, the budget of the kernel's GELU (erf by Abramowitz-Stegun 7.1.26), is TWICE the worst |gelu_AS - gelu| that the textbook formula gives in f32 numpy against
f64 erf on 2 10^6 points of [-8, 8] (test_gelu_budget; the factor 2 is for the 1-ulp hardware rcp / exp2 in place of numpy's correctly rounded ones).

The composite FFN bound with dense random weights is a worst case over two products -- a dropped lo half reaches only 0.3 .. 3 x of it -- so the precision claim
rests on the one-hot cases: W1 = W2 = I (F = 512: out = x + ls gelu(LN(x)), bound |ls| (TOL |g| + 1.2 TOL |y| + G) + ...) and four stacked identities (F = 2048),
where the kernels' arithmetic sits near 0.2 of the bound and either dropped lo half far above it (tried on the MI355X: with the lo-half matrix instructions
of ffn_fused.hip compiled out -- PTTS_ABLATE_LO, a measurement build -- all seven identity and one-hot cases fail, at 108 to 127 x the bound).
test_emulation_stays_within_half_the_bound (no GPU) holds a numpy emulation of the kernels' arithmetic to HALF the bound on every case;
test_planted_defects_exceed_the_bound plants the defects such kernels get into it.

LayerNorm of a constant row: the f64 reference gives ln_b exactly; the kernel's two-pass f32 form does too only if its sum of 512 equal values is exact, because
1 / sqrt(eps) = 316 multiplies whatever the mean's rounding leaves.  The constant is therefore a power of two (every partial sum is exact).

Observed error / bound per case on the MI355X: profiles/mimi_fused_parity_observed.json."""
import functools
import math
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_bits, bf16_round, bits, check_bound, split
from _parity import record

TOL = 3e-5
FLOOR = 1e-6
RND = 2.0 ** -23
F32 = np.float32
D = 512
EPS = 1e-5
MS = (1, 15, 16, 17, 63, 64, 65, 130)
FS = (32, 64, 96, 512, 2048)     # 32, 64: one and two chunks (the pipeline's degenerate tails); 96: an odd count
NS = (64, 128, 1536)             # 64: two chunks (the three-slot pipeline's shortest run)
BIG_M, BIG_DISTINCT = 16449, 67  # 257 full blocks + one row: more blocks than the 256 CUs hold at one block per CU
FFN, ROWLIN = 0, 1

try:
    from scipy.special import erf as erf64
except ImportError:   # pragma: no cover
    def erf64(v):
        return np.vectorize(math.erf, otypes=[np.float64])(v)


# ------------------------------------------------------------------------------------------------ number formats, functions
def gelu64(v):
    return 0.5 * v * (1.0 + erf64(v / math.sqrt(2.0)))


def gelu_as32(x):
    """ffn_fused.hip ff_gelu in f32 numpy: erf by Abramowitz-Stegun 7.1.26, every operation rounded to f32 (no fused multiply-add), exp2 correctly rounded."""
    x = np.asarray(x, F32)
    ax = np.abs(x)
    t = F32(1.0) / (F32(0.3275911) * F32(0.70710678118654752) * ax + F32(1.0))
    p = F32(1.061405429) * t + F32(-1.453152027)
    p = p * t + F32(1.421413741)
    p = p * t + F32(-0.284496736)
    p = p * t + F32(0.254829592)
    p = p * t
    e = np.exp2((F32(-1.4426950408889634) * F32(0.5) * x * x).astype(np.float64)).astype(F32)
    erfa = F32(1.0) - p * e
    return F32(0.5) * x * (F32(1.0) + np.copysign(erfa, x))


@functools.lru_cache(maxsize=None)
def gelu_as_worst():
    """(worst |gelu_AS in f32 - gelu in f64| on 2 10^6 + 1 points of [-8, 8], where)."""
    x = np.linspace(-8.0, 8.0, 2_000_001).astype(F32)
    err = np.abs(gelu_as32(x).astype(np.float64) - gelu64(x.astype(np.float64)))
    i = int(err.argmax())
    return float(err[i]), float(x[i])


def G():
    return 2.0 * gelu_as_worst()[0]


def ln64(x, w, b, eps=EPS):
    x = x.astype(np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=1, keepdims=True) + eps) * w.astype(np.float64) + b.astype(np.float64)


def ln32(x, w, b, eps=EPS):
    """ff_rows_layernorm: two passes in f32."""
    x = np.asarray(x, F32)
    mean = x.sum(axis=1, dtype=F32) * F32(1.0 / 512)
    d = x - mean[:, None]
    var = (d * d).sum(axis=1, dtype=F32)
    rstd = F32(1.0) / np.sqrt(var * F32(1.0 / 512) + F32(eps))
    return d * rstd[:, None] * w + b


def rope_tables(n_pos):
    """interleaved-pair tables [n_pos][32] in f32 for 64-wide heads (rope.go:81-105: theta_j = 10000^(-2 j / 64))."""
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * (10000.0 ** (-2.0 * np.arange(32) / 64))[None, :]
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


# ------------------------------------------------------------------------------------------------ cases
def ffn_case(M, F, ls=True, xl=("flat", 0), data="normal", w="rand"):
    """ls: True (given) or None (null); xl: x's RowMap -- ("flat", pad): ld = 512 + pad, ("seg", S, H, pad): segments of S rows behind H history rows
    each; data: "normal", "edges" (the LayerNorm edge rows) or "sweep" (pre-activations over [-8, 8] through identity weights); w: "rand" or "eye"."""
    return dict(kind=FFN, M=M, F=F, ls=ls, xl=xl, data=data, w=w)


def rowlin_case(M, N, rope=None, xl=("flat", 0), yl=("flat", 0), w="rand", data="normal"):
    """rope: None or (rope_cols, pos0, rows_per_seg); yl: y's RowMap, as xl with the width N; w: "rand" or "onehot"."""
    return dict(kind=ROWLIN, M=M, N=N, rope=rope, xl=xl, yl=yl, w=w, data=data)


def _lay(lay):
    return "" if lay == ("flat", 0) else "_".join(str(v) for v in lay)


def cid(c):
    if c["kind"] == FFN:
        s = f"k_mimi_ffn-M{c['M']}-F{c['F']}-" + ("ls" if c["ls"] else "nols")
    else:
        s = f"k_mimi_rowlin-M{c['M']}-N{c['N']}-" + ("norope" if c["rope"] is None else "rope{}p{}s{}".format(*c["rope"]))
        s += ("-y" + _lay(c["yl"])) if _lay(c["yl"]) else ""
    s += ("-x" + _lay(c["xl"])) if _lay(c["xl"]) else ""
    return s + ("" if c["data"] == "normal" else "-" + c["data"]) + ("" if c["w"] == "rand" else "-" + c["w"])


def census_name(c):
    return "k_mimi_ffn" if c["kind"] == FFN else "k_mimi_rowlin+rope" if c["rope"] is not None else "k_mimi_rowlin"


def rowmap(lay, M, width):
    """(ld, rows_per_batch, batch_stride, off, elems)."""
    if lay[0] == "flat":
        ld = width + lay[1]
        return ld, 0, 0, 0, M * ld
    _, S, H, pad = lay
    ld = width + pad
    return ld, S, (H + S) * ld, H * ld, -(-M // S) * (H + S) * ld


def row_offsets(m, M):
    ld, rpb, bs, off = m[:4]
    r = np.arange(M, dtype=np.int64)
    return off + ((r // rpb) * bs + (r % rpb) * ld if rpb else r * ld)


X_FLAT, X_SEG, X_SEG_PAD = ("flat", 64), ("seg", 24, 3, 0), ("seg", 24, 3, 64)   # 24-row segments: a wave's 16 rows straddle a segment
FFN_GRID = [ffn_case(M, F, ls=True if (i + j) % 2 == 0 else None) for i, M in enumerate(MS) for j, F in enumerate(FS)]
FFN_MAPS = [ffn_case(65, 96, xl=X_FLAT), ffn_case(130, 512, xl=X_SEG), ffn_case(130, 64, xl=X_SEG_PAD, ls=None), ffn_case(17, 2048, xl=X_SEG_PAD)]
FFN_EDGES = [ffn_case(17, 512, data="edges"), ffn_case(17, 96, data="edges", ls=None), ffn_case(65, 2048, data="edges")]
FFN_ONEHOT = [ffn_case(130, 512, w="eye"), ffn_case(130, 2048, w="eye"), ffn_case(65, 512, w="eye", ls=None), ffn_case(65, 512, w="eye", data="sweep")]
ROPE_POS = [(p0, rps) for p0 in (0, 7) for rps in (0, 5, 50, 64)]


def _rope_cols(N):
    return sorted({0, 64, N - 64, N})


# base grid: every M x N, without RoPE and with it (the variants in turn)
_VAR = [None] + [(cols, p0, rps) for cols in ("0", "64", "N-64", "N") for (p0, rps) in ROPE_POS]
ROWLIN_GRID = []
for _i, _M in enumerate(MS):
    for _j, _N in enumerate(NS):
        _v = _VAR[(5 * _i + 7 * _j) % len(_VAR)] if (_i + _j) % 2 else None
        ROWLIN_GRID.append(rowlin_case(_M, _N, rope=None if _v is None else ({"0": 0, "64": 64, "N-64": _N - 64, "N": _N}[_v[0]], _v[1], _v[2])))
# every rope_cols x pos0 x rows_per_seg at N = 128; every rope_cols at N = 64 and 1536 with the positions in turn
ROWLIN_ROPE = [rowlin_case(70, 128, rope=(cols, p0, rps)) for cols in _rope_cols(128) for (p0, rps) in ROPE_POS] + \
              [rowlin_case(100, N, rope=(cols, *ROPE_POS[(3 * i + 1) % 8])) for N in (64, 1536) for i, cols in enumerate(_rope_cols(N))]
Y_FLAT, Y_SEG = ("flat", 32), ("seg", 24, 2, 32)
ROWLIN_MAPS = [rowlin_case(65, 64, rope=(64, 7, 5), xl=X_FLAT, yl=Y_FLAT), rowlin_case(130, 128, rope=(64, 0, 50), xl=X_SEG_PAD, yl=Y_SEG),
               rowlin_case(130, 1536, rope=(1024, 7, 64), xl=X_SEG, yl=Y_SEG), rowlin_case(17, 128, xl=X_SEG_PAD, yl=Y_FLAT)]
ROWLIN_ONEHOT = [rowlin_case(130, 1536, w="onehot"), rowlin_case(65, 64, w="onehot", rope=(64, 7, 50)), rowlin_case(17, 128, w="onehot", data="sweep")]
GROUPS = {"ffn-grid": FFN_GRID, "ffn-maps": FFN_MAPS, "ffn-edges": FFN_EDGES, "ffn-onehot": FFN_ONEHOT, "rowlin-grid": ROWLIN_GRID, "rowlin-rope": ROWLIN_ROPE,
          "rowlin-maps": ROWLIN_MAPS, "rowlin-onehot": ROWLIN_ONEHOT}
# (rows_per_seg = the number of distinct rows: every repeat of a row sits at its first occurrence's position)
BIG_FFN, BIG_ROWLIN = ffn_case(BIG_M, 96), rowlin_case(BIG_M, 128, rope=(64, 7, BIG_DISTINCT))


def test_case_lists_cover_the_axes():
    for name, g in GROUPS.items():
        assert len({cid(c) for c in g}) == len(g), name
    assert {(c["M"], c["F"]) for c in FFN_GRID} == {(M, F) for M in MS for F in FS}
    for F in FS:   # every hidden width with and without a layer scale
        assert {c["ls"] for c in FFN_GRID if c["F"] == F} == {True, None}
    assert {c["xl"][0] for c in FFN_MAPS} == {"flat", "seg"} and all(c["xl"][-1] == 64 for c in FFN_MAPS if c["xl"][0] == "flat")
    assert any(c["xl"][0] == "seg" and c["xl"][1] == 24 and c["M"] > 24 for c in FFN_MAPS)
    assert {(c["F"], c["w"]) for c in FFN_ONEHOT} >= {(512, "eye"), (2048, "eye")} and any(c["data"] == "sweep" for c in FFN_ONEHOT)
    assert {(c["M"], c["N"]) for c in ROWLIN_GRID} == {(M, N) for M in MS for N in NS}
    rl = ROWLIN_GRID + ROWLIN_ROPE + ROWLIN_MAPS + ROWLIN_ONEHOT
    assert any(c["rope"] is None for c in rl)
    for N in NS:
        assert {c["rope"][0] for c in rl if c["N"] == N and c["rope"]} >= set(_rope_cols(N)), N
    assert {c["rope"][1:] for c in ROWLIN_ROPE if c["N"] == 128} == set(ROPE_POS)
    assert all(c["yl"][-1] == 32 for c in ROWLIN_MAPS) and {c["yl"][0] for c in ROWLIN_MAPS} == {"flat", "seg"}
    assert BIG_M == 257 * 64 + 1
    assert {census_name(c) for g in GROUPS.values() for c in g} == {"k_mimi_ffn", "k_mimi_rowlin", "k_mimi_rowlin+rope"}


# ------------------------------------------------------------------------------------------------ operands
def make_rows(c, rng, M):
    scale = (10.0 ** rng.uniform(-1.0, 1.0, (M, 1))).astype(F32)
    rows = (rng.standard_normal((M, D), dtype=F32) + F32(0.2) * rng.standard_normal((M, 1), dtype=F32)) * scale
    if c["data"] == "edges" and M >= 6:
        rows[0] = 2.0                                                  # variance 0 (a power of two: see the module's docstring)
        rows[1] = rng.standard_normal(D, dtype=F32) + F32(8.0)        # mean 8 and 50 at unit spread
        rows[2] = rng.standard_normal(D, dtype=F32) + F32(50.0)
        rows[3] = rng.standard_normal(D, dtype=F32) * F32(1e-3)       # below sqrt(eps)
        rows[4] = rng.standard_normal(D, dtype=F32) * F32(1e3)
        rows[5] = 0.0
    return rows


def operands(c, M=None):
    """M: build only the first M rows' worth of a taller case (the many-block cases repeat BIG_DISTINCT rows)."""
    rng = np.random.default_rng(zlib.crc32(cid(c).encode()))
    M = c["M"] if M is None else M
    xm = rowmap(c["xl"], M, D)
    xbuf = rng.standard_normal(xm[4], dtype=F32)   # history rows and padding hold values too
    xidx = row_offsets(xm, M)
    X = make_rows(c, rng, M)
    xbuf[xidx[:, None] + np.arange(D)[None, :]] = X
    o = {"M": M, "xbuf": xbuf, "xmap": xm[:4], "xidx": xidx, "X": X}
    if c["data"] == "sweep":   # y = 0.35 n + b with b spread over [-6.5, 6.5]: identity weights hand it to the GELU as it is
        o["ln_w"], o["ln_b"] = np.full(D, 0.35, F32), rng.permutation(np.linspace(-6.5, 6.5, D)).astype(F32)
    else:
        o["ln_w"], o["ln_b"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(F32), (0.1 * rng.standard_normal(D)).astype(F32)
    if c["kind"] == FFN:
        F = c["F"]
        if c["w"] == "eye":
            assert F % D == 0
            o["W1"], o["W2"] = np.tile(np.eye(D, dtype=F32), (F // D, 1)), np.tile(np.eye(D, dtype=F32), (1, F // D))
        else:
            o["W1"], o["W2"] = bf16_round(rng.standard_normal((F, D)) / math.sqrt(D)), bf16_round(rng.standard_normal((D, F)) / math.sqrt(F))
        ls = (0.5 * rng.standard_normal(D)).astype(F32)
        ls[::37] = 0.0
        ls[5] = -2.0
        o["ls"] = ls if c["ls"] else None
    else:
        N = c["N"]
        if c["w"] == "onehot":
            o["perm"] = rng.integers(0, D, N)
            W = np.zeros((N, D), F32)
            W[np.arange(N), o["perm"]] = 1.0
            o["W1"] = W
        else:
            o["W1"] = bf16_round(rng.standard_normal((N, D)) / math.sqrt(D))
        ym = rowmap(c["yl"], M, N)
        o["ymap"], o["y_elems"], o["yidx"] = ym[:4], ym[4], row_offsets(ym, M)
        if c["rope"] is not None:
            cols, p0, rps = c["rope"]
            o["pos"] = p0 + (np.arange(M) % rps if rps else np.arange(M))
            o["cos"], o["sin"] = rope_tables(int(o["pos"].max()) + 1)   # tables of exactly the length needed
    return o


# ------------------------------------------------------------------------------------------------ the operations: f64 with bounds, and the kernels' arithmetic
def rotate(pre, cos_t, sin_t, pos, cols, dt, sin_sign=1.0):
    """interleaved-pair RoPE (64-wide heads) of the first cols columns, every product and sum rounded in dt.  Returns (out, cos, sin as used)."""
    p = np.arange(cols // 2)
    cs, sn = cos_t[pos][:, p % 32].astype(dt), (sin_t[pos][:, p % 32] * F32(sin_sign)).astype(dt)
    out = pre.copy()
    x0, x1 = pre[:, 0:cols:2], pre[:, 1:cols:2]
    out[:, 0:cols:2] = x0 * cs - x1 * sn
    out[:, 1:cols:2] = x0 * sn + x1 * cs
    return out, cs, sn


def carry(b, absx, cs, sn, cols):
    """the pairs' pre-rotation bounds b carried through the rotation, plus the f32 rounding of two products and one sum."""
    cs, sn = np.abs(cs), np.abs(sn)
    be, bo, xe, xo = b[:, 0:cols:2], b[:, 1:cols:2], absx[:, 0:cols:2], absx[:, 1:cols:2]
    b = b.copy()
    b[:, 0:cols:2] = cs * be + sn * bo + RND * (xe * cs + xo * sn)
    b[:, 1:cols:2] = sn * be + cs * bo + RND * (xe * sn + xo * cs)
    return b


def ref_ffn(o):
    x = o["X"].astype(np.float64)
    y = ln64(o["X"], o["ln_w"], o["ln_b"])
    W1, W2 = o["W1"].astype(np.float64), o["W2"].astype(np.float64)
    g = gelu64(y @ W1.T)
    ls = np.ones(D) if o["ls"] is None else o["ls"].astype(np.float64)
    want = x + ls * (g @ W2.T)
    b_h = 1.2 * TOL * (np.abs(y) @ np.abs(W1).T) + G()
    bound = np.abs(ls) * (TOL * (np.abs(g) @ np.abs(W2).T) + b_h @ np.abs(W2).T) + RND * np.abs(want) + FLOOR
    return want, bound


def ref_rowlin(c, o):
    y = ln64(o["X"], o["ln_w"], o["ln_b"])
    W = o["W1"].astype(np.float64)
    pre = y @ W.T
    b = TOL * (np.abs(y) @ np.abs(W).T)
    if c["rope"] is not None and c["rope"][0]:
        cols = c["rope"][0]
        x = np.abs(pre)
        pre, cs, sn = rotate(pre, o["cos"], o["sin"], o["pos"], cols, np.float64)
        b = carry(b, x, cs, sn, cols)
    return pre, b + FLOOR


def reference(c, o):
    return ref_ffn(o) if c["kind"] == FFN else ref_rowlin(c, o)


def product(ah, al, W, lo=True):
    """sum over the 32-deep steps: bf16 x bf16 products are exact, sums in f32, the hi product of a step and then its lo product."""
    acc = np.zeros((ah.shape[0], W.shape[0]), F32)
    for k in range(0, ah.shape[1], 32):
        acc = acc + ah[:, k:k + 32] @ W[:, k:k + 32].T
        if lo:
            acc = acc + al[:, k:k + 32] @ W[:, k:k + 32].T
    return acc


def emulate(c, o, defect=None):
    """The kernels' arithmetic in f32 numpy: two-pass LayerNorm, bf16 hi + lo split (split2), exact bf16 products summed in f32, A&S GELU, unfused epilogue --
    optionally with a planted defect."""
    y = ln32(o["X"], o["ln_w"], o["ln_b"])
    yh, yl = split(y)
    W1 = o["W1"]
    if defect == "swap_k":   # two k positions of a W1 piece swapped in the image
        W1 = W1.copy()
        W1[:, [5, 6]] = W1[:, [6, 5]]
    if c["kind"] == ROWLIN:
        pre = product(yh, yl, W1, lo=defect != "lo_rowlin")
        if c["rope"] is None:
            return pre.astype(np.float64)
        cols = c["rope"][0] + {"rope_far": 32, "rope_short": -32}.get(defect, 0)
        assert 0 <= cols <= c["N"]
        return rotate(pre, o["cos"], o["sin"], o["pos"], cols, F32, sin_sign=-1.0 if defect == "sin_sign" else 1.0)[0].astype(np.float64)
    W2, nch = o["W2"], c["F"] // 32
    if defect == "stale_slot":   # the slots of chunk nch - 2 still (or already) hold the last chunk's images
        assert nch >= 2
        unit = np.arange(c["F"])
        unit[32 * (nch - 2):32 * (nch - 1)] = unit[32 * (nch - 1):]
        W1, W2 = W1[unit], W2[:, unit]
    g = gelu_as32(product(yh, yl, W1, lo=defect != "lo1"))
    gh, gl = split(g)
    acc = product(gh, gl, W2, lo=defect != "lo2")
    ls = np.ones(D, F32) if o["ls"] is None else o["ls"]
    return (o["X"] + ls * acc).astype(np.float64)


def ratio(got, want, bound):
    return float((np.abs(np.asarray(got, np.float64) - want) / bound).max())


# ------------------------------------------------------------------------------------------------ no GPU: G, the image layout, the emulation, planted defects
def test_gelu_budget():
    """G = 2 x the worst error of the textbook A&S 7.1.26 GELU in f32 on [-8, 8].  A&S state |erf error| <= 1.5e-7, so |gelu error| <= 0.5 * 8 * 1.5e-7 = 6e-7
    plus f32 rounding: the measured worst must lie between the two."""
    worst, at = gelu_as_worst()
    record("mimi_fused G", worst, 0.0, G(), (G(), 0))
    print(f"A&S GELU in f32: worst |error| {worst:.3e} at x = {at:.4g}; G = {G():.3e}")
    assert 1.5e-7 <= worst <= 8e-7


def w1_image_ref(W):
    """the layout comment of csrc/model.cpp, restated: [chunk c][k pair j (8)][unit h (32)][position (8)][8]."""
    n = W.shape[0]
    bits = bf16_bits(W)
    img = np.zeros((n // 32, 8, 32, 8, 8), np.uint16)
    for j in range(8):
        for h in range(32):
            for sg in range(2):
                for q in range(4):
                    pos = (4 * sg + q) ^ ((h >> 1) & 7)
                    k0 = 32 * (2 * j + sg) + 4 * q
                    img[:, j, h, pos, 0:4] = bits[h::32, k0:k0 + 4]
                    img[:, j, h, pos, 4:8] = bits[h::32, k0 + 16:k0 + 20]
    return img.reshape(n // 32, 16384)


def w2_image_ref(W2):
    """[chunk c][output o (512)][position (4)][8]."""
    n = W2.shape[1]
    bits = bf16_bits(W2)
    img = np.zeros((n // 32, D, 4, 8), np.uint16)
    for c in range(n // 32):
        for q in range(4):
            for par in range(2):
                pos = q ^ (3 * par)
                o = np.arange(D)[((np.arange(D) >> 3) & 1) == par]
                img[c, o, pos, 0:4] = bits[o, 32 * c + 4 * q:32 * c + 4 * q + 4]
                img[c, o, pos, 4:8] = bits[o, 32 * c + 16 + 4 * q:32 * c + 16 + 4 * q + 4]
    return img.reshape(n // 32, 16384)


def test_weight_images_follow_the_layout(pkg):
    """The packers the loader and the hook share (csrc/model.h pack_w1_image, pack_ffn_image) against a numpy restatement of the layout the fragment reads of
    ffn_fused.hip assume.  No GPU."""
    rng = np.random.default_rng(5)
    W1, W2 = rng.standard_normal((96, D), dtype=F32), rng.standard_normal((D, 96), dtype=F32)
    got1 = pkg.runtime.debug_mimi_pack(ROWLIN, W1)
    assert got1.shape == (3, 16384) and np.array_equal(got1, w1_image_ref(W1))
    got = pkg.runtime.debug_mimi_pack(FFN, W1, W2)
    assert got.shape == (3, 2, 16384)
    assert np.array_equal(got[:, 0], w1_image_ref(W1)) and np.array_equal(got[:, 1], w2_image_ref(W2))
    # every weight appears exactly once per image
    assert np.array_equal(np.sort(got[:, 0].reshape(-1)), np.sort(bf16_bits(W1).reshape(-1))) and np.array_equal(np.sort(got[:, 1].reshape(-1)), np.sort(bf16_bits(W2).reshape(-1)))
    with pytest.raises(pkg.PttsError):
        pkg.runtime.debug_mimi_pack(ROWLIN, W1[:40])


def test_sweep_covers_the_gelu_range():
    """the sweep cases hand the GELU pre-activations all over [-8, 8], the range G was measured on."""
    for c in (FFN_ONEHOT[3], ROWLIN_ONEHOT[2]):
        assert c["data"] == "sweep"
        o = operands(c)
        pre = ln64(o["X"], o["ln_w"], o["ln_b"])
        assert pre.min() < -7.0 and pre.max() > 7.0 and np.abs(pre).max() <= 8.0 and (np.histogram(pre, bins=28, range=(-7, 7))[0] > 0).all(), cid(c)


EMULATED = {}


def emulated_ratio(c):
    key = cid(c)
    if key not in EMULATED:
        o = operands(c)
        want, bound = reference(c, o)
        EMULATED[key] = ratio(emulate(c, o), want, bound)
    return EMULATED[key]


@pytest.mark.parametrize("group", list(GROUPS) + ["many-blocks"])
def test_emulation_stays_within_half_the_bound(group):
    """The kernels' arithmetic, emulated in numpy, stays within HALF the bound the GPU tests use, on every case of this file (the many-block cases: their
    distinct rows)."""
    worst = 0.0
    for c in GROUPS.get(group) or [dict(BIG_FFN, M=BIG_DISTINCT), dict(BIG_ROWLIN, M=BIG_DISTINCT)]:
        r = emulated_ratio(c)
        worst = max(worst, r)
        print(f"  {cid(c)}: emulated error / bound {r:.3f}")
        assert r <= 0.5, (cid(c), r)
    print(f"{group}: emulated error / bound, worst {worst:.3f}")


# each planted defect with the cases it must show on, at >= 2 x the bound on at least one
DEFECTS = {
    "lo1": FFN_ONEHOT[:2],                       # lo half dropped in the first product
    "lo2": FFN_ONEHOT[:2],                       # ... in the second
    "lo_rowlin": [ROWLIN_GRID[5], ROWLIN_ONEHOT[0]],
    "swap_k": [FFN_GRID[2], ROWLIN_GRID[4]],
    "stale_slot": [c for c in FFN_GRID if c["M"] == 17 and c["F"] >= 64],
    "rope_far": [c for c in ROWLIN_ROPE if c["rope"][0] < c["N"]][:4],
    "rope_short": [c for c in ROWLIN_ROPE if c["rope"][0] > 0][:4],
    "sin_sign": [c for c in ROWLIN_ROPE if c["rope"][0] > 0][:4],
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_exceed_the_bound(defect):
    worst = {}
    for c in DEFECTS[defect]:
        o = operands(c)
        want, bound = reference(c, o)
        assert emulated_ratio(c) <= 0.5
        worst[cid(c)] = ratio(emulate(c, o, defect), want, bound)
    print(f"{defect}: error / bound {worst}")
    assert max(worst.values()) >= 2.0, (defect, worst)
    if defect in ("lo1", "lo2"):   # the one-hot cases carry the precision claim: BOTH show either dropped half, far above the bound
        assert min(worst.values()) >= 20.0 and all(emulated_ratio(c) <= 0.3 for c in DEFECTS[defect]), (defect, worst)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
FILL = np.uint32(0xFFFFFFFF)


def run(pkg, c, o, **over):
    """one launch of case c on operands o; asserts the census: exactly one launch, of the kernel the case names."""
    kw = dict(xmap=o["xmap"], ln_w=o["ln_w"], ln_b=o["ln_b"], w1=o["W1"], eps=EPS)
    if c["kind"] == FFN:
        kw.update(w2=o["W2"], ls=o["ls"])
    else:
        kw.update(y_elems=o["y_elems"], ymap=o["ymap"])
        if c["rope"] is not None:
            kw.update(rope=(o["cos"], o["sin"]), rope_cols=c["rope"][0], pos0=c["rope"][1], rows_per_seg=c["rope"][2])
    kw.update(over)
    xbuf = kw.pop("xbuf", o["xbuf"])
    r = pkg.runtime.debug_mimi_fused(c["kind"], xbuf, o["M"], **kw)
    want = "k_mimi_ffn" if c["kind"] == FFN else "k_mimi_rowlin+rope" if kw.get("rope") is not None else "k_mimi_rowlin"
    assert r["launched"] == {want: 1}, (cid(c), r["launched"])
    return r["out"]


def rows_of(c, o, buf):
    """[M][width] of a returned buffer, and a mask of the buffer's elements outside the map."""
    idx = (o["xidx"] if c["kind"] == FFN else o["yidx"])[:, None] + np.arange(D if c["kind"] == FFN else c["N"])[None, :]
    outside = np.ones(buf.size, bool)
    outside[idx.reshape(-1)] = False
    return buf[idx], outside


def check(name, got, want, bound):
    check_bound("mimi_fused " + name, got, want, bound, TOL)


def check_case(pkg, c):
    """runs case c: the census, every value against the f64 reference, and every element outside the map -- the input's bits (in place) or the 0xff fill."""
    o = operands(c)
    want, bound = reference(c, o)
    out = run(pkg, c, o)
    got, outside = rows_of(c, o, out)
    if c["kind"] == FFN:
        assert np.array_equal(bits(out[outside]), bits(o["xbuf"][outside])), cid(c) + ": changed outside the rows"
    else:
        assert (bits(out[outside]) == FILL).all(), cid(c) + ": written outside the rows"
    check(cid(c), got, want, bound)
    return o, out, got


@gpu
@pytest.mark.parametrize("c", FFN_GRID + FFN_MAPS + FFN_EDGES + FFN_ONEHOT, ids=cid)
def test_ffn(pkg, c):
    """k_mimi_ffn: every M x F with and without a layer scale; strided and segmented rows, in place; the LayerNorm edge rows; identity weights (the cases that
    hold the lo halves of both products) and the pre-activation sweep over [-8, 8]."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", [ffn_case(M, F, ls=None) for M, F in ((17, 32), (130, 64), (17, 96), (65, 512), (130, 2048))], ids=cid)
def test_ffn_no_layer_scale_is_a_scale_of_ones(pkg, c):
    o = operands(c)
    assert o["ls"] is None
    assert np.array_equal(bits(run(pkg, c, o)), bits(run(pkg, c, o, ls=np.ones(D, F32))))


@gpu
@pytest.mark.parametrize("c", ROWLIN_GRID + ROWLIN_ROPE + ROWLIN_MAPS, ids=cid)
def test_rowlin(pkg, c):
    """k_mimi_rowlin: every M x N; RoPE off, and on over 0, 64, N - 64 and N columns at every position form with tables of exactly the length needed; strided and
    segmented input and output rows, the padding still 0xff."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", ROWLIN_ONEHOT, ids=cid)
def test_rowlin_one_hot_weights(pkg, c):
    """in_proj rows = one-hot: the product hands LN(x) through, column n from column perm[n], exact to the hi + lo split (2^-17)."""
    o, _, got = check_case(pkg, c)
    y = ln64(o["X"], o["ln_w"], o["ln_b"])[:, o["perm"]]
    lim = 2.0 ** -17 * np.abs(y)
    if c["rope"] is not None:
        absy = np.abs(y)
        y, cs, sn = rotate(y, o["cos"], o["sin"], o["pos"], c["rope"][0], np.float64)
        lim = carry(lim, absy, cs, sn, c["rope"][0])
    r = ratio(got, y, lim + FLOOR)
    print(f"{cid(c)}: error / (2^-17 |LN(x)| + 1e-6) {r:.3f}")
    assert r <= 1.0, (cid(c), r)


@gpu
@pytest.mark.parametrize("c", [c for c in ROWLIN_ROPE + ROWLIN_MAPS + ROWLIN_GRID if c["rope"] is not None], ids=cid)
def test_rowlin_rotation_is_the_f32_rotation_of_the_unrotated_launch(pkg, c):
    """The rotated launch equals, bit for bit, the numpy-f32 rotation of the same launch without tables: the kernel rounds the two products and the sum one by
    one (contraction off), and a rotation that reads a wrong value in any lane shows at any tolerance."""
    o = operands(c)
    plain, _ = rows_of(c, o, run(pkg, c, o, rope=None))
    got, _ = rows_of(c, o, run(pkg, c, o))
    want = rotate(plain, o["cos"], o["sin"], o["pos"], c["rope"][0], F32)[0]
    same = bits(got) == bits(want)
    assert same.all(), (cid(c), np.argwhere(~same)[:8].tolist())


def _with_rows(o, X):
    """x's buffer with other rows inside the same map."""
    xb = o["xbuf"].copy()
    xb[o["xidx"][:, None] + np.arange(D)[None, :]] = X
    return xb


@gpu
@pytest.mark.parametrize("c", [ffn_case(130, 96, xl=X_SEG_PAD), ffn_case(130, 2048), rowlin_case(130, 128, rope=(64, 7, 1), yl=Y_SEG), rowlin_case(130, 1536)], ids=cid)
def test_rows_are_independent(pkg, c):
    """bit for bit: permuting the input rows permutes the output rows; row 0 of a one-row launch equals the same row at index 129 of 130; a row of NaN and a row
    with an Inf leave every other row alone and are themselves non-finite.  (With RoPE every row sits at position 7: rows_per_seg 1.)"""
    o = operands(c)
    base, _ = rows_of(c, o, run(pkg, c, o))
    perm = np.random.default_rng(1).permutation(130)
    moved, _ = rows_of(c, o, run(pkg, c, o, xbuf=_with_rows(o, o["X"][perm])))
    assert np.array_equal(bits(moved), bits(base[perm]))
    # row 129 alone, as a one-row launch on flat maps
    c1 = dict(c, M=1, xl=("flat", 0), yl=("flat", 0))
    o1 = dict(o, M=1, xbuf=o["X"][129].copy(), xmap=(D, 0, 0, 0), xidx=np.zeros(1, np.int64))
    if c["kind"] == ROWLIN:
        o1.update(ymap=(c["N"], 0, 0, 0), y_elems=c["N"], yidx=np.zeros(1, np.int64))
    one, _ = rows_of(c1, o1, run(pkg, c1, o1))
    assert np.array_equal(bits(one[0]), bits(base[129]))
    # a row of NaN at 5, a row with one Inf at 70
    X = o["X"].copy()
    X[5] = np.nan
    X[70, 300] = np.inf
    xb = _with_rows(o, X)
    out = run(pkg, c, o, xbuf=xb)
    dirty, outside = rows_of(c, o, out)
    ok = np.ones(130, bool)
    ok[[5, 70]] = False
    assert np.array_equal(bits(dirty[ok]), bits(base[ok]))
    assert not np.isfinite(dirty[~ok]).any()
    if c["kind"] == FFN:
        assert np.array_equal(bits(out[outside]), bits(xb[outside]))
    else:
        assert (bits(out[outside]) == FILL).all()


@gpu
@pytest.mark.parametrize("c", [BIG_FFN, BIG_ROWLIN], ids=cid)
def test_many_blocks(pkg, c):
    """16 449 rows: 257 full blocks and one row -- a CU starts a second block into LDS it has just used.  The rows repeat 67 distinct ones (with RoPE, each at its own
    position: rows_per_seg 67): the 67 against f64, every repeat bit-equal to its first occurrence, and two launches bit-equal to each other."""
    small = dict(c, M=BIG_DISTINCT)
    o67 = operands(small)
    rep = np.arange(BIG_M) % BIG_DISTINCT
    o = dict(o67, M=BIG_M, xbuf=o67["X"][rep].reshape(-1), xmap=(D, 0, 0, 0), xidx=np.arange(BIG_M, dtype=np.int64) * D)
    if c["kind"] == ROWLIN:
        o.update(ymap=(c["N"], 0, 0, 0), y_elems=BIG_M * c["N"], yidx=np.arange(BIG_M, dtype=np.int64) * c["N"])
    out = run(pkg, c, o)
    got, outside = rows_of(c, o, out)
    assert not outside.any()
    assert np.array_equal(bits(got), bits(got[rep])), cid(c) + ": a repeated row differs from its first occurrence"
    assert np.array_equal(bits(run(pkg, c, o)), bits(out)), cid(c) + ": two launches differ"
    want, bound = reference(small, o67)
    check(cid(c), got[:BIG_DISTINCT], want, bound)


@gpu
def test_refusals_before_any_launch(pkg):
    """what mimi_ffn_supported / mimi_rowlin_supported and the hook's buffer checks refuse is answered with PTTS_EINVAL, and nothing is launched."""
    f = pkg.runtime.debug_mimi_fused
    z = lambda *s: np.zeros(s, F32)   # noqa: E731

    def ffn(M=20, F=64, **kw):
        d = dict(kind=FFN, x_buf=z(M * D), M=M, xmap=(D, 0, 0, 0), ln_w=z(D), ln_b=z(D), w1=z(F, D), w2=z(D, F), ls=z(D))
        d.update(kw)
        return d

    def rowlin(M=20, N=128, **kw):
        d = dict(kind=ROWLIN, x_buf=z(M * D), M=M, xmap=(D, 0, 0, 0), ln_w=z(D), ln_b=z(D), w1=z(N, D), y_elems=M * N, ymap=(N, 0, 0, 0))
        d.update(kw)
        return d

    def call(kw):
        kw = dict(kw)
        return f(kw.pop("kind"), kw.pop("x_buf"), kw.pop("M"), **kw)

    tabs = (z(20, 32), z(20, 32))
    bad = {
        "ffn: a width of 256": ffn(x_buf=z(20 * 256), xmap=(256, 0, 0, 0), ln_w=z(256), ln_b=z(256), w1=z(64, 256), w2=z(256, 64), ls=z(256)),
        "ffn: a width of 1024": ffn(x_buf=z(20 * 1024), xmap=(1024, 0, 0, 0), ln_w=z(1024), ln_b=z(1024), w1=z(64, 1024), w2=z(1024, 64), ls=z(1024)),
        "rowlin: a width of 256": rowlin(x_buf=z(20 * 256), xmap=(256, 0, 0, 0), ln_w=z(256), ln_b=z(256), w1=z(128, 256)),
        "ffn: F = 48": ffn(F=48),
        "ffn: F = 16": ffn(F=16),
        "rowlin: N = 96": rowlin(N=96),
        "rowlin: N = 32": rowlin(N=32),
        "ffn: ld = 514": ffn(x_buf=z(20 * 514), xmap=(514, 0, 0, 0)),
        "ffn: x off by 2 elements": ffn(x_buf=z(20 * D + 4), xmap=(D, 0, 0, 2)),
        "ffn: batch stride 10 ld + 2": ffn(x_buf=z(2 * (10 * D + 2)), xmap=(D, 10, 10 * D + 2, 0)),
        "rowlin: x ld = 514": rowlin(x_buf=z(20 * 514), xmap=(514, 0, 0, 0)),
        "rowlin: y ld = 130": rowlin(y_elems=20 * 130, ymap=(130, 0, 0, 0)),
        "ffn: ls misaligned by one element": ffn(ls_off=1),
        "ffn: ls misaligned by two elements": ffn(ls_off=2),
        "rowlin: rope_cols = 32": rowlin(rope=tabs, rope_cols=32),
        "rowlin: rope_cols = 96": rowlin(rope=tabs, rope_cols=96),
        "rowlin: rope_cols = N + 64": rowlin(rope=tabs, rope_cols=192),
        "rowlin: tables one position short": rowlin(rope=(z(19, 32), z(19, 32)), rope_cols=64),
        "rowlin: tables short behind pos0": rowlin(rope=tabs, rope_cols=64, pos0=1),
        "rowlin: tables short for a segment": rowlin(rope=(z(11, 32), z(11, 32)), rope_cols=64, pos0=7, rows_per_seg=5),
        "rowlin: cos without sin": rowlin(rope=(z(20, 32), None), rope_cols=64),
        "ffn: x one element short": ffn(x_buf=z(20 * D - 1)),
        "ffn: the last segment past the buffer": ffn(x_buf=z(2 * 13 * D - 1), xmap=(D, 10, 13 * D, 3 * D)),
        "rowlin: x one element short": rowlin(x_buf=z(20 * D - 1)),
        "rowlin: y one element short": rowlin(y_elems=20 * 128 - 1),
        "rowlin: y's last segment past the buffer": rowlin(y_elems=(2 + 12 + 9) * 160 + 128 - 1, ymap=(160, 10, 12 * 160, 2 * 160)),
        "ffn: rows overlap (ld = 508)": ffn(x_buf=z(20 * D), xmap=(508, 0, 0, 0)),
        "ffn: segments overlap": ffn(x_buf=z(20 * D), xmap=(D, 10, 9 * D, 0)),
        "rowlin: y rows overlap": rowlin(y_elems=20 * 128, ymap=(124, 0, 0, 0)),
        "ffn: no rows": ffn(M=0),
        "kind 2": ffn(kind=2),
    }
    pkg.runtime.launch_counts(True)
    try:
        for what, kw in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                call(kw)
            assert e.value.code == pkg.runtime.PTTS_EINVAL, what
            assert "ptts_debug_mimi_fused" in str(e.value), what
        assert pkg.runtime.launch_counts(True) == {}
        # and their neighbours are taken (a caller's census sees the hook's launch)
        ok = [ffn(F=32), ffn(ls_off=4), ffn(x_buf=z(2 * 13 * D), xmap=(D, 10, 13 * D, 3 * D)), rowlin(N=64), rowlin(rope=tabs, rope_cols=128),
              rowlin(rope=(z(12, 32), z(12, 32)), rope_cols=64, pos0=7, rows_per_seg=5), rowlin(x_buf=z(20 * 508 + 4), xmap=(508, 0, 0, 0)),
              rowlin(y_elems=(2 + 12 + 9) * 160 + 128, ymap=(160, 10, 12 * 160, 2 * 160))]
        for kw in ok:
            out = call(kw)["out"]
            stored = bits(out) != FILL   # (kind 0: the whole x buffer comes back; kind 1: 20 rows of N columns, the padding still 0xff)
            assert np.isfinite(out[stored]).all() and stored.sum() == (out.size if kw["kind"] == FFN else 20 * kw["w1"].shape[0])
        assert pkg.runtime.launch_counts(False) == {"k_mimi_ffn": 3, "k_mimi_rowlin": 3, "k_mimi_rowlin+rope": 2}
    finally:
        pkg.runtime.launch_counts(False)


@gpu
def test_cases_reach_every_variant(pkg):
    """From the census: a case of each family runs exactly ONE launch -- k_mimi_ffn, k_mimi_rowlin or k_mimi_rowlin+rope -- and nothing else, as the hook reports it
    (run() asserts that for every case of this file) and as a census the caller switched on sees it."""
    picks = [FFN_GRID[0], FFN_ONEHOT[1], FFN_MAPS[1], ROWLIN_GRID[0], ROWLIN_MAPS[3], ROWLIN_ROPE[0], ROWLIN_MAPS[2]]
    assert [census_name(c) for c in picks] == ["k_mimi_ffn"] * 3 + ["k_mimi_rowlin"] * 2 + ["k_mimi_rowlin+rope"] * 2
    pkg.runtime.launch_counts(True)
    try:
        for c in picks:
            run(pkg, c, operands(c))
            assert pkg.runtime.launch_counts(True) == {census_name(c): 1}, cid(c)
    finally:
        pkg.runtime.launch_counts(False)
