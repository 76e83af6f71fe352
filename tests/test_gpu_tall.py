"""The AR step's linears at 128 rows and more (csrc/tall.hip: k_rowprep + k_tall), stand-alone against f64 numpy on the same operands.

What they replace: Linear.Forward (internal/native/linear.go:117-182) behind LayerNorm (linear.go:295-309) in a transformer layer of the flow LM
(flow_transformer.go:326-389), GELU by erf (tensor_util.go:84-94).  The end-to-end checks -- teacher-forced against the oracle at 128 rows, slot symmetry and
64-row agreement at 128 / 256 -- are tests/test_gpu_wide_batch.py; here every shape of the launch plan and the edges of the tiling (rows that fill no whole
32- or 64-row tile, a last column block with one 16-column tile, split-K planes, the bf16 hi / lo plane epilogue) are checked value by value.

Tolerance: activations enter the matrix pipe as bf16 hi + lo (|x - hi - lo| <= 2^-17 |x|), weights are bf16 exactly, sums are f32 over K <= 4096:
|error| <= 3e-5 * (sum_k |a_k w_k| + |bias| + |R|) bounds both with a margin of ~4 (the same bound the 64-row step linear is tested with: tests/test_gpu_step_linear.py).

That bound is loose (observed errors are 0.02 - 0.25 of it), so the second half of the file -- each kernel alone through ptts_debug_tall, every buffer returned
whole -- does not lean on it: k_tall runs on operands whose product is exact in f32 (tests/_tall_ref.py) and is compared bit for bit, in both block heights, at
every ring fill, tile edge, epilogue and split-K slicing; k_rowprep's sums are compared bit for bit, its LayerNorm within the project's layer-norm tolerance and
bit for bit with k_skinny's prologue; GELU is measured against f64 by itself."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round
from _parity import record

pytestmark = pytest.mark.gpu
TOL = 3e-5


def layernorm64(x, w, b, eps):
    x = x.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)      # biased, linear.go:295-309
    return (x - mu) / np.sqrt(var + eps) * w.astype(np.float64) + b.astype(np.float64)


def gelu64(v):
    return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))


def check(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    record(name, float(err.max()), 0.0, float(np.abs(want).max()), (TOL, 0))
    assert np.isfinite(got).all() and worst <= 1.0, (name, float(err.max()), worst)


@pytest.mark.parametrize("rows,n_out", [(128, 3072), (256, 3072), (129, 1024), (200, 1040), (97, 64)])
def test_rowprep_then_tall_is_layernorm_then_linear(pkg, rows, n_out):
    """[sum of 3 split-K planes + bias + residual -> LayerNorm -> in_proj]: the updated rows bit for bit (f32 adds in the kernel's order), the product to the
    operand-split bound; 129 / 200 / 97 rows leave a ragged last row tile, 1040 columns a last column block of one 16-column tile."""
    rng = np.random.default_rng(rows * 7 + n_out)
    K = 1024
    x = rng.standard_normal((rows, K), dtype=np.float32)
    planes = (0.3 * rng.standard_normal((3, rows, K))).astype(np.float32)
    pbias = (0.1 * rng.standard_normal(K)).astype(np.float32)
    lw = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    lb = (0.1 * rng.standard_normal(K)).astype(np.float32)
    w = bf16_round(0.05 * rng.standard_normal((n_out, K)))
    bias = rng.standard_normal(n_out).astype(np.float32)
    got, x_out = pkg.runtime.debug_tall_linear(x, w, bias=bias, ln=(lw, lb, 1e-5), planes=planes, pbias=pbias)
    xs = x + (((planes[0] + planes[1]) + planes[2]) + pbias)          # the kernel's order, f32
    assert np.array_equal(x_out, xs)
    y = layernorm64(xs, lw, lb, 1e-5)
    want = y @ w.astype(np.float64).T + bias
    bound = TOL * (np.abs(y) @ np.abs(w.astype(np.float64)).T + np.abs(bias)) + 1e-6
    check(f"k_rowprep + k_tall [{rows} x {n_out} x 1024], LayerNorm + 3 planes", got, want, bound)


@pytest.mark.parametrize("rows", [128, 160, 256])
def test_tall_gelu_through_the_bf16_planes(pkg, rows):
    """linear1 + GELU leaving as the hi / lo planes linear2 reads: hi + lo is the value to 2^-16."""
    rng = np.random.default_rng(rows)
    K, N = 1024, 4096
    x = rng.standard_normal((rows, K), dtype=np.float32)
    lw, lb = np.ones(K, np.float32), np.zeros(K, np.float32)
    w = bf16_round(0.04 * rng.standard_normal((N, K)))
    bias = (0.2 * rng.standard_normal(N)).astype(np.float32)
    got, _ = pkg.runtime.debug_tall_linear(x, w, bias=bias, ln=(lw, lb, 1e-5), epi=1, out_planes=True)
    y = layernorm64(x, lw, lb, 1e-5)
    pre = y @ w.astype(np.float64).T + bias
    want = gelu64(pre)
    bound = 1.2 * TOL * (np.abs(y) @ np.abs(w.astype(np.float64)).T + np.abs(bias)) + 2.0 ** -16 * np.abs(want) + 1e-6   # |gelu'| <= 1.13
    check(f"k_tall [{rows} x 4096 x 1024] + GELU -> bf16 hi/lo planes", got, want, bound)


@pytest.mark.parametrize("rows,splitk", [(128, 4), (256, 4), (131, 4), (192, 1), (128, 2)])
def test_tall_linear2_split_k_planes_and_residual(pkg, rows, splitk):
    """linear2 over K = 4096: the split-K planes (plane 0 = residual + bias + its slice's sums, the others raw sums) add up to R + x W^T + b; splitk 1 is the
    residual-add epilogue."""
    rng = np.random.default_rng(rows + splitk)
    K, N = 4096, 1024
    x = rng.standard_normal((rows, K), dtype=np.float32)
    w = bf16_round(0.03 * rng.standard_normal((N, K)))
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((rows, N), dtype=np.float32)
    got, _ = pkg.runtime.debug_tall_linear(x, w, bias=bias, residual=res, epi=0 if splitk > 1 else 4, splitk=splitk)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    if splitk > 1:
        ks = K // splitk
        for z in range(splitk):
            part = x64[:, z * ks:(z + 1) * ks] @ w64[:, z * ks:(z + 1) * ks].T
            ab = np.abs(x64[:, z * ks:(z + 1) * ks]) @ np.abs(w64[:, z * ks:(z + 1) * ks]).T
            if z == 0:
                part = res + (part + bias)
                ab = ab + np.abs(bias) + np.abs(res)
            check(f"k_tall linear2 [{rows} x 1024 x 4096] split-K {splitk}, plane {z}", got[z], part, TOL * ab + 1e-6)
        got = got.astype(np.float64).sum(axis=0)
    want = res + (x64 @ w64.T + bias)
    bound = TOL * (np.abs(x64) @ np.abs(w64).T + np.abs(bias) + np.abs(res)) * (splitk if splitk > 1 else 1) + 1e-6
    check(f"k_tall linear2 [{rows} x 1024 x 4096] split-K {splitk}, sum", got, want, bound)


def test_tall_rejects_what_it_does_not_take(pkg):
    x = np.zeros((128, 1000), np.float32)        # K % 128 != 0
    with pytest.raises(pkg.PttsError):
        pkg.runtime.debug_tall_linear(x, np.zeros((64, 1000), np.float32))
    x = np.zeros((300, 1024), np.float32)        # more rows than a step takes
    with pytest.raises(pkg.PttsError):
        pkg.runtime.debug_tall_linear(x, np.zeros((64, 1024), np.float32))
    x = np.zeros((128, 768), np.float32)         # a LayerNorm width k_rowprep is not built for
    with pytest.raises(pkg.PttsError):
        pkg.runtime.debug_tall_linear(x, np.zeros((64, 768), np.float32), ln=(np.ones(768, np.float32), np.zeros(768, np.float32), 1e-5))


# ================================================================================================ value-level, on ptts_debug_tall (include/ptts_debug.h)
# Each kernel alone, every launch form and tile edge, every output buffer returned whole.  Operands, case lists and f64 models: tests/_tall_ref.py (their own
# premises are checked without a GPU in tests/test_tall_ref.py).
from _kernel_ref import F32, bits, split, untouched, gelu64 as gelu64_ref   # noqa: E402
from _tall_ref import (EPI_GELU, EPI_NONE, EPI_RESADD, EPI_SILU, FAMILIES, LN_TOL, PREP_CASES, SPLIT_CASES, TALL_CASES, exact_condition,   # noqa: E402
                       exact_operands, ln_close, prep_id, prep_operands, ss_slices, tall_id, tall_model, updated_rows)
from _tall_ref import layernorm64 as ln64   # noqa: E402

GELU_ABS = 3.88e-7   # 4 x 9.70e-8, the worst |gelu1 - gelu64| / max(1, |v|) test_tall_gelu_against_f64 observed on the MI355X (see its docstring)


def u16(a):
    """bf16 values held in f32 as their 16 bits"""
    return (np.ascontiguousarray(a, F32).view(np.uint32) >> 16).astype(np.uint16)


def grid_of(M, N, form, S=1):
    return (-(-N // 64), -(-M // form), max(1, S))


def same_planes(name, r, want32, M, N):
    """ch / cl are the kernels' split of the f32 result, as bits; nothing else of the two buffers was stored to"""
    hi, lo = split(want32)
    assert np.array_equal(r["ch"][:M, :N], u16(hi)) and np.array_equal(r["cl"][:M, :N], u16(lo)), name
    for p in (r["ch"], r["cl"]):
        assert untouched(p[M:]) and untouched(p[:, N:]), name + ": slack rows or padding columns of a result plane were written"


@pytest.mark.parametrize("c", TALL_CASES, ids=tall_id)
def test_tall_exact_operands_bit_for_bit(pkg, c):
    """k_tall alone on operands whose product is exact in f32 in any order of summation: the result IS the f64 product cast to f32.  K = 128 .. 768 leaves the LDS
    ring (3 stages at 64 rows, 5 at 32) under-filled, exactly filled and wrapped; N = 4 .. 144 ends in every width of the last 16-column tile; lda, ldc, ldr, ldp
    differ from the widths and three slack rows follow the M the launch is told of."""
    M, N, K, form = c["M"], c["N"], c["K"], c["form"]
    resadd = c["epi"] == EPI_RESADD
    x, cc, d, W, b, R = exact_operands(M * 131 + N * 7 + K, M, N, K, bias=c["bias"], residual=resadd)
    exact_condition(x, cc, d, W, b, R, M, N, K)
    r = pkg.runtime.debug_tall("tall", x, M=M, w=W, bias=b, residual=R, epi=c["epi"], form=form, out_planes=c["planes"], ldc=N + 4, ldp=N + 4)
    name = "k_tall " + tall_id(c)
    assert r["launched"] == {"k_tall": 1} and r["form"] == form and r["grid"] == grid_of(M, N, form), (name, r["launched"], r["form"], r["grid"])
    want = tall_model(x, W, b, R, M, N, K, c["epi"]).astype(F32)
    if c["planes"]:
        assert r["out"] is None
        same_planes(name, r, want, M, N)
    else:
        out = r["out"]
        assert out.shape == (M + 3, N + 4) and untouched(out[M:]) and untouched(out[:, N:]), name + ": slack rows or padding columns were written"
        assert np.array_equal(bits(out[:M, :N]), bits(want)), (name, float(np.abs(out[:M, :N].astype(np.float64) - want).max()))


@pytest.mark.parametrize("c", SPLIT_CASES, ids=tall_id)
def test_tall_split_k_planes_bit_for_bit(pkg, c):
    """split-K on exact operands, each plane for itself: slice z covers ss_per = ceil(K / 128 / S) chunks from z ss_per on -- uneven at (640, 2), empty (a plane of
    +0.0) at (128, 2) and (640, 4); with R plane 0 is R + (sums_0 + bias), without R (and without a bias: tall_supported refuses that) every plane is raw sums."""
    M, N, K, S, form = c["M"], c["N"], c["K"], c["S"], c["form"]
    x, cc, d, W, b, R = exact_operands(K + S + M, M, N, K, bias=c["full"], residual=c["full"])
    exact_condition(x, cc, d, W, b, R, M, N, K)
    rows = x.shape[0]
    r = pkg.runtime.debug_tall("tall", x, M=M, w=W, bias=b, residual=R, splitk=S, form=form, zstride=rows * N + 8)
    name = "k_tall " + tall_id(c)
    assert r["launched"] == {"k_tall": 1} and r["form"] == form and r["grid"] == grid_of(M, N, form, S), (name, r["launched"], r["form"], r["grid"])
    assert r["out"].shape == (S, rows * N + 8)
    want = tall_model(x, W, b, R, M, N, K, EPI_NONE, S)
    for z, (k0, k1) in enumerate(ss_slices(K, S)):
        got = r["out"][z]
        assert untouched(got[M * N:]), f"{name}: plane {z} was written behind its {M} rows"
        assert np.array_equal(bits(got[:M * N].reshape(M, N)), bits(want[z].astype(F32))), f"{name}: plane {z} (k {k0}..{k1})"
        if k0 == k1 and not (z == 0 and c["full"]):
            assert (bits(got[:M * N]) == 0).all(), f"{name}: the empty slice {z} is not +0.0"


@pytest.mark.parametrize("planes", [False, True], ids=["f32", "planes"])
def test_tall_gelu_against_f64(pkg, planes):
    """gelu1 (device_util.h: 0.5 v (1 + erff(v / sqrt 2))) against the f64 GELU over [-8, 8] and 0: identity weights and pre-activations of 16 significant bits make
    the product exact (hi + lo is the input), so EPI_GELU's output IS gelu1 of the input.  This measures the function, not a GEMM.  The installed HIP headers state
    no error for erff, so GELU_ABS -- an absolute error per max(1, |v|) -- is 4 x the worst observed on the MI355X (profiles/tall_parity_observed.json, "k_tall
    gelu1"); it has to stay below 2e-6, about 30 f32 ulps over what an erff of a few ulps gives.  As planes the result is the kernels' split of the same f32 values."""
    rng = np.random.default_rng(5)
    M, K = 256, 128
    v = rng.choice([-1.0, 1.0], (M, K)) * 10.0 ** rng.uniform(-6.0, math.log10(8.0), (M, K))
    v[rng.random(v.shape) < 0.01] = 0.0
    v[0, :4] = [8.0, -8.0, 1.0, -1.0]
    v = (v.astype(F32).view(np.uint32) & np.uint32(0xFFFF0000 | 0xFF00)).view(F32)   # 16 significant bits
    hi, lo = split(v)
    assert np.array_equal(hi + lo, v) and float(np.abs(v).max()) <= 8.0
    want = gelu64_ref(v.astype(np.float64))
    scale = np.maximum(1.0, np.abs(v.astype(np.float64)))
    for form in (32, 64):
        r = pkg.runtime.debug_tall("tall", v, w=np.eye(K, dtype=F32), epi=EPI_GELU, form=form, out_planes=planes)
        assert r["launched"] == {"k_tall": 1} and r["form"] == form
        if planes:
            f32 = pkg.runtime.debug_tall("tall", v, w=np.eye(K, dtype=F32), epi=EPI_GELU, form=form)["out"]
            same_planes(f"k_tall gelu form {form}", r, f32, M, K)
            continue
        err = np.abs(r["out"].astype(np.float64) - want) / scale
        worst = float(err.max())
        at = float(v.reshape(-1)[err.argmax()])
        record(f"k_tall gelu1 form {form}", worst, worst / GELU_ABS, 1.0, (GELU_ABS, 0))
        print(f"gelu1, form {form}: worst |gelu1 - gelu64| / max(1, |v|) {worst:.3e} at v = {at:.6g}; GELU_ABS {GELU_ABS:.2e}")
        assert np.isfinite(r["out"]).all() and 4.0 * worst <= GELU_ABS <= 2e-6, (worst, GELU_ABS)


_FORMS_REF = {}


def forms_operands(M):
    """random full-mantissa operands [M x 1040 x 1024] and their f64 products, whole and in 4 slices, once per M"""
    if M not in _FORMS_REF:
        rng = np.random.default_rng(M)
        N, K = 1040, 1024
        x = rng.standard_normal((M, K), dtype=np.float32)
        w = bf16_round(0.05 * rng.standard_normal((N, K)))
        bias = rng.standard_normal(N).astype(np.float32)
        R = rng.standard_normal((M, N), dtype=np.float32)
        x64, w64 = x.astype(np.float64), np.abs(w.astype(np.float64))
        ab = [np.abs(x64[:, k0:k1]) @ w64[:, k0:k1].T for k0, k1 in ss_slices(K, 4)]
        _FORMS_REF[M] = (x, w, bias, R, tall_model(x, w, bias, R, M, N, K, EPI_RESADD), tall_model(x, w, bias, R, M, N, K, EPI_NONE, 4), ab)
    return _FORMS_REF[M]


@pytest.mark.parametrize("kind", ["f32", "planes", "split4"])
@pytest.mark.parametrize("M", [97, 128, 200])
def test_tall_forms_give_the_same_bits(pkg, M, kind):
    """32- and 64-row blocks run the same MFMA sequence per output over the same slice: identical bits on random full-mantissa operands, f32 and planes, whole K
    and four slices; the same runs against f64 at the operand-split bound."""
    x, w, bias, R, want, want_planes, ab = forms_operands(M)
    N = 1040
    S = 4 if kind == "split4" else 1
    kw = dict(w=w, bias=bias, residual=R, epi=EPI_NONE if S > 1 else EPI_RESADD, splitk=S, out_planes=(kind == "planes"))
    r32, r64 = pkg.runtime.debug_tall("tall", x, form=32, **kw), pkg.runtime.debug_tall("tall", x, form=64, **kw)
    assert r32["launched"] == r64["launched"] == {"k_tall": 1} and r32["grid"] == grid_of(M, N, 32, S) and r64["grid"] == grid_of(M, N, 64, S)
    assert pkg.runtime.debug_tall("tall", x, form=0, **kw)["form"] == (32 if M <= 128 else 64)
    name = f"k_tall forms [{M} x 1040 x 1024] {kind}"
    if kind == "planes":
        assert np.array_equal(r32["ch"], r64["ch"]) and np.array_equal(r32["cl"], r64["cl"]), name
        got = pkg.runtime._bf16_bits_f32(r32["ch"]).astype(np.float64) + pkg.runtime._bf16_bits_f32(r32["cl"])
        check(name, got, want, TOL * (sum(ab) + np.abs(bias) + np.abs(R)) + 2.0 ** -16 * np.abs(want) + 1e-6)
        return
    assert np.array_equal(bits(r32["out"]), bits(r64["out"])), name
    if S > 1:
        for z in range(S):
            check(f"{name} plane {z}", r32["out"][z].reshape(M, N), want_planes[z], TOL * (ab[z] + (np.abs(bias) + np.abs(R) if z == 0 else 0.0)) + 1e-6)
    else:
        check(name, r32["out"], want, TOL * (sum(ab) + np.abs(bias) + np.abs(R)) + 1e-6)


def run_prep(pkg, c, seed=None, **over):
    x, pl, pb, lw, lb = prep_operands(c["D"] * 3 + c["M"] if seed is None else seed, c["family"], c["M"], c["D"], c["psplit"], c["pbias"], production=c["production"])
    kw = dict(M=c["M"], ln=(lw, lb, 1e-5), planes=pl, pbias=pb, ldy=c["D"] + 8, want_x_out=c["want_x"], want_y_out=c["want_y"])
    kw.update(over)
    return (x, pl, pb, lw, lb), pkg.runtime.debug_tall("rowprep", x, **kw)


@pytest.mark.parametrize("c", PREP_CASES, ids=prep_id)
def test_rowprep_rows(pkg, c):
    """k_rowprep alone: x_out is x + (((p0 + p1) + ...) + pbias) bit for bit, y_out the LayerNorm of it within LN_TOL of f64, yh / yl the kernels' split of y_out as
    bits; constant rows normalise to ln_b exactly; rows behind M, columns behind D, a plane's tail and a switched-off x_out / y_out keep the fill."""
    M, D = c["M"], c["D"]
    (x, pl, pb, lw, lb), r = run_prep(pkg, c)
    name = "k_rowprep " + prep_id(c)
    assert r["launched"] == {"k_rowprep": 1} and r["form"] == 0 and r["grid"] == (-(-M // 4), 1, 1), (name, r["launched"], r["grid"])
    xs = updated_rows(x, pl, pb, M, D)
    if c["psplit"] and c["want_x"]:
        assert np.array_equal(bits(r["x_out"][:M]), bits(xs)), name + ": x_out is not x + (((p0 + p1) + ...) + pbias) bit for bit"
        assert untouched(r["x_out"][M:])
    else:
        assert untouched(r["x_out"]), name + ": x_out was written without a pending sum, or switched off"
    want = ln64(xs, lw, lb, 1e-5)
    y = pkg.runtime._bf16_bits_f32(r["yh"][:M, :D]) + pkg.runtime._bf16_bits_f32(r["yl"][:M, :D])   # without y_out: hi + lo, the value to 2^-17
    if c["want_y"]:
        y = r["y_out"][:M]
        assert untouched(r["y_out"][M:])
        hi, lo = split(y)
        assert np.array_equal(r["yh"][:M, :D], u16(hi)) and np.array_equal(r["yl"][:M, :D], u16(lo)), name + ": yh / yl are not the split of y_out"
    else:
        assert untouched(r["y_out"]), name + ": y_out was written although switched off"
    worst = ln_close(y, want) if c["want_y"] else float((np.abs(y.astype(np.float64) - want) / (LN_TOL[0] + (LN_TOL[1] + 2.0 ** -16) * np.abs(want))).max())
    record(name + " y", float(np.abs(y.astype(np.float64) - want).max()), worst, float(np.abs(want).max()), LN_TOL)
    assert np.isfinite(y).all() and worst <= 1.0, (name, worst)
    if FAMILIES[c["family"]] is None and c["want_y"]:
        assert np.array_equal(bits(y), bits(np.broadcast_to(lb, y.shape))), name + ": a constant row does not normalise to ln_b"
    for p in (r["yh"], r["yl"]):
        assert untouched(p[M:]) and untouched(p[:, D:]), name + ": slack rows or padding columns of yh / yl were written"


@pytest.mark.parametrize("D", [512, 1024])
def test_rowprep_nan_stays_in_its_row(pkg, D):
    """a NaN in one row (in x, or in a pending plane) makes that row NaN and changes no bit of any other"""
    c = dict(D=D, M=9, psplit=3, pbias=True, production=False, family="normal", want_x=True, want_y=True)
    ops, clean = run_prep(pkg, c)
    for where in ("x", "plane"):
        x, pl = ops[0].copy(), ops[1].copy()
        if where == "x":
            x[4, 100] = np.nan
        else:
            pl[1, 4 * D + 100] = np.nan
        r = pkg.runtime.debug_tall("rowprep", x, M=9, ln=(ops[3], ops[4], 1e-5), planes=pl, pbias=ops[2], ldy=D + 8)
        keep = np.arange(r["y_out"].shape[0]) != 4
        assert np.isnan(r["y_out"][4]).all() and np.isnan(r["x_out"][4, 100])
        for k in ("x_out", "y_out", "yh", "yl"):
            assert np.array_equal(r[k][keep].view(np.uint8), clean[k][keep].view(np.uint8)), (where, k)


@pytest.mark.parametrize("psplit", [0, 3])
@pytest.mark.parametrize("M", [1, 17, 250])
@pytest.mark.parametrize("D", [512, 1024])
def test_rowprep_has_the_bits_of_the_step_kernels_prologue(pkg, D, M, psplit):
    """tall.hip: "a row normalises to the same bits on either path" -- the same x, planes, pbias, ln_w, ln_b, eps through k_skinny's fused prologue (64 dummy
    columns): its x_out and y_out equal k_rowprep's as bits."""
    c = dict(D=D, M=M, psplit=psplit, pbias=bool(psplit), production=False, family="normal", want_x=True, want_y=True)
    (x, pl, pb, lw, lb), r = run_prep(pkg, c)
    dense = np.ascontiguousarray(x[:M, :D])
    planes = None if pl is None else np.ascontiguousarray(pl[:, :M * D].reshape(psplit, M, D))
    s = pkg.runtime.debug_step_linear(dense, np.zeros((64, D), F32), ln=True, ln_wb=(lw, lb), eps=1e-5, planes=planes, pbias=pb)
    assert s["k_skinny"] >= 1
    if psplit:
        assert np.array_equal(bits(s["x_out"]), bits(r["x_out"][:M]))
    a, b = s["y_out"], r["y_out"][:M]
    want = ln64(updated_rows(x, pl, pb, M, D), lw, lb, 1e-5)
    assert ln_close(a, want) <= 1.0 and ln_close(b, want) <= 1.0
    ulps = np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))
    print(f"k_rowprep vs k_skinny prologue D {D} M {M} psplit {psplit}: {int((ulps != 0).sum())} of {ulps.size} values differ, at most {int(ulps.max())} ulps")
    assert np.array_equal(bits(a), bits(b)), int(ulps.max())


def _refusals():
    K, N, D, R = 128, 8, 512, 4
    x = np.ones((R, K), F32)
    w = np.ones((N, K), F32)
    xd = np.ones((R, D), F32)
    ln = (np.ones(D, F32), np.zeros(D, F32), 1e-5)
    res = lambda ld: np.ones((R, ld), F32)   # noqa: E731
    pln = lambda n: np.ones((1, n), F32)     # noqa: E731
    T = lambda xx=x, **kw: ("tall", xx, dict(dict(w=w), **kw))             # noqa: E731
    P = lambda xx=xd, **kw: ("rowprep", xx, dict(dict(ln=ln), **kw))       # noqa: E731
    return {   # clause: (refused, its accepted neighbour)
        "K % 128": (T(np.ones((R, 192), F32), w=np.ones((N, 192), F32)), T(np.ones((R, 256), F32), w=np.ones((N, 256), F32))),
        "N % 4": (T(w=np.ones((6, K), F32)), T(w=np.ones((4, K), F32))),
        "M > 256": (T(np.ones((257, K), F32)), T(np.ones((256, K), F32))),
        "lda % 8": (T(np.ones((R, K + 4), F32)), T(np.ones((R, K + 8), F32))),
        "ldc % 4": (T(ldc=N + 2), T(ldc=N + 4)),
        "ldr % 4": (T(residual=res(N + 2)), T(residual=res(N + 4))),
        "ldp % 4": (T(out_planes=True, ldp=N + 2), T(out_planes=True, ldp=N + 4)),
        "ldx % 4": (P(np.ones((R, D + 2), F32)), P(np.ones((R, D + 4), F32))),
        "ldy % 4": (P(ldy=D + 2), P(ldy=D + 4)),
        "pstride % 4": (P(planes=pln(R * D + 2)), P(planes=pln(R * D + 4))),
        "D = 768": (P(np.ones((R, 768), F32), ln=(np.ones(768, F32), np.zeros(768, F32), 1e-5)), P()),
        "splitk > 1 with an epilogue": (T(splitk=2, epi=EPI_GELU), T(splitk=2)),
        "splitk > 1 with planes": (T(splitk=2, out_planes=True), T(splitk=2)),
        "EPI_RESADD without R": (T(epi=EPI_RESADD), T(epi=EPI_RESADD, residual=res(N))),
        "epi = SILU": (T(epi=EPI_SILU), T(epi=EPI_GELU)),
        "splitk > 1 with a bias and no R": (T(splitk=2, bias=np.ones(N, F32)), T(splitk=2, bias=np.ones(N, F32), residual=res(N))),
        "form = 48": (T(form=48), T(form=64)),
        "rows < M": (T(M=R + 1), T(M=R)),
    }


REFUSALS = _refusals()


@pytest.mark.parametrize("clause", list(REFUSALS))
def test_tall_refusals_before_any_launch(pkg, clause):
    """one refusal per clause of tall_supported / rowprep_supported and of the hook's own checks: PTTS_EINVAL, nothing launched; beside it the nearest call that
    is taken, which launches exactly one kernel"""
    (op, x, kw), (gop, gx, gkw) = REFUSALS[clause]
    with pytest.raises(pkg.PttsError) as e:
        pkg.runtime.debug_tall(op, x, **kw)
    assert e.value.code == pkg.runtime.PTTS_EINVAL and e.value.partial["launched"] == {}, (clause, e.value.code, e.value.partial["launched"])
    r = pkg.runtime.debug_tall(gop, gx, **gkw)
    assert r["launched"] == {"k_tall" if gop == "tall" else "k_rowprep": 1}, (clause, r["launched"])


def test_tall_split_k_bias_rides_on_the_residual_only(pkg):
    """k_skinny's convention, kept: with R plane 0 carries R + (sums_0 + bias); without R the planes are raw sums and a bias would be dropped in silence -- refused
    (test_tall_refusals_before_any_launch), the consumer adds it (PendingSum::bias).  Here: the bias does arrive with R, and raw planes are raw."""
    M, N, K = 33, 68, 256
    x, cc, d, W, b, R = exact_operands(1, M, N, K)
    full = pkg.runtime.debug_tall("tall", x, M=M, w=W, bias=b, residual=R, splitk=2)["out"]
    raw = pkg.runtime.debug_tall("tall", x, M=M, w=W, splitk=2)["out"]
    p0 = raw[0, :M * N].reshape(M, N)
    assert np.array_equal(bits(full[0, :M * N].reshape(M, N)), bits(R[:M, :N] + (p0 + b)))
    assert np.array_equal(bits(full[1, :M * N]), bits(raw[1, :M * N]))
