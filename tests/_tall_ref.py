"""Operands, case lists and f64 models for the value-level tests of csrc/tall.hip (k_rowprep, k_tall): tests/test_gpu_tall.py runs them on the GPU,
tests/test_tall_ref.py checks without one that the operands are what they claim and that the tolerances have room for the kernels' f32 arithmetic.

Exact operands.  x = c + d with |c| in [1, 2) a multiple of 1/8 (bf16 holds it: hi = c) and d in {0, +-2^-9} (a quarter of c's bf16 ulp, so hi stays c and
lo = d exactly); W multiples of 1/8 (1/4 at K = 4096) in [-1, 1]; bias and R multiples of 2^-12.  Every product hi w is a multiple of 2^-6, every lo w of
2^-12, and as long as sum_k |x w| + |bias| + |R| < 2^12 every partial sum in ANY order is a multiple of 2^-12 below 2^24 of them: an f32 holds it exactly.
The kernel's result then does not depend on its order of summation and must equal the f64 product cast to f32 bit for bit (exact_condition asserts the
premises per case)."""
import numpy as np

from _kernel_ref import F32, bf16_round, split

LN_TOL = (1e-4, 1e-4)   # the project's layer-norm tolerance (tests/test_gpu_step_linear.py, TOL["layer_norm"] in test_gpu_ops.py)
EPI_NONE, EPI_GELU, EPI_SILU, EPI_RESADD = 0, 1, 2, 4   # kernels.h Epi
JUNK = F32(1.0e30)      # what padding columns and slack rows of an INPUT hold: a load that strays into them shows in every sum


# ------------------------------------------------------------------------------------------------ k_tall: exact operands
def exact_operands(seed, M, N, K, *, bias=True, residual=True, rows=None, lda=None, ldr=None):
    """(x [rows, lda], c, d, W [N, K], bias [N] or None, R [rows, ldr] or None); rows behind M and columns behind K / N hold JUNK."""
    rng = np.random.default_rng(seed)
    rows, lda, ldr = rows or M + 3, lda or K + 8, ldr or N + 8
    c = (rng.integers(8, 16, (M, K)) * rng.choice([-1, 1], (M, K)) / 8.0).astype(F32)
    d = (rng.integers(-1, 2, (M, K)) * 2.0 ** -9).astype(F32)
    x = np.full((rows, lda), JUNK, F32)
    x[:M, :K] = c + d
    den = 4 if K >= 4096 else 8
    W = (rng.integers(-den, den + 1, (N, K)) / float(den)).astype(F32)
    b = (rng.integers(-8192, 8193, N) * 2.0 ** -12).astype(F32) if bias else None
    R = None
    if residual:
        R = np.full((rows, ldr), JUNK, F32)
        R[:M, :N] = rng.integers(-8192, 8193, (M, N)) * 2.0 ** -12
    return x, c, d, W, b, R


def exact_condition(x, c, d, W, bias, R, M, N, K):
    """the premises of the docstring above, for one set of operands; returns log2 of the largest sum in units of 2^-12"""
    hi, lo = split(x[:M, :K])
    assert np.array_equal(hi, c) and np.array_equal(lo, d)
    assert np.array_equal(bf16_round(W), W)
    mag = np.abs(x[:M, :K].astype(np.float64)) @ np.abs(W.astype(np.float64)).T
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))
    if R is not None:
        mag = mag + np.abs(R[:M, :N].astype(np.float64))
    units = float(mag.max()) * 4096.0
    assert units < 2.0 ** 24, units
    return float(np.log2(units))


def ss_slices(K, S):
    """the K ranges of k_tall's split-K slices: ss_per = ceil(ceil(K / 128) / S) chunks of 128 each; a slice past the end is empty"""
    nss = (K + 127) // 128
    per = (nss + S - 1) // S if S > 1 else nss
    return [(min(z * per, nss) * 128, min((z + 1) * per, nss) * 128) for z in range(max(S, 1))]


def tall_model(x, W, bias, R, M, N, K, epi, S=1):
    """f64: the result [M, N], or the S planes (plane 0 = R + (sums_0 + bias) with R, raw sums otherwise)"""
    x64, w64 = x[:M, :K].astype(np.float64), W.astype(np.float64)
    if S > 1:
        planes = [x64[:, k0:k1] @ w64[:, k0:k1].T for k0, k1 in ss_slices(K, S)]
        if R is not None:
            planes[0] = R[:M, :N] + (planes[0] + (bias.astype(np.float64) if bias is not None else 0.0))
        return planes
    v = x64 @ w64.T
    if bias is not None:
        v = v + bias
    if epi == EPI_RESADD:
        v = R[:M, :N] + v
    return v


def _tall_cases():
    Ms, Ns, Ks = [1, 17, 32, 33, 64, 65, 128, 129, 193, 256], [4, 20, 64, 68, 144], [128, 256, 384, 512, 640, 768]
    kinds = [(EPI_NONE, False), (EPI_RESADD, False), (EPI_NONE, True), (EPI_RESADD, True)]   # (epi, result as bf16 planes)
    triples = [(M, Ns[i % 5], Ks[i % 6]) for i, M in enumerate(Ms)]
    triples += [(Ms[(3 * i + 1) % 10], N, Ks[(i + 2) % 6]) for i, N in enumerate(Ns)]
    triples += [(Ms[(3 * i + 5) % 10], Ns[(i + 3) % 5], K) for i, K in enumerate(Ks)]
    cases = []
    for i, (M, N, K) in enumerate(triples):
        for form in (32, 64):
            epi, planes = kinds[(i + (form == 64)) % 4]
            cases.append(dict(M=M, N=N, K=K, form=form, epi=epi, planes=planes, bias=((i // 4) % 2 == 0)))
    return cases, (Ms, Ns, Ks, kinds)


TALL_CASES, TALL_AXES = _tall_cases()
SPLIT_CASES = [dict(M=M, N=68, K=K, S=S, form=form, full=full)            # full: R + bias; otherwise neither
               for i, (K, S) in enumerate([(128, 2), (640, 2), (640, 4), (768, 3), (1024, 4), (4096, 4)])
               for j, (M, form) in enumerate([(33, 32), (129, 64), (33, 64), (129, 32)]) if (j < 2 or (i + j) % 2 == 0) for full in (True, False)]


def tall_id(c):
    s = f"{c['M']}x{c['N']}x{c['K']}-f{c['form']}"
    if "S" in c:
        return s + f"-S{c['S']}" + ("-R+b" if c["full"] else "-raw")
    return s + ("-resadd" if c["epi"] == EPI_RESADD else "-none") + ("-planes" if c["planes"] else "-f32") + ("-b" if c["bias"] else "-nob")


# ------------------------------------------------------------------------------------------------ k_rowprep
FAMILIES = {"normal": (0.0, 1.0), "offset": (30.0, 1.0), "small": (0.0, 0.01), "const": None}   # (mean, sigma) of the rows LayerNorm sees


def prep_operands(seed, family, M, D, psplit, pbias, *, production=False, rows=None, ldx=None, slack=8):
    """x [rows, ldx], planes [psplit, rows D + slack] or None, pbias [D] or None, ln_w, ln_b [D].  production: x is plane 0 of a split sum, `psplit` further
    planes follow, no bias (step.cpp after a split linear2).  const: every operand row is one dyadic constant, so the updated row is too."""
    rng = np.random.default_rng(seed)
    rows, ldx = rows or M + 3, ldx or (D if production else D + 4)
    x = np.full((rows, ldx), JUNK, F32)
    pl = np.full((psplit, rows * D + slack), JUNK, F32) if psplit else None
    pb = None
    if FAMILIES[family] is None:
        x[:M, :D] = rng.integers(-16, 17, (M, 1)) / 8.0
        for z in range(psplit):
            pl[z, :M * D] = np.repeat(rng.integers(-16, 17, M) / 8.0, D)
        if pbias:
            pb = np.full(D, rng.integers(-16, 17) / 8.0, F32)
    else:
        mean, sigma = FAMILIES[family]
        x[:M, :D] = mean + sigma * rng.standard_normal((M, D))
        for z in range(psplit):
            pl[z, :M * D] = (0.3 * sigma * rng.standard_normal(M * D))
        if pbias:
            pb = (0.1 * sigma * rng.standard_normal(D)).astype(F32)
    lw = (1.0 + 0.1 * rng.standard_normal(D)).astype(F32)
    lb = (0.1 * rng.standard_normal(D)).astype(F32)
    return x, pl, (None if production else pb), lw, lb


def updated_rows(x, pl, pb, M, D):
    """x + (((p0 + p1) + ...) + pbias) in f32, in the kernel's order; x itself without planes"""
    xs = np.ascontiguousarray(x[:M, :D])
    if pl is None:
        return xs
    ps = pl[0, :M * D].reshape(M, D).copy()
    for z in range(1, pl.shape[0]):
        ps = ps + pl[z, :M * D].reshape(M, D)
    if pb is not None:
        ps = ps + pb
    return xs + ps


def layernorm64(xs, lw, lb, eps):
    x = xs.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)      # biased, linear.go:295-309
    return (x - mu) / np.sqrt(var + eps) * lw.astype(np.float64) + lb.astype(np.float64)


def layernorm_f32(xs, lw, lb, eps):
    """k_rowprep's arithmetic in f32 (sums in f32, 1 / D and 1 / sqrt as one rounded operation each, (x - mean) inv_std, then w and b); the order of the sums
    over the row is numpy's, not the kernel's"""
    x = xs.astype(F32)
    rk = F32(1.0) / F32(x.shape[1])
    mean = x.sum(axis=1, keepdims=True, dtype=F32) * rk
    dx = x - mean
    var = (dx * dx).sum(axis=1, keepdims=True, dtype=F32) * rk
    inv = F32(1.0) / np.sqrt(var + F32(eps), dtype=F32)
    return (dx * inv) * lw + lb


def ln_close(y, want):
    """every element within LN_TOL of the f64 LayerNorm; returns the worst error / allowance"""
    err = np.abs(np.asarray(y, np.float64) - want)
    return float((err / (LN_TOL[0] + LN_TOL[1] * np.abs(want))).max())


def _prep_cases():
    fams = list(FAMILIES)
    cases, i = [], 0
    for D in (512, 1024):
        for M in (1, 3, 4, 5, 130, 256):
            for rep in range(2):   # two cases per (D, M); the other axes cycle at different periods (test_tall_ref.py checks what that covers)
                psplit = (0, 1, 3, 5)[(i + i // 4) % 4]
                cases.append(dict(D=D, M=M, psplit=psplit, pbias=bool(psplit) and (i // 2) % 2 == 0, production=False, family=fams[i % 4],
                                  want_x=(i % 3 != 2), want_y=(i % 5 != 1)))
                i += 1
    for D, M, fam in ((1024, 130, "normal"), (1024, 256, "offset"), (512, 5, "small"), (512, 129, "const")):
        cases.append(dict(D=D, M=M, psplit=3, pbias=False, production=True, family=fam, want_x=True, want_y=True))
    return cases


PREP_CASES = _prep_cases()


def prep_id(c):
    return (f"D{c['D']}-M{c['M']}-p{c['psplit']}" + ("+b" if c["pbias"] else "") + ("-prod" if c["production"] else "") + f"-{c['family']}" +
            ("" if c["want_x"] else "-nox") + ("" if c["want_y"] else "-noy"))
