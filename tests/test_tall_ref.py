"""What tests/test_gpu_tall.py rests on, checked without a GPU: the exact operands are exact, the case lists cover what they say, and the LayerNorm
tolerance has room for k_rowprep's f32 arithmetic on every row family the GPU tests use."""
import numpy as np
import pytest

from _kernel_ref import F32
from _tall_ref import (EPI_RESADD, FAMILIES, PREP_CASES, SPLIT_CASES, TALL_AXES, TALL_CASES, exact_condition, exact_operands, layernorm64, layernorm_f32,
                       ln_close, prep_id, prep_operands, ss_slices, tall_id, updated_rows)


def test_tall_cases_cover_every_value_with_both_forms():
    Ms, Ns, Ks, kinds = TALL_AXES
    assert 40 <= len(TALL_CASES) <= 60 and len({tall_id(c) for c in TALL_CASES}) == len(TALL_CASES)
    for form in (32, 64):
        seen = [c for c in TALL_CASES if c["form"] == form]
        assert {c["M"] for c in seen} == set(Ms) and {c["N"] for c in seen} == set(Ns) and {c["K"] for c in seen} == set(Ks)
        assert {(c["epi"], c["planes"], c["bias"]) for c in seen} == {(e, p, b) for e, p in kinds for b in (True, False)}
    # the LDS ring (3 stages at 64 rows, 5 at 32): fewer chunks than stages, exactly as many, and more
    assert {K // 128 for K in Ks} >= {1, 2, 3, 4, 5, 6}


def test_split_cases_have_uneven_and_empty_slices():
    assert ss_slices(128, 2) == [(0, 128), (128, 128)]
    assert ss_slices(640, 4) == [(0, 256), (256, 512), (512, 640), (640, 640)]
    assert ss_slices(640, 2) == [(0, 384), (384, 640)]
    assert ss_slices(768, 3) == [(0, 256), (256, 512), (512, 768)]
    for form in (32, 64):
        assert {(c["K"], c["S"]) for c in SPLIT_CASES if c["form"] == form} == {(128, 2), (640, 2), (640, 4), (768, 3), (1024, 4), (4096, 4)}
    assert {(c["M"], c["full"]) for c in SPLIT_CASES} == {(33, True), (33, False), (129, True), (129, False)}


@pytest.mark.parametrize("c", TALL_CASES + SPLIT_CASES, ids=tall_id)
def test_exact_operands_are_exact(c):
    """the premises hold, and f32 sums of hi and lo apart in two different orders equal the f64 product bit for bit"""
    M, N, K = c["M"], c["N"], c["K"]
    full = c.get("full", c.get("epi") == EPI_RESADD)
    x, cc, d, W, b, R = exact_operands(7, M, N, K, bias=c.get("bias", full), residual=full)
    assert exact_condition(x, cc, d, W, b, R, M, N, K) < 24.0
    want = (cc.astype(np.float64) + d.astype(np.float64)) @ W.astype(np.float64).T
    fwd = np.zeros((M, N), F32), np.zeros((M, N), F32)
    rev = np.zeros((M, N), F32), np.zeros((M, N), F32)
    for k0 in range(0, K, 32):
        k1 = K - k0 - 32
        for acc, ks, src in ((fwd[0], k0, cc), (fwd[1], k0, d), (rev[0], k1, cc), (rev[1], k1, d)):
            acc += src[:, ks:ks + 32] @ W[:, ks:ks + 32].T
    for h, l in (fwd, rev):
        assert np.array_equal((h + l).astype(np.float64), want)


@pytest.mark.parametrize("c", PREP_CASES, ids=prep_id)
def test_rowprep_emulation_stays_within_half_the_layernorm_tolerance(c):
    """k_rowprep's arithmetic, emulated in numpy f32, against the f64 LayerNorm of the same updated rows: at most half of LN_TOL on every family"""
    x, pl, pb, lw, lb = prep_operands(11, c["family"], c["M"], c["D"], c["psplit"], c["pbias"], production=c["production"])
    xs = updated_rows(x, pl, pb, c["M"], c["D"])
    assert np.isfinite(xs).all() and xs.dtype == F32
    want = layernorm64(xs, lw, lb, 1e-5)
    emu = layernorm_f32(xs, lw, lb, 1e-5)
    assert ln_close(emu, want) <= 0.5, (prep_id(c), ln_close(emu, want))
    if FAMILIES[c["family"]] is None:
        assert np.array_equal(emu, np.broadcast_to(lb, emu.shape)) and (xs == xs[:, :1]).all()


def test_row_families_are_what_they_say():
    assert {c["family"] for c in PREP_CASES if c["D"] == 512} == set(FAMILIES) == {c["family"] for c in PREP_CASES if c["D"] == 1024}
    for D in (512, 1024):
        seen = [c for c in PREP_CASES if c["D"] == D and not c["production"]]
        assert {c["M"] for c in seen} == {1, 3, 4, 5, 130, 256} and {c["psplit"] for c in seen} == {0, 1, 3, 5}
        assert {c["pbias"] for c in seen if c["psplit"]} == {True, False}
        assert {c["want_x"] for c in seen} == {True, False} == {c["want_y"] for c in seen}
        assert any(c["production"] for c in PREP_CASES if c["D"] == D)
    # sigma 0.01: eps = 1e-5 against a variance of 1e-4 moves y by about 5 %
    x, _, _, lw, lb = prep_operands(3, "small", 64, 1024, 0, False)
    xs = x[:64, :1024]
    moved = np.abs(layernorm64(xs, lw, lb, 1e-5) - layernorm64(xs, lw, lb, 0.0)) / np.abs(layernorm64(xs, lw, lb, 0.0) - lb)
    assert 0.03 < float(np.median(moved)) < 0.07
    # an unbiased variance (1 / (D - 1)) is outside LN_TOL on N(0, 1) rows of 512: the y_out check sees that slip
    x, _, _, lw, lb = prep_operands(4, "normal", 64, 512, 0, False)
    xs = x[:64, :512].astype(np.float64)
    mu = xs.mean(axis=1, keepdims=True)
    slipped = (xs - mu) / np.sqrt(((xs - mu) ** 2).sum(axis=1, keepdims=True) / 511.0 + 1e-5) * lw + lb
    assert ln_close(slipped, layernorm64(x[:64, :512], lw, lb, 1e-5)) > 1.0
