"""The host-rows entry points of include/ptts.h (ptts_dsp_rows, ptts_eq_rows, ptts_compress_rows, ptts_limit_rows, ptts_loudness_rows,
ptts_loudness_normalize_rows, ptts_true_peak_rows; ptts_resample and ptts_pcm_encode beside them) as one round trip: pack, upload, launch, download.  What each of them
promises at its edges -- rows that alias their outputs, calls with nothing in them, rows that share a call, tables that fill up, and the
launches of a call -- through the public ABI and the launch census alone."""
import ctypes as C

import numpy as np
import pytest

import _eq_ref as E
from test_gpu_dsp import tiny  # noqa: F401

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
TARGET = -16.0
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return len(got) == len(want) and all(g.size == w.size and np.array_equal(_u32(g), _u32(w)) for g, w in zip(got, want))


def _census(counts):
    return {k: v for k, v in counts.items() if k.startswith(("k_tp", "k_eq", "k_dsp", "k_loud")) or k == "k_resample"}


def _rows(lengths, seed):
    x = E.signal(max(lengths) + len(lengths), seed=seed)
    return [x[k:k + n].copy() for k, n in enumerate(lengths)]


def _raw(gm, rows, outs):
    n = len(rows)
    ns = np.array([r.size for r in rows], np.int64)
    pp = (FP * n)(*[C.cast(r.ctypes.data, FP) for r in rows])
    po = (FP * n)(*[C.cast(o.ctypes.data, FP) for o in outs])
    return C.c_void_p(gm.h), pp, ns.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(n), po, ns


@pytest.fixture(scope="module")
def chain(pkg):
    """Everything a ptts_dsp_opts switches on at once: normalise, DC block, both fades, an equaliser and a ceiling."""
    rt = pkg.runtime
    eq = rt.Eq(E.CASCADES["s4"])
    ext = rt.DspExt(true_peak_dbtp=-3.0)
    o = rt.DspOpts(1, 1, 50.0, 80.0)
    o.eq = eq.h
    o.ext = ext.h
    yield o, eq
    eq.free()
    ext.free()


def test_rows_may_alias_their_outputs(pkg, tiny, chain):  # noqa: F811
    """out[i] == in[i] gives what separate outputs give, as uint32 images."""
    _, gm = tiny
    rt = pkg.runtime
    L = rt.lib()
    rows = _rows([1921, 0, 29, 9601, 1920], seed=11)
    opts, eq = chain
    for o in (opts, rt.DspOpts()):
        want = gm.dsp_rows(rows, opts=o)
        mine = [r.copy() for r in rows]
        h, pp, ns, n, po, _keep = _raw(gm, mine, mine)
        assert L.ptts_dsp_rows(h, pp, ns, n, C.byref(o), po) == rt.PTTS_OK, L.ptts_last_error()
        assert _same(mine, want)
    assert _same(gm.dsp_rows(rows, opts=rt.DspOpts()), rows)
    which = [eq, eq, None, eq, None]
    want = gm.eq_rows(rows, which)
    assert _same([want[2], want[4]], [rows[2], rows[4]]) and not np.array_equal(_u32(want[3]), _u32(rows[3]))
    mine = [r.copy() for r in rows]
    h, pp, ns, n, po, _keep = _raw(gm, mine, mine)
    pe = (C.c_void_p * len(rows))(*[e.h if e is not None else None for e in which])
    assert L.ptts_eq_rows(h, pe, pp, ns, n, po) == rt.PTTS_OK, L.ptts_last_error()
    assert _same(mine, want)
    want, want_lufs = gm.loudness_normalize_rows(rows, TARGET)
    assert not np.array_equal(_u32(want[3]), _u32(rows[3]))
    mine = [r.copy() for r in rows]
    h, pp, ns, n, po, _keep = _raw(gm, mine, mine)
    lufs = np.zeros(len(rows), np.float64)
    assert L.ptts_loudness_normalize_rows(h, pp, ns, n, C.c_double(TARGET), po, lufs.ctypes.data_as(C.POINTER(C.c_double))) == rt.PTTS_OK, L.ptts_last_error()
    assert _same(mine, want) and np.array_equal(lufs.view(np.uint64), np.asarray(want_lufs, np.float64).view(np.uint64))


@pytest.mark.parametrize("rows", [[], [np.zeros(0, np.float32)] * 3], ids=["no rows", "rows of length 0"])
def test_empty_calls_launch_nothing(pkg, tiny, chain, rows):  # noqa: F811
    _, gm = tiny
    rt = pkg.runtime
    opts, eq = chain
    rt.launch_counts(True)
    a = gm.dsp_rows(rows, opts=opts)
    b = gm.dsp_rows(rows, opts=rt.DspOpts())
    c = gm.eq_rows(rows, eq)
    d, d_lufs = gm.loudness_normalize_rows(rows, TARGET)
    lufs = gm.loudness_rows(rows)
    peaks = gm.true_peak_rows(rows)
    assert _census(rt.launch_counts(False)) == {}
    for got in (a, b, c, d):
        assert len(got) == len(rows) and all(g.size == 0 for g in got)
    assert len(lufs) == len(d_lufs) == len(peaks) == len(rows)
    assert all(v == -np.inf for v in lufs) and all(v == -np.inf for v in d_lufs) and all(_u32(v) == 0 for v in peaks)


def test_one_chain_whatever_rows_share_the_call(pkg, tiny, chain):  # noqa: F811
    """Every switch of a ptts_dsp_opts at once, and one equaliser per row: a row alone, among the others, and in another order gives the same bits."""
    _, gm = tiny
    opts, _ = chain
    rows = _rows([1, 1919, 1921, 9601], seed=12)
    alone = [gm.dsp_rows(r, opts=opts) for r in rows]
    assert not np.array_equal(_u32(alone[3]), _u32(rows[3]))
    assert _same(gm.dsp_rows(rows, opts=opts), alone)
    assert _same(gm.dsp_rows(rows[::-1], opts=opts), alone[::-1])
    eqs = [pkg.runtime.Eq(E.CASCADES[k]) for k in ("s1", "s2", "s4")]
    which = [eqs[0], None, eqs[2], eqs[1]]
    alone = [gm.eq_rows([r], [e])[0] for r, e in zip(rows, which)]
    assert _same(alone, [e.apply(r) if e is not None else r for r, e in zip(rows, which)])
    assert _same(gm.eq_rows(rows, which), alone)
    assert _same(gm.eq_rows(rows[::-1], which[::-1]), alone[::-1])
    for e in eqs:
        e.free()


def test_a_call_larger_than_one_table(pkg, tiny):  # noqa: F811
    """257 rows with 17 distinct equalisers: more rows than one table holds (256), more equalisers than travel behind one (16)."""
    _, gm = tiny
    rt = pkg.runtime
    eqs = [rt.Eq([(E.PEAKING, 200.0 + 150.0 * i, 3.0, 1.0)]) for i in range(17)]
    x = E.signal(257 + 30, seed=13)
    rows = [x[i:i + 30].copy() for i in range(257)]
    which = [eqs[i % 17] for i in range(257)]
    rt.launch_counts(True)
    got = gm.eq_rows(rows, which)
    counts = _census(rt.launch_counts(False))
    assert counts.get("k_eq_apply", 0) == 17, counts   # greedy: the 17th equaliser starts the next table, so sixteen tables of 16 rows and one of 1
    assert _same(got, [e.apply(r) for r, e in zip(rows, which)])
    for e in eqs:
        e.free()
    rows = [x[i:i + 27].copy() for i in range(257)]
    got = gm.true_peak_rows(rows)
    assert np.array_equal(_u32(got), _u32(np.array([rt.true_peak(r) for r in rows], np.float32)))


def _peak_db(rows):
    return 20.0 * np.log10(min(float(np.abs(r).max()) for r in rows))


def test_compress_rows_larger_than_one_table(pkg, tiny):  # noqa: F811
    """257 rows with 17 distinct compressors: the compressor's own table cuts, at the 257th row and at the 17th design."""
    _, gm = tiny
    rt = pkg.runtime
    cs = [rt.CompressorOpts(threshold_db=-60.0 + i) for i in range(17)]
    x = E.signal(257 + 30, seed=15)
    rows = [x[i:i + 30].copy() for i in range(257)]
    assert _peak_db(rows) > -44.0 + 6.0   # every row's peak lies above every threshold and knee
    which = [cs[i % 17] for i in range(257)]
    rt.launch_counts(True)
    got = gm.compress_rows(rows, which)
    counts = rt.launch_counts(False)
    assert {k: v for k, v in counts.items() if k.startswith("k_cmp")} == {"k_cmp_carry_p": 17, "k_cmp_carry_s": 17, "k_cmp_apply": 17}, counts
    want = [rt.compress_apply(c, r) for r, c in zip(rows, which)]
    assert _same(got, want)
    assert not any(np.array_equal(_u32(w), _u32(r)) for w, r in zip(want, rows))
    assert len({_u32(rt.compress_apply(c, rows[0])).tobytes() for c in cs}) == 17   # (17 designs that differ in what they do)


def test_limit_rows_larger_than_one_table(pkg, tiny):  # noqa: F811
    """257 rows with 17 distinct limiters: the limiter's own table cuts, at the 257th row and at the 17th design."""
    _, gm = tiny
    rt = pkg.runtime
    ls = [rt.LimiterOpts(ceiling_db=-60.0 + i) for i in range(17)]
    x = E.signal(257 + 30, seed=16)
    rows = [x[i:i + 30].copy() for i in range(257)]
    assert _peak_db(rows) > -44.0   # every row's peak lies above every ceiling
    which = [ls[i % 17] for i in range(257)]
    rt.launch_counts(True)
    got = gm.limit_rows(rows, which)
    counts = rt.launch_counts(False)
    assert {k: v for k, v in counts.items() if k.startswith("k_lim")} == {"k_lim_carry": 17, "k_lim_gain": 17, "k_lim_apply": 17}, counts
    want = [rt.limit_apply(l, r) for r, l in zip(rows, which)]
    assert _same(got, want)
    assert not any(np.array_equal(_u32(w), _u32(r)) for w, r in zip(want, rows))
    assert len({_u32(rt.limit_apply(l, rows[0])).tobytes() for l in ls}) == 17   # (17 designs that differ in what they do)


def test_a_mixed_call_gives_every_row_its_own_scratch(pkg, tiny):  # noqa: F811
    """40 rows of four lengths through every stage that takes scratch at once -- a compressor, normalise, DC block, fades, a limiter and a
    ceiling: the bits of the same rows one per call, so no row's states lie in another row's region."""
    _, gm = tiny
    rt = pkg.runtime
    ext = rt.DspExt(true_peak_dbtp=-9.0, compressor=rt.CompressorOpts(threshold_db=-30.0), limiter=rt.LimiterOpts(ceiling_db=-6.0))
    o = rt.DspOpts(1, 1, 50.0, 80.0)
    o.ext = ext.h
    rows = _rows([1, 1919, 1921, 9601] * 10, seed=17)
    got = gm.dsp_rows(rows, opts=o)
    alone = [gm.dsp_rows(r, opts=o) for r in rows]
    assert _same(got, alone)
    assert not np.array_equal(_u32(got[3]), _u32(gm.dsp_rows(rows[3], normalize=True, dc_block=True, **FADES)))   # (the ext's stages ran)
    ext.free()


def test_launch_census_of_every_entry_point(pkg, tiny):  # noqa: F811
    """The launches of one 3-row call of each rows entry point, of a resample and of a format conversion."""
    _, gm = tiny
    rt = pkg.runtime
    rows = _rows([1921, 9601, 29], seed=14)
    eq = rt.Eq(E.CASCADES["s2"])
    calls = [
        (lambda: gm.dsp_rows(rows, normalize=True, dc_block=True, **FADES), {"k_dsp_peak": 1, "k_dsp_summary": 1, "k_dsp_carry": 1, "k_dsp_apply": 1}),
        (lambda: gm.eq_rows(rows, eq), {"k_dsp_apply": 1, "k_eq_summary": 1, "k_eq_carry": 1, "k_eq_apply": 1}),
        (lambda: gm.loudness_rows(rows), {"k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1}),
        (lambda: gm.loudness_normalize_rows(rows, TARGET), {"k_dsp_peak": 1, "k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1,
                                                          "k_dsp_apply": 1}),
        (lambda: gm.true_peak_rows(rows), {"k_tp_peak": 1}),
        (lambda: gm.resample(rows, 24000, 8000), {"k_resample": 1}),
        (lambda: gm.pcm_encode(rows[1], rt.PCM_ULAW), {"k_resample": 1}),
    ]
    for at, (call, want) in enumerate(calls):
        rt.launch_counts(True)
        call()
        got = _census(rt.launch_counts(False))
        print(f"census {at}: {got}")
        assert got == want, (at, got)
    eq.free()
