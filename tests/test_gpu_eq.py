"""The per-request equaliser on the GPU (go-pocket-tts_amd/csrc/dsp.hip k_eq_*, scan_block.h): ptts_eq_rows and a request's
`eq` give the bits of ptts_eq_apply -- the host instantiation of the blocked form -- whatever rows share the launch; a request's result is the host
statement gain -> DC block -> equaliser -> fades -> egress of its own plain audio; requests without an equaliser launch what they launched."""
import numpy as np
import pytest

import _eq_ref as E
import test_gpu_dsp as TD   # the egress relations and their bounds (_check_dc, _convert), the dispatcher and raw-call helpers
from test_gpu_loudness import tiny  # noqa: F401  (the tiny model with audible output: loudness can be measured on it)

pytestmark = pytest.mark.gpu

FILL = [100 + 997 * i for i in range(64)]        # the 64 other rows of a shared launch: ragged, 100 .. 62911 samples
STEPS = [7, 3, 9, 6, 12, 5]
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)
TARGET = -1600


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


@pytest.fixture(scope="module")
def eqs(pkg):
    made = {name: pkg.runtime.Eq(secs) for name, secs in E.CASCADES.items()}
    yield made
    for e in made.values():
        e.free()


@pytest.fixture(scope="module")
def rows():
    x = E.signal(max(E.LENGTHS), seed=5)
    return [x[:n] for n in E.LENGTHS], [E.signal(m, seed=7) for m in FILL]


@pytest.mark.parametrize("name", ["s1", "s2", "s3", "s4", "corner"])
def test_rows_are_the_host_bits(pkg, tiny, eqs, rows, name):  # noqa: F811
    """Every length alone, among 64 other rows, and with the rows in another order."""
    _, gm = tiny
    eq = eqs[name]
    mine, others = rows
    want = [eq.apply(x) for x in mine]
    want_others = [eq.apply(x) for x in others]
    for x, w in zip(mine, want):
        got = gm.eq_rows(x, eq)
        assert got.size == x.size and np.array_equal(_u32(got), _u32(w)), (name, x.size)
        if x.size >= 1920:
            assert not np.array_equal(_u32(got), _u32(x))         # the filter ran
    table = others[:20] + mine + others[20:]
    want_table = want_others[:20] + want + want_others[20:]
    for order in (slice(None), slice(None, None, -1)):
        got = gm.eq_rows(table[order], eq)
        for g, w in zip(got, want_table[order]):
            assert g.size == w.size and np.array_equal(_u32(g), _u32(w)), (name, w.size)
    assert np.array_equal(_u32(eq.rows(gm, mine[7])), _u32(want[7]))


def test_one_table_with_different_equalisers_and_a_null_row(pkg, tiny, eqs, rows):  # noqa: F811
    _, gm = tiny
    mine, others = rows
    table = [mine[7], mine[10], others[3], mine[8], mine[11], others[40], np.zeros(0, np.float32)]
    which = [eqs["s2"], eqs["s4"], None, eqs["s4"], eqs["s1"], eqs["s3"], eqs["s1"]]
    got = gm.eq_rows(table, which)
    for x, e, g in zip(table, which, got):
        assert np.array_equal(_u32(g), _u32(e.apply(x) if e is not None else x)), x.size
    # more distinct equalisers than one table carries behind its rows (16): the rows go in two tables, the bits stay
    many = [pkg.runtime.Eq([(E.PEAKING, 200.0 + 150.0 * i, 3.0, 1.0)]) for i in range(20)]
    got = gm.eq_rows([mine[8]] * 20, many)
    for e, g in zip(many, got):
        assert np.array_equal(_u32(g), _u32(e.apply(mine[8])))
    rt = pkg.runtime
    dead = rt.Eq(E.CASCADES["s1"])
    h = dead.h
    dead.free()
    dead.h = h
    with pytest.raises(pkg.PttsError) as ei:
        gm.eq_rows([mine[7], mine[8]], [eqs["s1"], dead])
    dead.h = None
    assert ei.value.code == rt.PTTS_EINVAL and "eq" in str(ei.value) and "row 1" in str(ei.value)


def _statement(pkg, pcm, eq, loudness=0, normalize=False, dc_block=False, fade_in_ms=0.0, fade_out_ms=0.0):
    """The host statement of a request's 24 kHz result (include/ptts.h)."""
    rt = pkg.runtime
    x = rt.loudness_normalize(pcm, loudness / 100.0)[0] if loudness else rt.dsp_apply(pcm, normalize=normalize, dc_block=dc_block)
    if loudness and dc_block:
        x = rt.dsp_apply(x, dc_block=True)
    x = eq.apply(x)
    return rt.dsp_apply(x, fade_in_ms=fade_in_ms, fade_out_ms=fade_out_ms)


def test_generated_requests_are_the_host_statement(pkg, tiny, eqs):  # noqa: F811
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4), two equalisers in one call."""
    cfg, gm = tiny
    toks = _toks(len(STEPS))
    base = gm.generate_batch(toks, [TD._cfg(pkg, s) for s in STEPS])
    which = [eqs["s4"] if i % 2 else eqs["s2"] for i in range(len(STEPS))]
    moved = max(float(np.abs(e.apply(b.pcm) - b.pcm).max() / np.abs(b.pcm).max()) for b, e in zip(base, which))
    print(f"the equalisers move the tiny model's audio by {moved:.3e} of its peak")
    assert moved > 1e-3                                         # the case cannot pass vacuously
    for fmt, rate in (("f32", 0), ("s16", 16000), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, eq=e) for s, e in zip(STEPS, which)])
        for b, g, e in zip(base, got, which):
            want = TD._convert(pkg, gm, _statement(pkg, b.pcm, e), fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
    # loudness, the equaliser and the fades: still bit for bit
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, loudness=TARGET, eq=e, **FADES) for s, e in zip(STEPS, which)])
    for b, g, e in zip(base, got, which):
        want = _statement(pkg, b.pcm, e, loudness=TARGET, **FADES)
        assert np.array_equal(_u32(g.pcm), _u32(want)), b.n_frames
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, normalize=True, eq=e, **FADES) for s, e in zip(STEPS, which)])
    for b, g, e in zip(base, got, which):
        assert np.array_equal(_u32(g.pcm), _u32(_statement(pkg, b.pcm, e, normalize=True, **FADES))), b.n_frames
    # an equaliser request beside plain ones: the plain ones keep their bits
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, eq=e if i % 2 else None) for i, (s, e) in enumerate(zip(STEPS, which))])
    for i, (b, m, e) in enumerate(zip(base, mixed, which)):
        assert np.array_equal(_u32(m.pcm), _u32(e.apply(b.pcm) if i % 2 else b.pcm)), i
    # everything switched on, the DC block included: within the DC block's bounds
    for fmt, rate in (("f32", 0), ("s16", 0), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET, dc_block=True, eq=eqs["s2"], **FADES) for s in STEPS])
        for b, g in zip(base, got):
            host = _statement(pkg, b.pcm, eqs["s2"], loudness=TARGET, dc_block=True, **FADES)
            TD._check_dc(pkg, gm, g.pcm, host, fmt, rate, f"generate loudness+dc+eq+fades {fmt} {rate or 24000} Hz frames={b.n_frames}")


@pytest.mark.parametrize("continuous", [False, True])
def test_dispatcher_serves_eq_dsp_and_plain_requests_mixed(pkg, tiny, eqs, continuous):  # noqa: F811
    cfg, gm = tiny
    specs = [(7, "f32", 0, dict(eq=eqs["s2"])), (6, "ulaw", 8000, dict(eq=eqs["s3"], fade_out_ms=80.0)), (9, "f32", 0, None),
             (5, "s16", 16000, dict(normalize=True, fade_in_ms=50.0))]
    toks = _toks(len(specs))
    got = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs], continuous)
    off = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r) for s, f, r, _ in specs], continuous)
    own = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s) for s, _, _, _ in specs], continuous)
    for i, (s, f, r, sw) in enumerate(specs):
        assert got[i].n_frames == s
        if sw is None:
            assert np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i
            continue
        sw = dict(sw)
        eq = sw.pop("eq", None)
        host = _statement(pkg, own[i].pcm, eq, **sw) if eq is not None else pkg.runtime.dsp_apply(own[i].pcm, **sw)
        assert np.array_equal(TD._bits(got[i].pcm), TD._bits(TD._convert(pkg, gm, host, f, r))), (i, f, r)
        assert not np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i


def _dsp_census(counts):
    return {k: v for k, v in counts.items() if k.startswith("k_eq") or k.startswith("k_dsp") or k.startswith("k_loud") or k == "k_resample"}


def test_launch_census(pkg, tiny, eqs):  # noqa: F811
    """A batch with an equaliser row: the three k_eq_* launches once for the decoded group, behind k_dsp_apply.  Without one: the parent's census."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [5, 9, 13]]
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, eq=eqs["s4"]), TD._cfg(pkg, 6)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_apply": 1, "k_eq_summary": 1, "k_eq_carry": 1, "k_eq_apply": 1, "k_resample": 1}
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, eq=eqs["s4"], **TD.ALL4), TD._cfg(pkg, 6, eq=eqs["s1"])])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_peak": 1, "k_dsp_summary": 1, "k_dsp_carry": 1, "k_dsp_apply": 1, "k_eq_summary": 1,
                                                    "k_eq_carry": 1, "k_eq_apply": 1, "k_resample": 1}
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6), TD._cfg(pkg, 6, "s16")])
    assert _dsp_census(rt.launch_counts(False)) == {}
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, **TD.ALL4), TD._cfg(pkg, 6, fade_in_ms=5.0)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_peak": 1, "k_dsp_summary": 1, "k_dsp_carry": 1, "k_dsp_apply": 1, "k_resample": 1}
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, loudness=TARGET), TD._cfg(pkg, 6)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_peak": 1, "k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1,
                                                    "k_dsp_apply": 1, "k_resample": 1}


def test_refusals_name_the_field_and_the_others_run(pkg, tiny, eqs):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm
    cb = lambda off, x: None  # noqa: E731
    dead = rt.Eq(E.CASCADES["s1"])
    freed = rt.DspOpts()
    freed.eq = dead.h
    dead.free()
    res3 = rt.DspOpts()
    res3.eq = eqs["s1"].h
    res3.reserved[3] = 1
    for kw, field in [(dict(eq=eqs["s1"], pcm_callback=cb), "eq"), (dict(dsp_opts=freed), "dsp: eq"), (dict(dsp_opts=res3), "reserved")]:
        rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, **kw), TD._cfg(pkg, 4)])
        assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and field in msg and "dsp" in msg, (field, rc, msg)
        assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32)), field
    with pytest.raises(pkg.PttsError) as ei:
        gm.dsp_rows(np.ones(10, np.float32), opts=freed)
    assert ei.value.code == rt.PTTS_EINVAL and "dsp: eq" in str(ei.value)
    # ptts_dsp_rows takes the same options: the whole chain on host rows
    x = E.signal(5000, seed=9)
    live = rt.DspOpts(1, 0, 50.0, 80.0)
    live.eq = eqs["s3"].h
    want = rt.dsp_apply(eqs["s3"].apply(rt.dsp_apply(x, normalize=True)), fade_in_ms=50.0, fade_out_ms=80.0)
    assert np.array_equal(_u32(gm.dsp_rows(x, opts=live)), _u32(want))
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500, continuous=True, cont_kv_capacity=64, cont_max_steps=32)
    try:
        with pytest.raises(pkg.PttsError) as ei:
            d.generate(toks[0], TD._cfg(pkg, 4, dsp_opts=freed))
        assert ei.value.code == rt.PTTS_EINVAL and "dsp: eq" in str(ei.value)
    finally:
        d.close()
