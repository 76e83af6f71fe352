"""The true-peak ceiling on the GPU (go-pocket-tts_amd/csrc/true_peak.hip k_tp_peak, k_tp_scale; true_peak.h):
ptts_true_peak_rows gives the bits of ptts_true_peak whatever rows share the launch; a request's ceiling (ptts_dsp_opts.ext) is
ptts_true_peak_limit of what the chain in front of it made of the request's own audio, bit for bit, in front of the egress; requests without a
ceiling launch what they launched."""
import json
import math
import os

import numpy as np
import pytest

import _eq_ref as E
import _true_peak_ref as T
import test_gpu_dsp as TD   # the egress relations and their bounds (_check_dc, _convert), the dispatcher and raw-call helpers
import test_gpu_eq as TE    # the host statement of the chain in front of the ceiling
from test_gpu_loudness import tiny  # noqa: F401  (the tiny model with audible output: loudness can be measured on it)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 25, 26, 27, 53, 54, 55, 1919, 1920, 1921, 3841, 124801]      # 124801: 65 tiles and one sample
STEPS = [7, 3, 9, 6, 12, 5]
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)
TARGET = -1600
BOOST = [(E.PEAKING, 1000.0, 18.0, 0.7)]         # behind the loudness gain (which holds the sample peak at 1) this is what the ceiling has to act on


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _db(v):
    return 20.0 * math.log10(float(v))


def _under(tp, by_db=6.0):
    """A ceiling by_db under a true peak, inside the range of the header."""
    return min(max(_db(tp) - by_db, -60.0), 0.0)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _record(case, observed, bound):
    out = os.environ.get("PTTS_TP_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": case, "observed": observed, "bound": bound, "observed_over_bound": observed / bound}) + "\n")


@pytest.fixture(scope="module")
def rows():
    x = E.signal(max(LENGTHS), seed=31)
    mine = [x[:n] for n in LENGTHS]
    bursts = [T.burst(3000, 0, seed=1), T.burst(4000, 1900, seed=2), T.burst(3841, 3801, seed=3)]     # the first 40, across a tile boundary, the last 40
    nan = E.signal(2500, seed=4)
    nan[1930] = np.nan
    return mine, bursts, nan


def test_rows_are_the_host_bits(pkg, tiny, rows):  # noqa: F811
    """Every length alone, all beside each other, and in the other order; bursts whose crest lies between samples; a NaN."""
    _, gm = tiny
    rt = pkg.runtime
    mine, bursts, nan = rows
    h = T.taps(pkg)
    for x in bursts:
        assert rt.true_peak(x) > 1.01 * float(np.abs(x).max())           # the case cannot pass on the sample peak alone
        assert abs(float(rt.true_peak(x)) - T.true_peak(x, h)) <= T.y_bound(x, h)
    table = mine + bursts + [nan]
    want = [rt.true_peak(x) for x in table]
    assert np.isfinite(want[-1]) and want[-1] > 0
    for x, w in zip(table, want):
        got = gm.true_peak_rows(x)
        assert _u32(got) == _u32(w), (x.size, float(got), float(w))
    for order in (slice(None), slice(None, None, -1)):
        got = gm.true_peak_rows(table[order])
        assert np.array_equal(_u32(got), _u32(np.array(want[order], np.float32))), [x.size for x in table[order]]
    worst = 0.0
    for x in mine[1:] + bursts:                                           # what the GPU run observes of the host meter against its float64 restatement
        worst = max(worst, float(np.abs(rt.true_peak_oversample(x).astype(np.float64) - T.oversample(x, h)).max()) / T.y_bound(x, h))
    print(f"largest |host y - ref y| over its bound: {worst:.3f}")
    _record("host y against the float64 restatement, worst row", worst, 1.0)
    assert worst <= 1.0


def _ext_opts(rt, ext, **kw):
    o = rt.DspOpts(1 if kw.get("normalize") else 0, 1 if kw.get("dc_block") else 0, float(kw.get("fade_in_ms", 0.0)), float(kw.get("fade_out_ms", 0.0)))
    if kw.get("eq") is not None:
        o.eq = kw["eq"].h
    o.ext = ext.h
    return o


def test_dsp_rows_take_the_ceiling(pkg, tiny, rows):  # noqa: F811
    _, gm = tiny
    rt = pkg.runtime
    mine, bursts, _ = rows
    S = T.gain_sum(T.taps(pkg))
    eq = rt.Eq(E.CASCADES["s2"])
    for x in (mine[10], mine[12], bursts[1]):
        x = (np.float32(0.5) * x).astype(np.float32)            # under 0 dBTP, so that a ceiling of 0 dBTP lies above it
        tp = rt.true_peak(x)
        low, high = rt.DspExt(true_peak_dbtp=_under(tp)), rt.DspExt(true_peak_dbtp=0.0)
        assert tp < 1.0
        # the ceiling alone: ptts_true_peak_limit's bits; a ceiling above the true peak: the input's bits
        want = rt.true_peak_limit(x, _under(tp))[0]
        got = gm.dsp_rows(x, opts=_ext_opts(rt, low))
        assert not np.array_equal(_u32(want), _u32(x)) and np.array_equal(_u32(got), _u32(want)), x.size
        again, c = float(rt.true_peak(got)), float(np.float32(10.0 ** (_under(tp) / 20.0)))
        bound = (2 * T.K + 3) * T.EPS * S
        print(f"n={x.size}: true peak {float(tp):.6f} -> {again:.6f}, ceiling {c:.6f}, excess {again / c - 1.0:+.2e} (bound {bound:.2e})")
        _record(f"ceiling excess n={x.size}", max(again / c - 1.0, 0.0), bound)
        assert again <= c * (1.0 + bound)
        assert np.array_equal(_u32(gm.dsp_rows(x, opts=_ext_opts(rt, high))), _u32(x)), x.size
        # behind normalise, an equaliser and the fades: the host statement, bit for bit
        chain = rt.dsp_apply(eq.apply(rt.dsp_apply(x, normalize=True)), **FADES)
        c_db = _under(rt.true_peak(chain))
        both = rt.DspExt(true_peak_dbtp=c_db)
        want = rt.true_peak_limit(chain, c_db)[0]
        got = gm.dsp_rows(x, opts=_ext_opts(rt, both, normalize=True, eq=eq, **FADES))
        assert not np.array_equal(_u32(want), _u32(chain)) and np.array_equal(_u32(got), _u32(want)), x.size
        # with the DC block: within the DC block's bound
        chain = rt.dsp_apply(eq.apply(rt.dsp_apply(x, normalize=True, dc_block=True)), **FADES)
        want = rt.true_peak_limit(chain, c_db)[0]
        got = gm.dsp_rows(x, opts=_ext_opts(rt, both, normalize=True, dc_block=True, eq=eq, **FADES))
        TD._check_dc(pkg, gm, got, want, "f32", 0, f"rows n={x.size} normalise+dc+eq+fades+ceiling")
        # several rows, one of them empty, in one launch sequence
        got = gm.dsp_rows([x, np.zeros(0, np.float32), x[:1000]], opts=_ext_opts(rt, low))
        assert np.array_equal(_u32(got[0]), _u32(rt.true_peak_limit(x, _under(tp))[0])) and got[1].size == 0
        assert np.array_equal(_u32(got[2]), _u32(rt.true_peak_limit(x[:1000], _under(tp))[0]))
        for e in (low, high, both):
            e.free()
    eq.free()


def _before_ceiling(pkg, base, boost):
    return [TE._statement(pkg, b.pcm, boost, loudness=TARGET) for b in base]


def test_generated_requests_are_the_host_statement(pkg, tiny):  # noqa: F811
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4): loudness and a boosting equaliser, then the ceiling -- a handle
    6 dB under each even request's own true peak, one handle at 0 dBTP shared by the odd ones."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    boost = rt.Eq(BOOST)
    base = gm.generate_batch(toks, [TD._cfg(pkg, s) for s in STEPS])
    pre = _before_ceiling(pkg, base, boost)
    tps = [float(rt.true_peak(p)) for p in pre]
    ceil = [0.0 if i % 2 else _under(tp) for i, tp in enumerate(tps)]
    acts = [tp > float(np.float32(10.0 ** (c / 20.0))) for tp, c in zip(tps, ceil)]
    print("true peaks behind the equaliser (dBTP):", [round(_db(tp), 2) for tp in tps], "ceilings:", [round(c, 2) for c in ceil], "acts:", acts)
    assert any(acts)                                             # the ceiling is what acts: the case cannot pass vacuously
    want24 = [rt.true_peak_limit(p, c)[0] for p, c in zip(pre, ceil)]
    assert any(not np.array_equal(_u32(w), _u32(p)) for w, p in zip(want24, pre))
    zero = rt.DspExt(true_peak_dbtp=0.0)
    own = [None if i % 2 else rt.DspExt(true_peak_dbtp=c) for i, c in enumerate(ceil)]

    def opts(i):
        o = rt.DspOpts()
        o.eq = boost.h
        o.ext = (own[i] or zero).h
        return o
    for fmt, rate in (("f32", 0), ("s16", 16000), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET, dsp_opts=opts(i)) for i, s in enumerate(STEPS)])
        for i, (b, g, w) in enumerate(zip(base, got, want24)):
            want = TD._convert(pkg, gm, w, fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, i, b.n_frames)
    # the keyword of the generate config makes and keeps a handle of its own
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, loudness=TARGET, eq=boost, true_peak_dbtp=c) for s, c in zip(STEPS, ceil)])
    for g, w in zip(got, want24):
        assert np.array_equal(_u32(g.pcm), _u32(w))
    # ceiling requests beside plain ones: the plain ones keep their bits
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, **(dict(loudness=TARGET, eq=boost, true_peak_dbtp=c) if i % 3 else {}))
                                     for i, (s, c) in enumerate(zip(STEPS, ceil))])
    for i, (b, m, w) in enumerate(zip(base, mixed, want24)):
        assert np.array_equal(_u32(m.pcm), _u32(w if i % 3 else b.pcm)), i
    # the ceiling as the only switch
    alone = [_under(rt.true_peak(b.pcm)) for b in base]
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, true_peak_dbtp=c) for s, c in zip(STEPS, alone)])
    for b, g, c in zip(base, got, alone):
        want = rt.true_peak_limit(b.pcm, c)[0]
        assert not np.array_equal(_u32(want), _u32(b.pcm)) and np.array_equal(_u32(g.pcm), _u32(want)), b.n_frames
    for e in own + [zero]:
        if e is not None:
            e.free()
    boost.free()


@pytest.mark.parametrize("continuous", [False, True])
def test_dispatcher_serves_ceiling_eq_and_plain_requests_mixed(pkg, tiny, continuous):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    boost, s3 = rt.Eq(BOOST), rt.Eq(E.CASCADES["s3"])
    steps = [7, 6, 9, 5]
    toks = _toks(len(steps))
    own = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s) for s in steps], continuous)
    pre0 = TE._statement(pkg, own[0].pcm, boost, loudness=TARGET)
    c0, c3 = _under(rt.true_peak(pre0)), _under(rt.true_peak(own[3].pcm))
    specs = [(7, "f32", 0, dict(loudness=TARGET, eq=boost, true_peak_dbtp=c0)), (6, "ulaw", 8000, dict(eq=s3, fade_out_ms=80.0)), (9, "f32", 0, None),
             (5, "s16", 16000, dict(true_peak_dbtp=c3))]
    got = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs], continuous)
    off = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r) for s, f, r, _ in specs], continuous)
    host = [rt.true_peak_limit(pre0, c0)[0], TE._statement(pkg, own[1].pcm, s3, fade_out_ms=80.0), None, rt.true_peak_limit(own[3].pcm, c3)[0]]
    assert not np.array_equal(_u32(host[0]), _u32(pre0))
    for i, (s, f, r, sw) in enumerate(specs):
        assert got[i].n_frames == s
        if sw is None:
            assert np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i
            continue
        assert np.array_equal(TD._bits(got[i].pcm), TD._bits(TD._convert(pkg, gm, host[i], f, r))), (i, f, r)
        assert not np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i
    boost.free()
    s3.free()


def _dsp_census(counts):
    return {k: v for k, v in counts.items() if k.startswith(("k_tp", "k_eq", "k_dsp", "k_loud")) or k == "k_resample"}


def test_launch_census(pkg, tiny, rows):  # noqa: F811
    """A batch with a ceiling row: k_tp_peak and k_tp_scale once for the decoded group, behind the table's other kernels.  The measurement:
    k_tp_peak alone.  Without the handle: the parent's census."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [5, 9, 13]]
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, true_peak_dbtp=-1.0), TD._cfg(pkg, 6)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_apply": 1, "k_tp_peak": 1, "k_tp_scale": 1, "k_resample": 1}
    eq = rt.Eq(E.CASCADES["s4"])
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, loudness=TARGET, eq=eq, true_peak_dbtp=-1.0, **FADES), TD._cfg(pkg, 6, dc_block=True)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_peak": 1, "k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1,
                                                    "k_dsp_summary": 1, "k_dsp_carry": 1, "k_dsp_apply": 1, "k_eq_summary": 1, "k_eq_carry": 1,
                                                    "k_eq_apply": 1, "k_tp_peak": 1, "k_tp_scale": 1, "k_resample": 1}
    rt.launch_counts(True)
    gm.true_peak_rows(rows[0][8:12])
    assert _dsp_census(rt.launch_counts(False)) == {"k_tp_peak": 1}
    # without the handle: what the parent launched
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
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, eq=eq), TD._cfg(pkg, 6)])
    assert _dsp_census(rt.launch_counts(False)) == {"k_dsp_apply": 1, "k_eq_summary": 1, "k_eq_carry": 1, "k_eq_apply": 1, "k_resample": 1}
    eq.free()


def test_refusals_name_the_field_and_the_others_run(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm
    cb = lambda off, x: None  # noqa: E731
    dead = rt.DspExt(true_peak_dbtp=-1.0)
    freed = rt.DspOpts()
    freed.ext = dead.h
    dead.free()
    for kw, field in [(dict(true_peak_dbtp=-1.0, pcm_callback=cb), "ext"), (dict(dsp_opts=freed), "dsp: ext")]:
        rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, **kw), TD._cfg(pkg, 4)])
        assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and field in msg and "dsp" in msg, (field, rc, msg)
        assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32)), field
    with pytest.raises(pkg.PttsError) as ei:
        gm.dsp_rows(np.ones(10, np.float32), opts=freed)
    assert ei.value.code == rt.PTTS_EINVAL and "dsp: ext" in str(ei.value) and "reserved[2..3]" in str(ei.value)
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500, continuous=True, cont_kv_capacity=64, cont_max_steps=32)
    try:
        for kw, field in [(dict(dsp_opts=freed), "dsp: ext"), (dict(true_peak_dbtp=-1.0, pcm_callback=cb), "ext")]:
            with pytest.raises(pkg.PttsError) as ei:
                d.generate(toks[0], TD._cfg(pkg, 4, **kw))
            assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value) and "dsp" in str(ei.value), (field, str(ei.value))
        assert np.array_equal(_u32(d.generate(toks[1], TD._cfg(pkg, 4)).pcm), _u32(good))
    finally:
        d.close()
