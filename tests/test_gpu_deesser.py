"""The de-esser on the GPU (go-pocket-tts_amd/csrc/deesser.hip k_de_*; deesser.h): ptts_deess_rows gives the bits of
ptts_deess_apply whatever rows and designs share the launch; a request's de-esser (ptts_dsp_ext_set_deesser on the handle of ptts_dsp_opts.ext) is
ptts_deess_apply of the request's own audio, directly behind the compressor and in front of everything else, bit for bit, alone, in a whole
chain and over a joined call's audio; requests without one launch what they launched; where a row is handed over window after window the stage
is refused by name and nothing launches."""
import ctypes as C
import math

import numpy as np
import pytest

import _deesser_ref as R
import _eq_ref as E
import test_gpu_compressor as TC   # a compressor for the model's own level
import test_gpu_dsp as TD          # _cfg, the raw-call helper
import test_gpu_eq as TE           # the host statement of the chain behind the de-esser
import test_gpu_limiter as TL      # a limiter for the audio's own level
from test_gpu_loudness import tiny  # noqa: F401  (the tiny model with audible output, max_batch = 4)

pytestmark = pytest.mark.gpu

STEPS = [7, 3, 9, 6, 12, 5]
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)
BOOST = [(E.PEAKING, 4000.0, 9.0, 0.9)]     # the presence peak that raises sibilants
C_FP = C.POINTER(C.c_float)
DE_KERNELS = ("k_de_summary_b", "k_de_carry_b", "k_de_summary_p", "k_de_carry_p", "k_de_summary_s", "k_de_carry_s", "k_de_apply")
CMP_KERNELS = ("k_cmp_summary_p", "k_cmp_carry_p", "k_cmp_summary_s", "k_cmp_carry_s", "k_cmp_apply")
NEW_MESSAGE = "deesser is not carried from window to window yet"


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _opts(rt, name):
    return rt.DeesserOpts(*R.DESIGNS[name])


def _for_audio(rt, pcm, **kw):
    """A de-esser whose threshold lies 20 dB under the peak of the audio's own band, inside the header's range: it engages whatever the
    model's level."""
    kw.setdefault("freq_hz", 4000.0)
    peak = float(np.abs(rt.deess_band(rt.DeesserOpts(**kw), pcm)).max())
    assert peak > 0
    return rt.DeesserOpts(threshold_db=min(max(20.0 * math.log10(peak) - 20.0, -60.0), 0.0), ratio=8.0, knee_db=6.0, attack_ms=0.5, release_ms=40.0,
                          max_reduction_db=18.0, **kw)


def _bites(rt, d, pcm):
    """The de-essed audio, after the assertion that the stage moved it far above one f32 step at its peak."""
    y = rt.deess_apply(d, pcm)
    moved, bound = float(np.abs(y.astype(np.float64) - pcm).max()), E.bound(pcm)
    assert moved > 1000.0 * bound, (moved, bound)
    return y


def _census(counts, prefixes=("k_de", "k_lim", "k_cmp", "k_tp", "k_eq", "k_dsp", "k_loud")):
    return {k: v for k, v in counts.items() if k.startswith(prefixes)}


@pytest.fixture(scope="module")
def rows():
    """The engagement input cut to every length, and a row with a NaN inside a burst: computed once, never written to"""
    whole = R.engagement(max(R.GPU_LENGTHS))
    nan = np.array(whole[:3 * R.TILE + 5])
    nan[R.BURST_AT + 700] = np.nan
    for a in (whole, nan):
        a.setflags(write=False)
    return [whole[:n] for n in R.GPU_LENGTHS], nan


def test_rows_are_the_host_bits(pkg, tiny, rows):  # noqa: F811
    """Every length, two designs and a NULL row in one call; each design alone; the seven kernels in the census, each once."""
    _, gm = tiny
    rt = pkg.runtime
    by_len, nan = rows
    a, b = _opts(rt, "soft"), _opts(rt, "hard")
    # on the host first: the comparison bites
    for d in (a, b):
        for x in by_len:
            y = rt.deess_apply(d, x)
            if x.size >= 1919:                                   # (shorter rows end before the first burst has raised the level: they pass)
                assert not np.array_equal(_u32(y), _u32(x)), x.size
            else:
                assert np.array_equal(_u32(y), _u32(x)), x.size
            if x.size > R.TILE:                                  # a run from zero state per tile, the stateless form, gives other bits
                stateless = np.concatenate([rt.deess_apply(d, x[t:t + R.TILE]) for t in range(0, x.size, R.TILE)])
                assert not np.array_equal(_u32(stateless), _u32(y)), x.size
    _bites(rt, a, by_len[-1])
    assert not np.array_equal(_u32(rt.deess_apply(a, by_len[-1])), _u32(rt.deess_apply(b, by_len[-1])))
    # two designs and a row that is copied, in one call: the designs table
    table = by_len + [nan, by_len[-2], by_len[-1][:30000]]
    ds = [a if i % 2 else b for i in range(len(by_len))] + [a, None, b]
    want = [x if d is None else rt.deess_apply(d, x) for x, d in zip(table, ds)]
    assert np.isnan(want[len(by_len)]).any() and np.isfinite(want[len(by_len)][:R.BURST_AT + 700]).all()
    rt.launch_counts(True)
    got = gm.deess_rows(table, ds)
    assert _census(rt.launch_counts(False)) == {k: 1 for k in DE_KERNELS}
    for x, g, w in zip(table, got, want):
        if x is nan:                                             # where the NaNs are, and every other sample's bits (which NaN is the processor's)
            there = ~np.isnan(w)
            bad = np.flatnonzero(_u32(g)[there] != _u32(w)[there])
            assert np.array_equal(np.isnan(g), np.isnan(w)) and bad.size == 0, (int((np.isnan(g) != np.isnan(w)).sum()), int(bad.size))
            continue
        assert g.shape == w.shape and np.array_equal(_u32(g), _u32(w)), x.size
    # each design alone over every length, and in the other order
    for d, order in ((a, slice(None)), (b, slice(None, None, -1))):
        got = gm.deess_rows(by_len[order], d)
        for x, g in zip(by_len[order], got):
            assert np.array_equal(_u32(g), _u32(rt.deess_apply(d, x))), x.size
    # rows of one tile at the most hand nothing on: no summary
    short = [x for x in by_len if x.size <= R.TILE]
    rt.launch_counts(True)
    got = gm.deess_rows(short, a)
    assert _census(rt.launch_counts(False)) == {"k_de_carry_b": 1, "k_de_carry_p": 1, "k_de_carry_s": 1, "k_de_apply": 1}
    for x, g in zip(short, got):
        assert np.array_equal(_u32(g), _u32(rt.deess_apply(a, x))), x.size
    # in place
    x = np.array(by_len[-2], np.float32)
    pp = (C_FP * 1)(x.ctypes.data_as(C_FP))
    ns = (C.c_int64 * 1)(x.size)
    pd = (C.POINTER(rt.DeesserOpts) * 1)(C.pointer(a))
    assert rt.lib().ptts_deess_rows(gm.h, pd, pp, ns, 1, pp) == rt.PTTS_OK
    assert np.array_equal(_u32(x), _u32(rt.deess_apply(a, by_len[-2])))
    # a bad row is named
    with pytest.raises(pkg.PttsError) as ei:
        gm.deess_rows([by_len[3], by_len[3]], [a, rt.DeesserOpts(freq_hz=100.0)])
    assert ei.value.code == rt.PTTS_EINVAL and "freq_hz" in str(ei.value) and "row 1" in str(ei.value)


@pytest.fixture(scope="module")
def base(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    return gm.generate_batch(_toks(len(STEPS)), [TD._cfg(pkg, s) for s in STEPS])


def test_generated_requests_are_the_host_statement(pkg, tiny, base):  # noqa: F811
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4): the de-esser alone is ptts_deess_apply of the plain call's audio;
    with compressor, equaliser, fades and limiter around it the result is the host chain in the documented order."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    ds = [_for_audio(rt, b.pcm) for b in base]
    alone = [_bites(rt, d, b.pcm) for d, b in zip(ds, base)]
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, deesser=d) for s, d in zip(STEPS, ds)])
    for b, g, w in zip(base, got, alone):
        assert g.n_frames == b.n_frames and np.array_equal(_u32(g.pcm), _u32(w)), b.n_frames
    # a neighbour without one keeps its plain bits
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, deesser=d) if i % 2 else TD._cfg(pkg, s) for i, (s, d) in enumerate(zip(STEPS, ds))])
    for i, (b, m, w) in enumerate(zip(base, mixed, alone)):
        assert np.array_equal(_u32(m.pcm), _u32(w if i % 2 else b.pcm)), i
    # compressor -> de-esser -> equaliser -> fades -> limiter
    boost = rt.Eq(BOOST)
    cs = [TC._for_audio(rt, b.pcm) for b in base]
    squeezed = [TC._bites(rt, c, b.pcm) for c, b in zip(cs, base)]
    ds = [_for_audio(rt, x) for x in squeezed]
    pre = [TE._statement(pkg, _bites(rt, d, x), boost, **FADES) for d, x in zip(ds, squeezed)]
    ls = [TL._for_audio(rt, p) for p in pre]
    want = [TL._bites(rt, l, p) for l, p in zip(ls, pre)]
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, compressor=c, deesser=d, eq=boost, limiter=l, **FADES) for s, c, d, l in zip(STEPS, cs, ds, ls)])
    for b, g, w in zip(base, got, want):
        assert g.n_frames == b.n_frames and np.array_equal(_u32(g.pcm), _u32(w)), b.n_frames
    # the order matters: the de-esser in front of the compressor would give other bits
    other = rt.compress_apply(cs[0], rt.deess_apply(ds[0], base[0].pcm))
    assert not np.array_equal(_u32(other), _u32(rt.deess_apply(ds[0], squeezed[0])))
    boost.free()


def test_a_joined_call_runs_it_once_over_the_joined_audio(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    steps = [2, 5, 3, 4, 1, 6]                                   # two groups at max_batch = 4
    cfgs = [TD._cfg(pkg, s) for s in steps]
    plain = gm.generate_joined(_toks(len(steps)), cfgs, rt.JoinOpts())
    d = _for_audio(rt, plain.pcm)
    want = _bites(rt, d, plain.pcm)
    dsp = rt._dsp_opts(pkg.RuntimeGenerateConfig(deesser=d))
    rt.launch_counts(True)
    got = gm.generate_joined(_toks(len(steps)), cfgs, rt.JoinOpts(dsp=dsp))
    assert _census(rt.launch_counts(False)) == {k: 1 for k in DE_KERNELS}
    assert got.pcm.size == plain.pcm.size and np.array_equal(_u32(got.pcm), _u32(want))
    p = plain.parts[1]                                           # once over the whole, not part by part: the second part starts from the first's states
    mine = slice(p.offset, p.offset + p.n_samples)
    assert p.offset > 0 and not np.array_equal(_u32(rt.deess_apply(d, plain.pcm[mine])), _u32(want[mine]))


def test_requests_without_a_deesser_launch_what_they_launched(pkg, tiny, base):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    sw = dict(normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    c = TC._for_audio(rt, base[0].pcm)
    # the censuses of the chains as they were before the stage existed (tests/test_gpu_limiter.py and tests/test_gpu_compressor.py assert the same)
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, true_peak_dbtp=-20.0, **sw), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == dict(k_dsp_peak=1, k_dsp_apply=1, k_tp_peak=1, k_tp_scale=1)
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, compressor=c, true_peak_dbtp=-20.0, **sw), TD._cfg(pkg, 6)])
    with_cmp = dict({k: 1 for k in CMP_KERNELS}, k_dsp_peak=1, k_dsp_apply=1, k_tp_peak=1, k_tp_scale=1)
    assert _census(rt.launch_counts(False)) == with_cmp
    quiet = rt.DspExt(deesser=rt.DeesserOpts())                  # a live handle that switches nothing on: set, then cleared
    quiet.set_deesser(None)
    o = rt.DspOpts()
    o.ext = quiet.h
    rt.launch_counts(True)
    got = gm.generate_batch(toks[:2], [TD._cfg(pkg, s, dsp_opts=o) for s in STEPS[:2]])
    assert _census(rt.launch_counts(False)) == {}
    for g, b in zip(got, gm.generate_batch(toks[:2], [TD._cfg(pkg, s) for s in STEPS[:2]])):
        assert np.array_equal(_u32(g.pcm), _u32(b.pcm))
    quiet.free()
    # with one: its own seven kernels and nothing else new
    d = _for_audio(rt, base[0].pcm)
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, compressor=c, deesser=d, true_peak_dbtp=-20.0, **sw), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == dict(with_cmp, **{k: 1 for k in DE_KERNELS})
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, deesser=d), TD._cfg(pkg, 6)])     # alone: no row of the DSP table
    assert _census(rt.launch_counts(False)) == {k: 1 for k in DE_KERNELS}


def test_refused_where_samples_are_handed_over(pkg, tiny, rows):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    d = rt.DeesserOpts()
    cb = lambda off, x: None  # noqa: E731
    # a request with a pcm_callback: like every other switch of ext
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm
    rt.launch_counts(True)
    rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, deesser=d, pcm_callback=cb), TD._cfg(pkg, 4)])
    assert _census(rt.launch_counts(False)) == {}
    assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and "ext" in msg and "pcm_callback" in msg, (rc, msg)
    assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32))
    # a streamed joined call with a callback, and the windows hook: the message of its own, nothing launched
    dsp = rt._dsp_opts(pkg.RuntimeGenerateConfig(deesser=d))
    cfgs = [TD._cfg(pkg, 2), TD._cfg(pkg, 2)]
    rt.launch_counts(True)
    with pytest.raises(pkg.PttsError) as ei:
        gm.generate_joined(_toks(2), cfgs, rt.JoinOpts(dsp=dsp), pcm_callback=cb)
    assert not rt.launch_counts(False)
    assert ei.value.code == rt.PTTS_EINVAL and "join: stream" in str(ei.value) and NEW_MESSAGE in str(ei.value) and "pcm_callback" in str(ei.value), str(ei.value)
    by_len, _ = rows
    rt.launch_counts(True)
    with pytest.raises(pkg.PttsError) as ei:
        gm.dsp_windows([by_len[7]], [R.TILE], dsp)
    assert not rt.launch_counts(False)
    assert ei.value.code == rt.PTTS_EINVAL and NEW_MESSAGE in str(ei.value), str(ei.value)
    # the limiter's refusal keeps its wording and comes first
    both = rt._dsp_opts(pkg.RuntimeGenerateConfig(deesser=d, limiter=rt.LimiterOpts()))
    with pytest.raises(pkg.PttsError) as ei:
        gm.dsp_windows([by_len[7]], [R.TILE], both)
    assert "limiter looks ahead" in str(ei.value)
    # the model serves on: without a callback the joined call runs the stage, and the windows run what is causal
    assert gm.generate_joined(_toks(2), cfgs, rt.JoinOpts(dsp=dsp), first_group=1).n_frames == 4
    assert np.array_equal(_u32(gm.dsp_windows([by_len[7]], [R.TILE], rt.DspOpts(0, 1, 0.0, 0.0))[0]), _u32(gm.dsp_rows([by_len[7]], dc_block=True)[0]))
    assert np.array_equal(_u32(gm.deess_rows(by_len[7], d)), _u32(rt.deess_apply(d, by_len[7])))
