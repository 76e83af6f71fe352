"""The look-ahead peak limiter on the GPU (go-pocket-tts_amd/csrc/limiter.hip k_lim_*; limiter.h): ptts_limit_rows gives
the bits of ptts_limit_apply whatever rows share the launch; a request's limiter (ptts_dsp_ext_set_limiter on the handle of ptts_dsp_opts.ext)
is ptts_limit_apply of what the chain in front of it made of the request's own audio, bit for bit, and the true-peak ceiling and the egress
follow it; requests without a limiter launch what they launched."""
import ctypes as C
import math

import numpy as np
import pytest

import _compressor_ref as CR
import _eq_ref as E
import _limiter_ref as R
import test_gpu_compressor as TC   # a compressor for the model's own level
import test_gpu_dsp as TD          # the egress relations and their bounds (_check_dc, _convert), the dispatcher and raw-call helpers
import test_gpu_eq as TE           # the host statement of the chain in front of the limiter
from test_limiter_cpu import crest_rows
from test_gpu_loudness import tiny  # noqa: F401  (the tiny model with audible output)

pytestmark = pytest.mark.gpu

STEPS = [7, 3, 9, 6, 12, 5]
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)
TARGET = -1600
BOOST = [(E.PEAKING, 1000.0, 18.0, 0.7)]
C_FP = C.POINTER(C.c_float)
LIM_KERNELS = ("k_lim_summary", "k_lim_carry", "k_lim_gain", "k_lim_apply")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _opts(rt, name):
    return rt.LimiterOpts(*R.DESIGNS[name])


def _for_audio(rt, pcm, **kw):
    """A limiter whose ceiling lies 6 dB under the audio's own peak, inside the header's range: it engages whatever the model's level."""
    peak = float(np.abs(pcm).max())
    assert peak > 0
    kw.setdefault("lookahead_ms", 1.5)
    kw.setdefault("release_ms", 40.0)
    return rt.LimiterOpts(ceiling_db=min(max(20.0 * math.log10(peak) - 6.0, -60.0), 0.0), **kw)


def _bites(rt, l, pcm):
    """The limited audio, after the assertion that the stage moved it far above one f32 step at its peak."""
    y = rt.limit_apply(l, pcm)
    moved, bound = float(np.abs(y.astype(np.float64) - pcm).max()), E.bound(pcm)
    assert moved > 1000.0 * bound, (moved, bound)
    return y


def _census(counts, prefixes=("k_lim", "k_cmp", "k_tp", "k_eq", "k_dsp", "k_loud")):
    return {k: v for k, v in counts.items() if k.startswith(prefixes)}


@pytest.fixture(scope="module")
def rows():
    """design name -> the rows of every length; the placed crests, the burst and a NaN row"""
    whole = E.signal(124801, seed=31)
    by_len = {name: [whole[:n] for n in R.lengths(R.ahead(d))] for name, d in R.DESIGNS.items()}
    crests = [x for _, x, _ in crest_rows(R.DESIGNS["gentle"])]
    burst = CR.burst(9601)
    nan = E.signal(3841, seed=4)
    nan[1930] = np.nan
    for a in [whole, burst, nan] + crests:
        a.setflags(write=False)
    return by_len, crests, burst, nan


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_rows_are_the_host_bits(pkg, tiny, rows, name):  # noqa: F811
    """Every length alone, all beside each other, and in the other order; the placed crests, the burst and a NaN row; the four kernels in the
    census, each once."""
    _, gm = tiny
    rt = pkg.runtime
    by_len, crests, burst, nan = rows
    l = _opts(rt, name)
    table = by_len[name] + crests + [burst, nan]
    want = [rt.limit_apply(l, x) for x in table]
    assert int(np.isnan(want[-1]).sum()) == 1 and np.isnan(want[-1][1930])
    _bites(rt, l, by_len[name][-1])
    for x, w in zip(table, want):
        got = gm.limit_rows(x, l)
        assert got.shape == w.shape and np.array_equal(_u32(got), _u32(w)), (name, x.size)
    for order in (slice(None), slice(None, None, -1)):
        rt.launch_counts(True)
        got = gm.limit_rows(table[order], l)
        assert _census(rt.launch_counts(False), ("k_lim",)) == {k: 1 for k in LIM_KERNELS}
        for g, w in zip(got, want[order]):
            assert np.array_equal(_u32(g), _u32(w)), (name, w.size)
    # rows of one tile at the most hand nothing on: no summary
    short = [x for x in by_len[name] if x.size <= 1920]
    rt.launch_counts(True)
    gm.limit_rows(short, l)
    assert _census(rt.launch_counts(False), ("k_lim",)) == {"k_lim_carry": 1, "k_lim_gain": 1, "k_lim_apply": 1}
    # in place
    x = np.array(by_len[name][-2], np.float32)
    pp = (C_FP * 1)(x.ctypes.data_as(C_FP))
    ns = (C.c_int64 * 1)(x.size)
    pl = (C.POINTER(rt.LimiterOpts) * 1)(C.pointer(l))
    assert rt.lib().ptts_limit_rows(gm.h, pl, pp, ns, 1, pp) == rt.PTTS_OK
    assert np.array_equal(_u32(x), _u32(want[len(by_len[name]) - 2]))


def test_one_table_with_different_designs_and_a_null_row(pkg, tiny, rows):  # noqa: F811
    _, gm = tiny
    rt = pkg.runtime
    by_len, crests, burst, _ = rows
    mine = by_len["gentle"]
    a, b = _opts(rt, "fast"), _opts(rt, "driven")
    xs = [mine[8], burst, mine[7], mine[-1][:30000], mine[4], crests[4]]
    ls = [a, b, None, b, a, a]
    got = gm.limit_rows(xs, ls)
    for x, l, g in zip(xs, ls, got):
        want = x if l is None else rt.limit_apply(l, x)
        assert np.array_equal(_u32(g), _u32(want)), (x.size, l is None)
    assert not np.array_equal(_u32(rt.limit_apply(a, burst)), _u32(rt.limit_apply(b, burst)))
    with pytest.raises(pkg.PttsError) as ei:
        gm.limit_rows([mine[3], mine[3]], [a, rt.LimiterOpts(lookahead_ms=0.1)])
    assert ei.value.code == rt.PTTS_EINVAL and "lookahead_ms" in str(ei.value) and "row 1" in str(ei.value)


@pytest.fixture(scope="module")
def base(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    return gm.generate_batch(_toks(len(STEPS)), [TD._cfg(pkg, s) for s in STEPS])


def test_generated_requests_are_the_host_statement(pkg, tiny, base):  # noqa: F811
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4): the limiter alone; behind the compressor, loudness, a boosting
    equaliser and the fades; and in front of the true-peak ceiling.  Through k_resample as PCM16 at 16 kHz and mu-law at 8 kHz."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    # alone: ptts_limit_apply's bits, through the keyword and through a handle of the caller's; a neighbour without one keeps its plain bits
    ls = ls_alone = [_for_audio(rt, b.pcm, drive_db=3.0 if i % 2 else 0.0) for i, b in enumerate(base)]
    alone = [_bites(rt, l, b.pcm) for l, b in zip(ls, base)]
    for fmt, rate in (("f32", 0), ("s16", 16000), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, limiter=l) for s, l in zip(STEPS, ls)])
        for b, g, w in zip(base, got, alone):
            want = TD._convert(pkg, gm, w, fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
    exts = [rt.DspExt(limiter=l) for l in ls]

    def handle(i):
        o = rt.DspOpts()
        o.ext = exts[i].h
        return o
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, dsp_opts=handle(i)) if i % 2 else TD._cfg(pkg, s) for i, s in enumerate(STEPS)])
    for i, (b, m, w) in enumerate(zip(base, mixed, alone)):
        assert np.array_equal(_u32(m.pcm), _u32(w if i % 2 else b.pcm)), i
    for e in exts:
        e.free()
    # behind the compressor, loudness, a boosting equaliser and the fades: the host chain, then ptts_limit_apply
    boost = rt.Eq(BOOST)
    cs = [TC._for_audio(rt, b.pcm) for b in base]
    pre = [TE._statement(pkg, rt.compress_apply(c, b.pcm), boost, loudness=TARGET, **FADES) for c, b in zip(cs, base)]
    ls = [_for_audio(rt, p) for p in pre]
    want24 = [_bites(rt, l, p) for l, p in zip(ls, pre)]
    sw = [dict(loudness=TARGET, eq=boost, compressor=c, limiter=l, **FADES) for c, l in zip(cs, ls)]
    for fmt, rate in (("f32", 0), ("s16", 16000), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, **k) for s, k in zip(STEPS, sw)])
        for b, g, w in zip(base, got, want24):
            want = TD._convert(pkg, gm, w, fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
    # ... and in front of the true-peak ceiling, which sits 3 dB under what the limiter left
    ceil = [min(max(20.0 * math.log10(float(rt.true_peak(w))) - 3.0, -60.0), 0.0) for w in want24]
    tp24 = [rt.true_peak_limit(w, c)[0] for w, c in zip(want24, ceil)]
    assert all(not np.array_equal(_u32(t), _u32(w)) for t, w in zip(tp24, want24))
    for fmt, rate in (("f32", 0), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, true_peak_dbtp=t, **k) for s, k, t in zip(STEPS, sw, ceil)])
        for b, g, w in zip(base, got, tp24):
            want = TD._convert(pkg, gm, w, fmt, rate)
            assert g.n_frames == b.n_frames and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
    # the ceiling with the limiter alone in front of it (no other switch in the DSP table)
    ceil_alone = [min(max(20.0 * math.log10(float(rt.true_peak(w))) - 3.0, -60.0), 0.0) for w in alone]
    tp_alone = [rt.true_peak_limit(w, c)[0] for w, c in zip(alone, ceil_alone)]
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, limiter=l, true_peak_dbtp=t) for s, l, t in zip(STEPS, ls_alone, ceil_alone)])
    for g, w, a in zip(got, tp_alone, alone):
        assert np.array_equal(_u32(g.pcm), _u32(w)) and not np.array_equal(_u32(w), _u32(a))
    # ... and with the DC block: within the DC block's bounds (TD._check_dc's relations)
    pre = [TE._statement(pkg, rt.compress_apply(c, b.pcm), boost, loudness=TARGET, dc_block=True, **FADES) for c, b in zip(cs, base)]
    host = [rt.limit_apply(l, p) for l, p in zip(ls, pre)]
    for fmt, rate in (("f32", 0), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, dc_block=True, **k) for s, k in zip(STEPS, sw)])
        for b, g, h in zip(base, got, host):
            TD._check_dc(pkg, gm, g.pcm, h, fmt, rate, f"generate compressor+loudness+dc+eq+fades+limiter {fmt} {rate or 24000} Hz frames={b.n_frames}")
    boost.free()


def test_continuous_dispatcher_gives_the_one_shot_bits(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    steps = [7, 6, 9, 5]
    toks = _toks(len(steps))
    for continuous in (False, True):
        own = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s) for s in steps], continuous)
        ls = [_for_audio(rt, o.pcm) for o in own]
        specs = [(7, "f32", 0, dict(limiter=ls[0])), (6, "ulaw", 8000, dict(limiter=ls[1], fade_out_ms=80.0)), (9, "f32", 0, None),
                 (5, "s16", 16000, dict(limiter=ls[3], fade_in_ms=50.0))]
        got = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs], continuous)
        shot = gm.generate_batch(toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs])
        host = [_bites(rt, ls[0], own[0].pcm), _bites(rt, ls[1], rt.dsp_apply(own[1].pcm, fade_out_ms=80.0)), own[2].pcm,
                _bites(rt, ls[3], rt.dsp_apply(own[3].pcm, fade_in_ms=50.0))]
        for i, (s, f, r, sw) in enumerate(specs):
            assert got[i].n_frames == s
            assert np.array_equal(TD._bits(got[i].pcm), TD._bits(shot[i].pcm)), (continuous, i, f, r)
            assert np.array_equal(TD._bits(got[i].pcm), TD._bits(TD._convert(pkg, gm, host[i], f, r))), (continuous, i, f, r)


def test_requests_without_a_limiter_launch_what_they_launched(pkg, tiny, base):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    sw = dict(normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    rt.launch_counts(True)
    got = gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, true_peak_dbtp=-20.0, **sw), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == dict(k_dsp_peak=1, k_dsp_apply=1, k_tp_peak=1, k_tp_scale=1)
    quiet = rt.DspExt(limiter=rt.LimiterOpts())                           # a live handle that switches nothing on: set, then cleared
    quiet.set_limiter(None)
    o = rt.DspOpts()
    o.ext = quiet.h
    rt.launch_counts(True)
    got = gm.generate_batch(toks[:2], [TD._cfg(pkg, s, dsp_opts=o) for s in STEPS[:2]])
    assert _census(rt.launch_counts(False)) == {}
    for g, b in zip(got, gm.generate_batch(toks[:2], [TD._cfg(pkg, s) for s in STEPS[:2]])):   # (a batch of two: the decoder's bits are the batch shape's)
        assert np.array_equal(_u32(g.pcm), _u32(b.pcm))
    quiet.free()
    # with one: its kernels once for the decoded group, behind the table's other kernels and in front of the ceiling's pair
    l = _for_audio(rt, base[0].pcm)
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, limiter=l, true_peak_dbtp=-20.0, **sw), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == dict({k: 1 for k in LIM_KERNELS}, k_dsp_peak=1, k_dsp_apply=1, k_tp_peak=1, k_tp_scale=1)


def test_refused_with_pcm_callback(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm
    cb = lambda off, x: None  # noqa: E731
    rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, limiter=rt.LimiterOpts(), pcm_callback=cb), TD._cfg(pkg, 4)])
    assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and "ext" in msg and "pcm_callback" in msg, (rc, msg)
    assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32))
