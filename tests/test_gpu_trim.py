"""Silence control on the GPU (go-pocket-tts_amd/csrc/trim.hip, generate.cpp generate_joined; include/ptts.h ptts_trim_opts; DESIGN.md section
8, N3): ptts_trim_rows gives ptts_trim_apply's samples and records bit for bit on the crafted rows; a joined call with a trim is the host join
of the host trim of the same requests' audio from one generate_batch call, within a group and across groups; the chain reads the trimmed,
joined audio; one launch of each kernel per group and none without a trim; refusals launch nothing; one request is the trimmed utterance.

The tiny checkpoint's audio peaks near 3.0 -- a fifth of its samples lie above the highest threshold a trim may name (0 dB), and the level comes from
make_checkpoint's initialisation scale, which another seed does not change: its last convolution is scaled by 2^-6 here, so that thresholds taken from the audio's own quantiles -- and one above its peak -- lie inside -120 .. 0 dB."""
import ctypes as C
import math

import numpy as np
import pytest

import _trim_ref as R

pytestmark = pytest.mark.gpu

SPF = 1920
STEPS3, STEPS6 = [2, 5, 3], [2, 5, 3, 4, 1, 6]   # six: two groups at max_batch = 4
MODES = [dict(), dict(gap_ms=37.5), dict(crossfade_ms=10.0)]


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    tensors = synth.make_checkpoint(cfg, seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("trim") / "tiny_quiet.safetensors")
    synth.write_safetensors(path, tensors)
    gm = pkg.Model.open(path, device=0, max_batch=4)
    yield cfg, gm
    gm.close()


def _cfg(pkg, steps, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, **kw)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _with_trim(rt, trim, normalize=0, fade_in_ms=0.0, fade_out_ms=0.0):
    """a DspOpts whose ext carries the trim (the handle lives as long as the struct)"""
    d = rt.DspOpts(normalize, 0, fade_in_ms, fade_out_ms)
    d._ext = rt.DspExt(trim=trim)
    d.ext = d._ext.h
    return d


@pytest.fixture(scope="module")
def chunks(pkg, tiny):
    """steps -> the requests' own 24 kHz audio from ONE generate_batch call (which groups as the joined call does): computed once, never written to."""
    _, gm = tiny
    out = {}
    for steps in (STEPS3, STEPS6):
        res = gm.generate_batch(_toks(len(steps)), [_cfg(pkg, s) for s in steps])
        pcm = [np.array(r.pcm, np.float32) for r in res]
        for p, s in zip(pcm, steps):
            assert p.size == s * SPF
            p.setflags(write=False)
        out[tuple(steps)] = pcm
    return out


def _thresholds(pcm):
    """dB values at the 50th, 99th and 99.9th percentile of the chunks' |x|, and one above their peak"""
    a = np.abs(np.concatenate(pcm)).astype(np.float64)
    peak = float(a.max())
    levels = [float(np.quantile(a, q)) for q in (0.5, 0.99, 0.999)] + [peak * 1.25]
    assert 0.0 < levels[0] and levels[-1] < 1.0, levels                  # inside -120 .. 0 dB
    return [20.0 * math.log10(v) for v in levels]


def test_rows_are_the_host_trim_bit_for_bit(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    cases = R.cases()
    designs = {tuple(sorted(kw.items())) for _, _, kw in cases}
    assert len(designs) > 16                                              # more distinct designs than one table holds, in one call
    opts = [rt.TrimOpts(**kw) for _, _, kw in cases]
    rows = [x for _, x, _ in cases]
    got, recs = gm.trim_rows(rows, opts)
    for (name, x, kw), o, g, rec in zip(cases, opts, got, recs):
        want, info = rt.trim_apply(o, x)
        assert rec.astuple() == info.astuple() == R.plan(x, **kw)[1], (name, rec.astuple(), info.astuple())
        assert g.size == want.size and np.array_equal(_u32(g), _u32(want)), (name, int((_u32(g) != _u32(want)).sum()))
    # 300 rows of 1 .. 7 samples: the 256-row table boundary; every third row without a trim is a copy
    rows, kws = R.many_rows()
    opts = [None if kw is None else rt.TrimOpts(**kw) for kw in kws]
    got, recs = gm.trim_rows(rows, opts)
    for i, (x, o, g, rec) in enumerate(zip(rows, opts, got, recs)):
        if o is None:
            assert rec.astuple() == (0, x.size, x.size, 0, 0) and np.array_equal(_u32(g), _u32(x)), i
            continue
        want, info = rt.trim_apply(o, x)
        assert rec.astuple() == info.astuple() and np.array_equal(_u32(g), _u32(want)), (i, rec.astuple(), info.astuple())
    # one array alone; in[i] == out[i]
    x = R.row(2 * R.T + 9, [700, R.T + 900])
    o = rt.TrimOpts(edges=1, threshold_db=R.THR_DB, pad_ms=2.0, max_pause_ms=20.0)
    g, rec = gm.trim_rows(x, o)
    want, info = rt.trim_apply(o, x)
    assert rec.astuple() == info.astuple() and info.cuts == 1 and np.array_equal(_u32(g), _u32(want))
    y = x.copy()
    infos = (rt.TrimInfo * 1)()
    pp, po = rt._row_ptrs([y]), (C.POINTER(rt.TrimOpts) * 1)(C.pointer(o))
    assert rt.lib().ptts_trim_rows(gm.h, po, pp, rt._ip(np.array([y.size], np.int64)), 1, pp, infos) == rt.PTTS_OK
    assert infos[0].n_out == want.size and np.array_equal(_u32(y[:want.size]), _u32(want))
    # a bad row is named
    with pytest.raises(pkg.PttsError) as ei:
        gm.trim_rows([x, x], [o, rt.TrimOpts(pad_ms=-1.0)])
    assert ei.value.code == rt.PTTS_EINVAL and "row 1" in str(ei.value) and "pad_ms" in str(ei.value)


def test_joined_with_trim_is_the_host_join_of_the_host_trim(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    seen = dict(lo=0, hi=0, cuts=0, whole=0)
    for steps in (STEPS3, STEPS6):
        pcm = chunks[tuple(steps)]
        for db in _thresholds(pcm):
            trim = rt.TrimOpts(edges=1, threshold_db=db, pad_ms=5.0, max_pause_ms=20.0)
            parts, infos = zip(*[rt.trim_apply(trim, p) for p in pcm])
            for p, i in zip(pcm, infos):
                seen["lo"] += i.lo > 0
                seen["hi"] += i.speech == 1 and i.hi < p.size
                seen["cuts"] += i.cuts >= 1
                seen["whole"] += i.speech == 0 and i.n_out == p.size
            for mode in MODES:
                got = gm.generate_joined(_toks(len(steps)), [_cfg(pkg, s) for s in steps], rt.JoinOpts(dsp=_with_trim(rt, trim), **mode))
                o = rt.JoinOpts(**mode)
                want = rt.join(parts, o)
                total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
                assert got.pcm.size == want.size == total and np.array_equal(_u32(got.pcm), _u32(want)), (steps, db, mode, got.pcm.size, want.size)
                assert [p.offset for p in got.parts] == [int(v) for v in offs] and [p.n_samples for p in got.parts] == [p.size for p in parts], (steps, db, mode)
                assert [p.n_frames for p in got.parts] == steps and got.n_frames == sum(steps)          # frames still count what was decoded
    print("parts with lo > 0 / hi < n / cuts >= 1 / no speech, kept whole:", seen)
    assert all(v >= 1 for v in seen.values()), seen                       # inputs that do not exercise the feature fail


def test_trim_and_the_chain(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    pcm = chunks[tuple(STEPS6)]
    db = _thresholds(pcm)[2]
    trim = rt.TrimOpts(edges=1, threshold_db=db, pad_ms=5.0, max_pause_ms=20.0)
    parts = [rt.trim_apply(trim, p)[0] for p in pcm]
    assert sum(p.size for p in parts) < sum(p.size for p in pcm)
    o = rt.JoinOpts(gap_ms=37.5)
    want = rt.dsp_apply(rt.join(parts, o), normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    got = gm.generate_joined(_toks(6), [_cfg(pkg, s) for s in STEPS6], rt.JoinOpts(gap_ms=37.5, dsp=_with_trim(rt, trim, 1, 50.0, 80.0)))
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want))
    assert abs(float(np.abs(got.pcm).max()) - 1.0) < 1e-6 and got.pcm[0] == 0.0 and got.pcm[-1] == 0.0


def test_launch_counts(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    kernels = ("k_trim_mark", "k_trim_carry", "k_trim_store")
    trim = rt.TrimOpts(edges=1, threshold_db=_thresholds(chunks[tuple(STEPS6)])[1], pad_ms=5.0, max_pause_ms=20.0)
    for steps, groups in ((STEPS3, 1), (STEPS6, 2)):
        cfgs = [_cfg(pkg, s) for s in steps]
        rt.launch_counts(True)
        gm.generate_joined(_toks(len(steps)), cfgs, rt.JoinOpts(dsp=_with_trim(rt, trim)))
        counts = rt.launch_counts(False)
        assert [counts.get(k) for k in kernels] == [groups] * 3 and counts.get("k_join") == groups, counts
        rt.launch_counts(True)
        got = gm.generate_joined(_toks(len(steps)), cfgs)
        counts = rt.launch_counts(False)
        assert not [k for k in counts if k.startswith("k_trim")] and counts.get("k_join") == groups, counts
        assert np.array_equal(_u32(got.pcm), _u32(np.concatenate(chunks[tuple(steps)])))   # as today


def test_refusals_launch_nothing(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    d = _with_trim(rt, rt.TrimOpts())
    x = R.row(4000, [100, 3000])

    def refused(call):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            call()
        counts = rt.launch_counts(False)
        msg = str(ei.value)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (msg, counts)
        assert "dsp: ext: trim" in msg and "ptts_generate_joined" in msg and "ptts_trim_rows" in msg, msg

    refused(lambda: gm.generate_batch(_toks(1), [_cfg(pkg, 2, dsp_opts=d)]))
    refused(lambda: gm.dsp_rows(x, opts=d))
    refused(lambda: gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2, dsp_opts=d)]))
    # an ext without a trim behaves as before, and the model serves on
    d._ext.set_trim(None)
    assert np.array_equal(_u32(gm.dsp_rows(x, opts=d)), _u32(x))
    assert gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2)]).n_frames == 4


def test_one_request_is_the_trimmed_utterance(pkg, tiny):
    """The single-utterance form: no lead-in silence in front of the first loud sample but the pad."""
    _, gm = tiny
    rt = pkg.runtime
    whole = np.array(gm.generate_batch(_toks(1), [_cfg(pkg, STEPS3[0])])[0].pcm, np.float32)
    trim = rt.TrimOpts(edges=1, threshold_db=_thresholds([whole])[2], pad_ms=1.0, max_pause_ms=0.0)
    want, info = rt.trim_apply(trim, whole)
    assert info.speech == 1 and info.lo > 0 and info.n_out == info.hi - info.lo < whole.size
    got = gm.generate_joined(_toks(1), [_cfg(pkg, STEPS3[0])], rt.JoinOpts(dsp=_with_trim(rt, trim)))
    assert np.array_equal(_u32(got.pcm), _u32(want)) and got.n_frames == STEPS3[0]
    assert got.parts[0].offset == 0 and got.parts[0].n_samples == info.n_out


def test_every_record_of_trim_rows_is_trim_plans(pkg, tiny):
    """Every TrimInfo field ptts_trim_rows reports is ptts_trim_plan's for the same row: rows the trim shortens at the edges and at a pause, a row
    it leaves whole (all loud; quiet throughout, which counts as no speech), the row whose n_out is 0 (the trim keeps a sample wherever there is
    speech, so it is the row of no samples) and rows without a trim, whose record is the preset one."""
    _, gm = tiny
    rt = pkg.runtime
    o = rt.TrimOpts(edges=1, threshold_db=R.THR_DB, pad_ms=2.0, max_pause_ms=20.0)
    loud = np.full(1921, 0.5, np.float32)
    rows = [R.row(2 * R.T + 9, [700, R.T + 900]), R.quiet(1919), loud, R.row(481, [0, 480]), np.zeros(0, np.float32), R.quiet(1920), R.row(1921, [1920]), loud]
    opts = [o, o, o, o, o, None, o, None]
    got, recs = gm.trim_rows(rows, opts)
    seen = set()
    for i, (x, t, g, rec) in enumerate(zip(rows, opts, got, recs)):
        if t is None:
            assert (rec.lo, rec.hi, rec.n_out, rec.cuts, rec.speech, rec.reserved) == (0, x.size, x.size, 0, 0, 0) and np.array_equal(_u32(g), _u32(x)), i
            continue
        want = rt.trim_plan(t, x)
        assert (rec.lo, rec.hi, rec.n_out, rec.cuts, rec.speech, rec.reserved) == (want.lo, want.hi, want.n_out, want.cuts, want.speech, 0), (i, rec.astuple(), want.astuple())
        assert g.size == want.n_out == R.plan(x, edges=1, threshold_db=R.THR_DB, pad_ms=2.0, max_pause_ms=20.0)[1][2], i
        seen.add("empty" if want.n_out == 0 else "whole" if want.n_out == x.size else "cut" if want.cuts else "edges")
    assert seen == {"empty", "whole", "cut", "edges"} and recs[4].n_out == 0 and (recs[1].n_out, recs[1].speech) == (1919, 0), seen


def test_refusal_texts_of_trim_rows(pkg, tiny):
    """Every refusal site of ptts_trim_rows, byte for byte.  A length of 2^31 is refused before any row is read: the row behind it holds one sample."""
    _, gm = tiny
    rt = pkg.runtime
    x = R.row(2000, [700])
    o = rt.TrimOpts(edges=1, threshold_db=R.THR_DB)

    def trim(t, rows, n=None, null=None):
        pp = rt._row_ptrs(rows)
        po = (C.POINTER(rt.TrimOpts) * len(t))(*[None if v is None else C.pointer(v) for v in t])
        outs = rt._row_ptrs([np.empty(max(r.size, 1), np.float32) for r in rows])
        ns = np.array([r.size for r in rows] if n is None else n, np.int64)
        args = dict(t=po, rows=pp, n=rt._ip(ns), out=outs, info=(rt.TrimInfo * len(rows))())
        if null:
            args[null] = None
        rt._check(rt.lib().ptts_trim_rows(gm.h, args["t"], args["rows"], args["n"], len(rows), args["out"], args["info"]))

    def refusal(call):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            call()
        assert ei.value.code == rt.PTTS_EINVAL and not rt.launch_counts(False)
        return str(ei.value)

    for null in ("t", "rows", "n", "out", "info"):
        assert refusal(lambda: trim([o], [x], null=null)) == "ptts-hip: trim: null argument"
    assert refusal(lambda: trim([o, o], [x, x], n=[x.size, -1])) == "ptts-hip: trim: row 1 is negative or null"
    assert refusal(lambda: trim([o, rt.TrimOpts(pad_ms=-1.0)], [x, x])) == "ptts-hip: row 1: trim: pad_ms -1 is not a finite value from 0 to 500"
    assert refusal(lambda: trim([o, rt.TrimOpts(edges=0)], [x, x])) == "ptts-hip: row 1: trim: nothing switched on (edges is 0 and max_pause_ms is 0)"
    one = np.zeros(1, np.float32)
    for t in (o, None):                                                    # (a row without a trim is held to the length as well)
        assert refusal(lambda: trim([None, t], [one, one], n=[1, 1 << 31])) == f"ptts-hip: trim: row 1 has {1 << 31} samples, a row must stay below 2^31"
    got, rec = gm.trim_rows(x, o)                                          # the model serves on
    assert rec.astuple() == rt.trim_plan(o, x).astuple() and got.size == rec.n_out
