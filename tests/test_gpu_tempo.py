"""The speaking rate on the GPU (go-pocket-tts_amd/csrc/tempo.hip, generate.cpp generate_joined; include/ptts.h ptts_tempo_opts; DESIGN.md
section 8, N3): ptts_tempo_rows gives ptts_tempo_apply's bits on the crafted rows, speeds mixed in one call, across the 256-row table boundary;
a joined call with a tempo is the host chain trim -> tempo -> join -> chain -> egress of the same requests' audio from one generate_batch call,
bit for bit, within a group and across groups; one launch of each kernel per group and none without a tempo; refusals launch nothing.

The tiny checkpoint's audio peaks near 3.0, above the search's clamp and above the highest threshold a trim may name: its last convolution is
scaled by 2^-6 here, as test_gpu_trim.py does."""
import math
import re

import numpy as np
import pytest

import _tempo_ref as R

pytestmark = pytest.mark.gpu

SPF = 1920
STEPS = [2, 4, 3]            # three parts, two groups at max_batch = 2
KERNELS = ("k_tempo_plan", "k_tempo_store")


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    tensors = synth.make_checkpoint(cfg, seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("tempo") / "tiny_quiet.safetensors")
    synth.write_safetensors(path, tensors)
    gm = pkg.Model.open(path, device=0, max_batch=2)
    yield cfg, gm
    gm.close()


def _cfg(pkg, steps, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, **kw)


def _toks(n):
    return [[3 + i % 40, 7, 11 + i % 40] for i in range(n)]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _with(rt, trim=None, tempo=None, normalize=0, fade_in_ms=0.0, fade_out_ms=0.0):
    """a DspOpts whose ext carries the trim and the tempo (the handle lives as long as the struct)"""
    d = rt.DspOpts(normalize, 0, fade_in_ms, fade_out_ms)
    d._ext = rt.DspExt(trim=trim, tempo=tempo)
    d.ext = d._ext.h
    return d


@pytest.fixture(scope="module")
def chunks(pkg, tiny):
    """the requests' own 24 kHz audio from ONE generate_batch call (which groups as the joined call does): computed once, never written to"""
    _, gm = tiny
    res = gm.generate_batch(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS])
    pcm = [np.array(r.pcm, np.float32) for r in res]
    for p, s in zip(pcm, STEPS):
        assert p.size == s * SPF
        p.setflags(write=False)
    return pcm


def _joined(pkg, gm, join=None):
    return gm.generate_joined(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS], join)


def test_rows_are_the_host_tempo_bit_for_bit(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    cases = R.cases()
    assert len({s for _, _, s in cases}) == len(R.SPEEDS)                 # per-row speeds mixed in one call (and fewer designs than a table holds)
    rows = [x for _, x, _ in cases]
    opts = [rt.TempoOpts(s) for _, _, s in cases]
    got = gm.tempo_rows(rows, opts)
    for (name, x, s), o, g in zip(cases, opts, got):
        want = rt.tempo_apply(o, x)
        assert g.size == want.size == R.length(x.size, s), (name, g.size, want.size)
        assert np.array_equal(_u32(g), _u32(want)), (name, int((_u32(g) != _u32(want)).sum()))
    # 260 rows of 481 samples with a tempo, so that the second launch group runs, and 65 without one among them, which are copies
    rows, speeds = R.many_rows()
    assert sum(s is not None for s in speeds) == 260
    opts = [None if s is None else rt.TempoOpts(s) for s in speeds]
    rt.launch_counts(True)
    got = gm.tempo_rows(rows, opts)
    counts = rt.launch_counts(False)
    assert [counts.get(k) for k in KERNELS] == [2, 2], counts
    for i, (x, o, g) in enumerate(zip(rows, opts, got)):
        want = x if o is None else rt.tempo_apply(o, x)
        assert g.size == want.size and np.array_equal(_u32(g), _u32(want)), (i, speeds[i])
    # one array alone; copies alone launch nothing; a bad row is named
    x = R.tone(5000, 137.0)
    o = rt.TempoOpts(800)
    assert np.array_equal(_u32(gm.tempo_rows(x, o)), _u32(rt.tempo_apply(o, x)))
    rt.launch_counts(True)
    assert np.array_equal(_u32(gm.tempo_rows(x, None)), _u32(x))
    assert not rt.launch_counts(False)
    with pytest.raises(pkg.PttsError) as ei:
        gm.tempo_rows([x, x], [o, rt.TempoOpts(2001)])
    assert ei.value.code == rt.PTTS_EINVAL and "row 1" in str(ei.value) and "speed_permille" in str(ei.value)


def _trim_db(pcm):
    """the 99th percentile of the chunks' |x| in dB: a threshold that cuts edges and pauses"""
    v = float(np.quantile(np.abs(np.concatenate(pcm)).astype(np.float64), 0.99))
    assert 0.0 < v < 1.0
    return 20.0 * math.log10(v)


def _check_parts(rt, got, parts, o):
    total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
    assert got.pcm.size == total
    assert [p.offset for p in got.parts] == [int(v) for v in offs] and [p.n_samples for p in got.parts] == [p.size for p in parts]
    assert [p.n_frames for p in got.parts] == STEPS and got.n_frames == sum(STEPS)          # frames still count what was decoded


@pytest.mark.parametrize("speed", [800, 1250])
def test_joined_with_tempo_is_the_host_join_of_the_host_tempo(pkg, tiny, chunks, speed):
    _, gm = tiny
    rt = pkg.runtime
    tempo = rt.TempoOpts(speed)
    parts = [rt.tempo_apply(tempo, p) for p in chunks]
    assert [p.size for p in parts] == [s * SPF * 1000 // speed for s in STEPS]
    spliced = sum(int((np.diff(rt.tempo_plan(tempo, p).astype(np.int64)) != R.HS).sum()) for p in chunks)
    assert spliced >= len(STEPS), spliced                                  # inputs that do not exercise the feature fail
    got = _joined(pkg, gm, rt.JoinOpts(dsp=_with(rt, tempo=tempo)))
    want = np.concatenate(parts)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    _check_parts(rt, got, parts, rt.JoinOpts())


def test_trim_tempo_and_gap(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(chunks), pad_ms=5.0, max_pause_ms=20.0)
    tempo = rt.TempoOpts(800)
    trimmed = [rt.trim_apply(trim, p)[0] for p in chunks]
    assert all(0 < t.size < p.size for t, p in zip(trimmed, chunks))       # the tempo reads what the trim left, not the decoder's rows
    parts = [rt.tempo_apply(tempo, t) for t in trimmed]
    want = rt.join(parts, rt.JoinOpts(gap_ms=37.5))
    got = _joined(pkg, gm, rt.JoinOpts(gap_ms=37.5, dsp=_with(rt, trim=trim, tempo=tempo)))
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    _check_parts(rt, got, parts, rt.JoinOpts(gap_ms=37.5))


def test_tempo_crossfade_chain_and_egress(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    tempo = rt.TempoOpts(1250)
    parts = [rt.tempo_apply(tempo, p) for p in chunks]
    o = rt.JoinOpts(crossfade_ms=10.0)
    joined = rt.dsp_apply(rt.join(parts, o), normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    want = gm.pcm_encode(gm.resample(joined, 24000, 8000), pkg.PCM_ULAW)
    got = _joined(pkg, gm, rt.JoinOpts(crossfade_ms=10.0, sample_rate=8000, pcm_format=pkg.PCM_ULAW, dsp=_with(rt, tempo=tempo, normalize=1, fade_in_ms=50.0, fade_out_ms=80.0)))
    assert got.pcm.dtype == want.dtype and got.pcm.size == want.size == rt.resample_length(joined.size, 24000, 8000)
    assert np.array_equal(_bits(got.pcm), _bits(want)), int((_bits(got.pcm) != _bits(want)).sum())
    total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
    assert joined.size == total and [p.offset for p in got.parts] == [int(v) for v in offs]      # parts count 24 kHz samples, whatever the egress
    assert [p.n_samples for p in got.parts] == [p.size for p in parts] and got.n_frames == sum(STEPS)


def test_launch_counts(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    rt.launch_counts(True)
    _joined(pkg, gm, rt.JoinOpts(dsp=_with(rt, tempo=rt.TempoOpts(1250))))
    counts = rt.launch_counts(False)
    assert [counts.get(k) for k in KERNELS] == [2, 2] and counts.get("k_join") == 2 and not [k for k in counts if k.startswith("k_trim")], counts
    rt.launch_counts(True)
    plain = _joined(pkg, gm)
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith("k_tempo")] and counts.get("k_join") == 2, counts
    assert np.array_equal(_u32(plain.pcm), _u32(np.concatenate(chunks)))   # as today
    d = _with(rt, tempo=rt.TempoOpts(800))
    d._ext.set_tempo(None)                                                 # set and cleared: the handle switches nothing on
    rt.launch_counts(True)
    cleared = _joined(pkg, gm, rt.JoinOpts(dsp=d))
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith("k_tempo")], counts
    assert np.array_equal(_u32(cleared.pcm), _u32(plain.pcm)) and [p.n_samples for p in cleared.parts] == [p.n_samples for p in plain.parts]


def test_refusals_launch_nothing(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    d = _with(rt, tempo=rt.TempoOpts(1250))
    x = R.tone(4000, 200.0)

    def refused(call, *words):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            call()
        counts = rt.launch_counts(False)
        msg = str(ei.value)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (msg, counts)
        assert all(w in msg for w in words), msg
        return msg

    words = ("dsp: ext: tempo", "ptts_generate_joined", "ptts_tempo_rows")
    refused(lambda: gm.generate_batch(_toks(1), [_cfg(pkg, 2, dsp_opts=d)]), *words)
    refused(lambda: gm.dsp_rows(x, opts=d), *words)
    refused(lambda: gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2, dsp_opts=d)]), *words)
    # a text whose step budgets stay below 2^31 samples as they are and pass it slowed to half speed: a part's budget is the decoder's
    # reach (8192 positions of the upsampled sequence), whatever larger step count the request names
    big = 1 << 20
    per_part = 8192 // gm.info.steps_per_latent * gm.info.samples_per_frame
    n = (3 << 29) // per_part                                             # n parts allow about 1.5 * 2^30 samples
    assert 1 <= n <= 4096 and (1 << 30) <= n * per_part < (1 << 31)
    slow = _with(rt, tempo=rt.TempoOpts(500))
    msg = refused(lambda: gm.generate_joined(_toks(n), [_cfg(pkg, big)] * n, rt.JoinOpts(dsp=slow)), "2^31")
    assert int(re.search(r"allow (\d+) samples", msg).group(1)) == 2 * n * per_part
    # an ext without a tempo behaves as before, and the model serves on
    d._ext.set_tempo(None)
    assert np.array_equal(_u32(gm.dsp_rows(x, opts=d)), _u32(x))
    assert gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2)]).n_frames == 4
