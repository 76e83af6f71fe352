"""The pitch on the GPU (go-pocket-tts_amd/csrc/pitch.hip, generate.cpp generate_joined; include/ptts.h ptts_pitch_opts):
ptts_pitch_rows gives ptts_pitch_apply's bits (outside NaN outputs) on rows around every length at which the kernel takes another path, pitches
mixed in one call, with and without a tempo, across the 256-row table boundary; a joined call with a pitch is the host chain trim -> pitch ->
tempo -> join -> chain -> egress of the same requests' audio from one generate_batch call, bit for bit, within a group and across groups, streamed
too; one k_pitch_resample launch per group, none without a pitch or at 1000; refusals launch nothing.

The tiny checkpoint's audio peaks near 3.0, above the tempo search's clamp and above the highest threshold a trim may name: its last
convolution is scaled by 2^-6 here, as test_gpu_tempo.py does."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import _pitch_ref as R

pytestmark = pytest.mark.gpu

SPF = 1920
STEPS = [2, 4, 3]            # three parts, two groups at max_batch = 2
TILE = 1024                  # kernels.h kPitchTile: the outputs of one workgroup
PITCHES = (500, 501, 707, 999, 1001, 1250, 1999, 2000)
TEMPO_KERNELS = ("k_tempo_plan", "k_tempo_store")


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    tensors = synth.make_checkpoint(cfg, seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("pitch") / "tiny_quiet.safetensors")
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


def _same(got, want):
    """bit for bit outside NaN outputs, and NaN where the host has one"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.size == want.size and np.array_equal(np.isnan(got), nan) and np.array_equal(_u32(got)[~nan], _u32(want)[~nan])


def _with(rt, trim=None, tempo=None, pitch=None, normalize=0, fade_in_ms=0.0, fade_out_ms=0.0):
    """a DspOpts whose ext carries the trim, the tempo and the pitch (the handle lives as long as the struct)"""
    d = rt.DspOpts(normalize, 0, fade_in_ms, fade_out_ms)
    d._ext = rt.DspExt(trim=trim, tempo=tempo, pitch=pitch)
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


def _joined(pkg, gm, join=None, **kw):
    return gm.generate_joined(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS], join, **kw)


def _input_lengths(p):
    """the row lengths whose resampled forms lie around one tile: the longest with at most TILE - 1 outputs, the shortest with at least TILE and
    the shortest with at least TILE + 1 (below 1000 not every output length exists: at 500 they are all even, so two of the three may be one row)"""
    n = TILE * p // 1000 - 2
    while R.resample_length(n + 1, p) <= TILE - 1:
        n += 1
    out = [n]
    for least in (TILE, TILE + 1):
        while R.resample_length(n, p) < least:
            n += 1
        out.append(n)
    return sorted(set(out))


def _crafted():
    """[(row, p)]: per pitch the short lengths (nothing, one tap's worth, rows shorter than a support at 1000 and at 2000) and the rows whose
    OUTPUT is one tile less one, one tile and one tile and one"""
    out = []
    for p in PITCHES:
        for n in (0, 1, 2, 53, 54, 107, 108):
            out.append((R.noise(n, p), p))
        for n in _input_lengths(p):
            out.append((R.noise(n, p + 1), p))
    around = {R.resample_length(x.size, p) for x, p in out}
    assert {TILE - 1, TILE, TILE + 1} <= around, sorted(around)
    x = R.noise(1500, 77)                    # a NaN and infinities: they reach the outputs whose support holds them, and no other
    x[40], x[700], x[1400] = np.nan, np.inf, -np.inf
    out.append((x, 707))
    out.append((x, 1999))
    return out


@pytest.mark.parametrize("tempo", [False, True], ids=["alone", "tempo"])
def test_rows_are_the_host_stage_bit_for_bit(pkg, tiny, tempo):
    _, gm = tiny
    rt = pkg.runtime
    cases = _crafted()
    speeds = (None, 800, 1250, 1000)
    rows, po, to = [], [], []
    for i, (x, p) in enumerate(cases):
        s = speeds[i % 4] if tempo else None
        if s is not None and not R.served(s, p):
            s = None
        rows.append(x)
        po.append(rt.PitchOpts(p))
        to.append(None if s is None else rt.TempoOpts(s))
    assert len({o.pitch_permille for o in po}) == len(PITCHES) and (not tempo or sum(t is not None for t in to) >= 20)
    got = gm.pitch_rows(rows, po, to)
    nans = 0
    for i, (x, p, t, g) in enumerate(zip(rows, po, to, got)):
        want = rt.pitch_apply(p, t, x)
        assert g.size == want.size == rt.pitch_length(p, t, x.size), (i, x.size, p.pitch_permille)
        assert _same(g, want), (i, x.size, p.pitch_permille, None if t is None else t.speed_permille, int((_u32(g) != _u32(want)).sum()))
        nans += int(np.isnan(want).sum())
    assert nans >= 50                                                      # the special rows did reach outputs


def test_rows_across_the_table_boundary_and_copies(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    # 260 rows of 481 samples with a pitch, so that the second table runs, and 65 with neither option among them, which are copies
    rows, po, to = [], [], []
    for i in range(325):
        rows.append(R.noise(481, 1000 + i))
        if i % 5 == 4:
            po.append(None)
            to.append(None)
        else:
            p = PITCHES[i % len(PITCHES)]
            po.append(rt.PitchOpts(p))
            to.append(rt.TempoOpts(1250) if i % 3 == 0 and R.served(1250, p) else None)
    assert sum(p is not None for p in po) == 260
    rt.launch_counts(True)
    got = gm.pitch_rows(rows, po, to)
    counts = rt.launch_counts(False)
    assert 0 < sum(t is not None for t in to) <= 256                       # the rows with a tempo behind the resample fill one table
    assert counts.get("k_pitch_resample") == 2 and [counts.get(k) for k in TEMPO_KERNELS] == [1, 1], counts
    for i, (x, p, t, g) in enumerate(zip(rows, po, to, got)):
        want = x if p is None else rt.pitch_apply(p, t, x)
        assert g.size == want.size and np.array_equal(_u32(g), _u32(want)), (i, None if p is None else p.pitch_permille)
    # one array alone; the tempo alone is ptts_tempo_rows; copies and identities launch nothing; a bad row is named
    x = R.tone(5000, 137.0)
    p = rt.PitchOpts(1100)
    assert np.array_equal(_u32(gm.pitch_rows(x, p)), _u32(rt.pitch_apply(p, None, x)))
    assert np.array_equal(_u32(gm.pitch_rows(x, None, rt.TempoOpts(800))), _u32(rt.tempo_apply(rt.TempoOpts(800), x)))
    rt.launch_counts(True)
    assert np.array_equal(_u32(gm.pitch_rows(x, None)), _u32(x))
    assert np.array_equal(_u32(gm.pitch_rows(x, rt.PitchOpts(1000))), _u32(x))
    assert np.array_equal(_u32(gm.pitch_rows(x, rt.PitchOpts(1000), rt.TempoOpts(1000))), _u32(x))
    assert not rt.launch_counts(False)
    rt.launch_counts(True)                                                 # E == 1000: the resample alone
    both = gm.pitch_rows(x, rt.PitchOpts(1250), rt.TempoOpts(1250))
    counts = rt.launch_counts(False)
    assert counts == {"k_pitch_resample": 1}, counts
    assert np.array_equal(_u32(both), _u32(rt.pitch_resample(rt.PitchOpts(1250), x)))
    for bad, words in ((dict(pitch=[p, rt.PitchOpts(2001)]), ("row 1", "pitch_permille")),
                       (dict(pitch=[p, rt.PitchOpts(2000)], tempo=[None, rt.TempoOpts(500)]), ("row 1", "speed_permille 500", "pitch_permille 2000"))):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            gm.pitch_rows([x, x], **bad)
        assert not rt.launch_counts(False)
        assert ei.value.code == rt.PTTS_EINVAL and all(w in str(ei.value) for w in words), str(ei.value)


def _trim_db(pcm):
    """the 99th percentile of the chunks' |x| in dB: a threshold that cuts edges and pauses"""
    v = float(np.quantile(np.abs(np.concatenate(pcm)).astype(np.float64), 0.99))
    assert 0.0 < v < 1.0
    return 20.0 * math.log10(v)


def _check_parts(rt, got, parts, o, steps=STEPS):
    total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
    assert got.pcm.size == total
    assert [p.offset for p in got.parts] == [int(v) for v in offs] and [p.n_samples for p in got.parts] == [p.size for p in parts]
    assert [p.n_frames for p in got.parts] == steps and got.n_frames == sum(steps)          # frames still count what was decoded


@pytest.mark.parametrize("pitch", [800, 1250])
def test_joined_with_pitch_is_the_host_join_of_the_host_stage(pkg, tiny, chunks, pitch):
    _, gm = tiny
    rt = pkg.runtime
    po = rt.PitchOpts(pitch)
    parts = [rt.pitch_apply(po, None, p) for p in chunks]
    E = rt.pitch_speed(po)
    assert E != 1000 and [p.size for p in parts] == [R.length(s * SPF, 1000, pitch) for s in STEPS]
    assert all(abs(p.size - c.size) <= 2 for p, c in zip(parts, chunks))   # the duration stays
    assert not any(np.array_equal(p[:1000], c[:1000]) for p, c in zip(parts, chunks))   # inputs that do not exercise the feature fail
    got = _joined(pkg, gm, rt.JoinOpts(dsp=_with(rt, pitch=po)))
    want = np.concatenate(parts)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    _check_parts(rt, got, parts, rt.JoinOpts())


def test_trim_pitch_tempo_and_gap(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(chunks), pad_ms=5.0, max_pause_ms=20.0)
    po, to = rt.PitchOpts(1100), rt.TempoOpts(1250)
    assert rt.pitch_speed(po, to) == 1136
    trimmed = [rt.trim_apply(trim, p)[0] for p in chunks]
    assert all(0 < t.size < p.size for t, p in zip(trimmed, chunks))       # the pitch reads what the trim left, not the decoder's rows
    parts = [rt.pitch_apply(po, to, t) for t in trimmed]
    want = rt.join(parts, rt.JoinOpts(gap_ms=37.5))
    got = _joined(pkg, gm, rt.JoinOpts(gap_ms=37.5, dsp=_with(rt, trim=trim, tempo=to, pitch=po)))
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    _check_parts(rt, got, parts, rt.JoinOpts(gap_ms=37.5))


def test_pitch_crossfade_chain_and_egress(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    po = rt.PitchOpts(1250)
    parts = [rt.pitch_apply(po, None, p) for p in chunks]
    o = rt.JoinOpts(crossfade_ms=10.0)
    joined = rt.dsp_apply(rt.join(parts, o), normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    want = gm.pcm_encode(gm.resample(joined, 24000, 8000), pkg.PCM_ULAW)
    got = _joined(pkg, gm, rt.JoinOpts(crossfade_ms=10.0, sample_rate=8000, pcm_format=pkg.PCM_ULAW, dsp=_with(rt, pitch=po, normalize=1, fade_in_ms=50.0, fade_out_ms=80.0)))
    assert got.pcm.dtype == want.dtype and got.pcm.size == want.size == rt.resample_length(joined.size, 24000, 8000)
    assert np.array_equal(_bits(got.pcm), _bits(want)), int((_bits(got.pcm) != _bits(want)).sum())
    total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
    assert joined.size == total and [p.offset for p in got.parts] == [int(v) for v in offs]      # parts count 24 kHz samples, whatever the egress
    assert [p.n_samples for p in got.parts] == [p.size for p in parts] and got.n_frames == sum(STEPS)


def test_streamed_with_a_smaller_first_group(pkg, tiny):
    """first_group = 1 at max_batch = 2: groups of 1 + 2.  The hand-overs tile the result, and the result is the host statement over the audio of
    the same groups."""
    _, gm = tiny
    rt = pkg.runtime
    toks, cfgs = _toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS]
    pcm = [np.array(r.pcm, np.float32) for lo, hi in ((0, 1), (1, 3)) for r in gm.generate_batch(toks[lo:hi], cfgs[lo:hi])]
    po = rt.PitchOpts(1100)
    parts = [rt.pitch_apply(po, None, p) for p in pcm]
    want = rt.join(parts, rt.JoinOpts(gap_ms=20.0))
    hand = []
    got = gm.generate_joined(toks, cfgs, rt.JoinOpts(gap_ms=20.0, dsp=_with(rt, pitch=po)), pcm_callback=lambda off, x: hand.append((off, x)), first_group=1)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    _check_parts(rt, got, parts, rt.JoinOpts(gap_ms=20.0))
    at = 0
    for off, x in hand:
        assert off == at and x.size > 0 and x.dtype == got.pcm.dtype, (off, at, x.size)
        at += x.size
    assert at == got.pcm.size and len(hand) == 2
    assert np.array_equal(_bits(np.concatenate([x for _, x in hand])), _bits(got.pcm))


def test_launch_counts(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime

    def counts_of(**kw):
        rt.launch_counts(True)
        res = _joined(pkg, gm, rt.JoinOpts(dsp=_with(rt, **kw)) if kw else None)
        counts = rt.launch_counts(False)
        assert counts.get("k_join") == 2 and not [k for k in counts if k.startswith("k_trim")], counts
        return res, counts.get("k_pitch_resample"), [counts.get(k) for k in TEMPO_KERNELS]

    assert counts_of(pitch=rt.PitchOpts(1250))[1:] == (2, [2, 2])          # E = 800: one launch of each per group
    assert counts_of(pitch=rt.PitchOpts(800), tempo=rt.TempoOpts(1250))[1:] == (2, [2, 2])
    assert counts_of(pitch=rt.PitchOpts(1250), tempo=rt.TempoOpts(1250))[1:] == (2, [None, None])   # E == 1000: no tempo kernel
    assert counts_of(tempo=rt.TempoOpts(1250))[1:] == (None, [2, 2])       # as before
    plain, n_pitch, n_tempo = counts_of()
    assert (n_pitch, n_tempo) == (None, [None, None])
    assert np.array_equal(_u32(plain.pcm), _u32(np.concatenate(chunks)))   # as today
    same, n_pitch, n_tempo = counts_of(pitch=rt.PitchOpts(1000))           # 1000: z is x, nothing is launched for it
    assert (n_pitch, n_tempo) == (None, [None, None]) and np.array_equal(_u32(same.pcm), _u32(plain.pcm))
    d = _with(rt, pitch=rt.PitchOpts(800))
    d._ext.set_pitch(None)                                                 # set and cleared: the handle switches nothing on
    rt.launch_counts(True)
    cleared = _joined(pkg, gm, rt.JoinOpts(dsp=d))
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith(("k_pitch", "k_tempo"))], counts
    assert np.array_equal(_u32(cleared.pcm), _u32(plain.pcm)) and [p.n_samples for p in cleared.parts] == [p.n_samples for p in plain.parts]


def test_refusals_launch_nothing(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    d = _with(rt, pitch=rt.PitchOpts(1100))
    x = R.tone(4000, 200.0)

    def refused(call, *words, count=True):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            call()
        counts = rt.launch_counts(False)
        msg = str(ei.value)
        assert ei.value.code == rt.PTTS_EINVAL and not (count and counts), (msg, counts)
        assert all(w in msg for w in words), msg
        return msg

    words = ("dsp: ext: pitch changes a row's length", "ptts_generate_joined", "ptts_pitch_rows")
    refused(lambda: gm.generate_batch(_toks(1), [_cfg(pkg, 2, dsp_opts=d)]), *words)
    refused(lambda: gm.generate_batch(_toks(1), [_cfg(pkg, 2, dsp_opts=d, pcm_callback=lambda off, s: None)]), *words)   # streaming
    refused(lambda: gm.dsp_rows(x, opts=d), *words)
    refused(lambda: rt.dsp_windows(gm, np.zeros(3840, np.float32), [1920], d), *words)                                     # the debug hook
    refused(lambda: gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2, dsp_opts=d)]), *words)
    for continuous in (False, True):   # (an engine's own thread may launch its set-up while the census is on: the words alone)
        disp = pkg.Dispatcher([gm], max_batch=2, window_us=500, continuous=continuous, cont_kv_capacity=64, cont_max_steps=32)
        try:
            refused(lambda: disp.generate(_toks(1)[0], _cfg(pkg, 2, dsp_opts=d)), *words, count=False)
        finally:
            disp.close()
    # the pair is resolved before anything launches
    both = _with(rt, pitch=rt.PitchOpts(2000), tempo=rt.TempoOpts(500))
    refused(lambda: _joined(pkg, gm, rt.JoinOpts(dsp=both)), "join: pitch", "speed_permille 500", "pitch_permille 2000", "250")
    # a text whose step budgets stay below 2^31 samples as they are and pass it resampled to half the pitch: a part's budget is the decoder's
    # reach (8192 positions of the upsampled sequence), whatever larger step count the request names
    big = 1 << 20
    per_part = 8192 // gm.info.steps_per_latent * gm.info.samples_per_frame
    n = (3 << 29) // per_part                                             # n parts allow about 1.5 * 2^30 samples
    assert 1 <= n <= 4096 and (1 << 30) <= n * per_part < (1 << 31)
    low = _with(rt, pitch=rt.PitchOpts(500))                               # resampled: twice the budget; final (E = 2000): the budget
    msg = refused(lambda: gm.generate_joined(_toks(n), [_cfg(pkg, big)] * n, rt.JoinOpts(dsp=low)), "2^31")
    assert int(re.search(r"allow (\d+) samples", msg).group(1)) == 2 * n * per_part
    # an ext without a pitch behaves as before, and the model serves on
    d._ext.set_pitch(None)
    assert np.array_equal(_u32(gm.dsp_rows(x, opts=d)), _u32(x))
    assert gm.generate_joined(_toks(2), [_cfg(pkg, 2), _cfg(pkg, 2)]).n_frames == 4


def test_tempo_rows_and_pitch_rows_without_a_pitch_are_one_path(pkg, tiny):
    """One row list through ptts_tempo_rows and through ptts_pitch_rows with every pitch null: the same bits from the same launches.  Lengths
    around one hop (480) and one DSP tile (1920), and nothing.  17 speeds on the first 17 rows, so that the first table ends at its design limit
    of 16; 15 of them on the rows behind, enough of them non-empty that the second table ends at its 256 rows and a third runs (rows of no
    samples, and rows whose result is empty, never reach the device: 400 host rows for it)."""
    _, gm = tiny
    rt = pkg.runtime
    lens = (1921, 0, 1, 479, 480, 481, 1919, 1920)
    speeds = [500, 2000, 1000] + [560 + 97 * k for k in range(14)]
    assert len(set(speeds)) == 17 and all(500 <= s <= 2000 for s in speeds)
    rows = [R.noise(lens[i % 8], 3000 + i) for i in range(400)]
    to = [rt.TempoOpts(speeds[i] if i < 17 else speeds[i % 15]) for i in range(400)]
    assert {r.size for r in rows} == set(lens) and len({t.speed_permille for t in to}) == 17
    # the tables the rule cuts (row_tables.h): rows in order, a new table at 256 rows or at a 17th distinct design
    tables, n_rows, designs, by_rows, by_designs = 1, 0, set(), 0, 0
    for x, t in zip(rows, to):
        if R.tempo_length(x.size, t.speed_permille) <= 0:
            continue
        full, many = n_rows == 256, len(designs | {t.speed_permille}) > 16
        if full or many:
            tables, n_rows, designs = tables + 1, 0, set()
            by_rows, by_designs = by_rows + full, by_designs + (many and not full)
        n_rows, designs = n_rows + 1, designs | {t.speed_permille}
    assert (tables, by_rows, by_designs) == (3, 1, 1)
    rt.launch_counts(True)
    a = gm.tempo_rows(rows, to)
    counts_a = rt.launch_counts(False)
    rt.launch_counts(True)
    b = gm.pitch_rows(rows, None, to)
    counts_b = rt.launch_counts(False)
    assert counts_a == counts_b and [counts_a.get(k) for k in TEMPO_KERNELS] == [tables, tables], (counts_a, counts_b)
    for i, (x, t, u, v) in enumerate(zip(rows, to, a, b)):
        assert u.size == v.size == R.tempo_length(x.size, t.speed_permille) and np.array_equal(_u32(u), _u32(v)), (i, x.size, t.speed_permille)
    for i in (2, 7, 399):                                                  # and what both give is the host statement (a row at speed 1000 among them)
        assert np.array_equal(_u32(a[i]), _u32(rt.tempo_apply(to[i], rows[i]))), i
    assert to[2].speed_permille == 1000 and rows[7].size == 1920 and rows[399].size == 1920


def _refusal(pkg, call):
    rt = pkg.runtime
    rt.launch_counts(True)
    with pytest.raises(pkg.PttsError) as ei:
        call()
    assert ei.value.code == rt.PTTS_EINVAL and not rt.launch_counts(False)
    return str(ei.value)


def test_refusal_texts_of_the_tempo_and_pitch_rows(pkg, tiny):
    """Every refusal site of ptts_tempo_rows and ptts_pitch_rows, byte for byte as the entry points worded them before they shared one path.  The
    lengths of 2^31 and around are refused before any row is read: the rows behind them hold one sample."""
    _, gm = tiny
    rt = pkg.runtime
    L = rt.lib()
    x = R.tone(2000, 200.0)
    one = np.zeros(1, np.float32)
    t8, p11 = rt.TempoOpts(800), rt.PitchOpts(1100)

    def tempo(t, rows, n=None, outs=None, null=None):
        pp = rt._row_ptrs(rows)
        po = (C.POINTER(rt.TempoOpts) * len(t))(*[None if o is None else C.pointer(o) for o in t])
        outs = rt._row_ptrs(outs if outs is not None else [np.empty(2 * r.size + 1, np.float32) for r in rows])
        ns = np.array([r.size for r in rows] if n is None else n, np.int64)
        got = np.zeros(len(rows), np.int64)
        args = dict(t=po, rows=pp, n=rt._ip(ns), out=outs, n_out=rt._ip(got))
        if null:
            args[null] = None
        rt._check(L.ptts_tempo_rows(gm.h, args["t"], args["rows"], args["n"], len(rows), args["out"], args["n_out"]))

    def pitch(p, t, rows, n=None, outs=None, null=None):
        pp = rt._row_ptrs(rows)
        pa = (C.POINTER(rt.PitchOpts) * len(p))(*[None if o is None else C.pointer(o) for o in p])
        ta = (C.POINTER(rt.TempoOpts) * len(t))(*[None if o is None else C.pointer(o) for o in t])
        outs = rt._row_ptrs(outs if outs is not None else [np.empty(4 * r.size + 1, np.float32) for r in rows])
        ns = np.array([r.size for r in rows] if n is None else n, np.int64)
        got = np.zeros(len(rows), np.int64)
        args = dict(p=pa, t=ta, rows=pp, n=rt._ip(ns), out=outs, n_out=rt._ip(got))
        if null:
            args[null] = None
        rt._check(L.ptts_pitch_rows(gm.h, args["p"], args["t"], args["rows"], args["n"], len(rows), args["out"], args["n_out"]))

    for null in ("t", "rows", "n", "out", "n_out"):
        assert _refusal(pkg, lambda: tempo([t8], [x], null=null)) == "ptts-hip: tempo: null argument"
    for null in ("p", "t", "rows", "n", "out", "n_out"):
        assert _refusal(pkg, lambda: pitch([p11], [None], [x], null=null)) == "ptts-hip: pitch: null argument"
    assert _refusal(pkg, lambda: tempo([t8, t8], [x, x], n=[x.size, -1])) == "ptts-hip: tempo: row 1 is negative or null"
    assert _refusal(pkg, lambda: pitch([p11, p11], [None, None], [x, x], n=[x.size, -1])) == "ptts-hip: pitch: row 1 is negative or null"
    assert _refusal(pkg, lambda: tempo([t8, rt.TempoOpts(2001)], [x, x])) == "ptts-hip: row 1: tempo: speed_permille 2001 is not from 500 to 2000 (1000: unchanged)"
    assert _refusal(pkg, lambda: pitch([p11, rt.PitchOpts(499)], [None, None], [x, x])) == "ptts-hip: row 1: pitch: pitch_permille 499 is not from 500 to 2000 (1000: unchanged)"
    assert _refusal(pkg, lambda: pitch([None, None], [t8, rt.TempoOpts(2001)], [x, x])) == "ptts-hip: row 1: tempo: speed_permille 2001 is not from 500 to 2000 (1000: unchanged)"
    assert _refusal(pkg, lambda: tempo([None, t8], [x, x], outs=[x.copy(), x])) == "ptts-hip: tempo: row 1: out is in"
    assert _refusal(pkg, lambda: pitch([None, p11], [None, None], [x, x], outs=[x.copy(), x])) == "ptts-hip: row 1: pitch: out is in"
    assert _refusal(pkg, lambda: pitch([None, None], [None, t8], [x, x], outs=[x.copy(), x])) == "ptts-hip: row 1: pitch: out is in"
    assert (_refusal(pkg, lambda: pitch([p11, rt.PitchOpts(2000)], [None, rt.TempoOpts(500)], [x, x]))
            == "ptts-hip: row 1: pitch: speed_permille 500 with pitch_permille 2000 needs the tempo at 250, which is not from 500 to 2000")
    assert (_refusal(pkg, lambda: pitch([p11, rt.PitchOpts(500)], [None, rt.TempoOpts(1500)], [x, x]))
            == "ptts-hip: row 1: pitch: speed_permille 1500 with pitch_permille 500 needs the tempo at 3000, which is not from 500 to 2000")
    # the lengths, refused before a row is read
    big = (1 << 31) - 240
    assert _refusal(pkg, lambda: tempo([None, t8], [one, one], n=[1, big], outs=[one.copy(), one.copy()])) == f"ptts-hip: tempo: row 1 has {big} samples, a row must stay below 2^31 - 240"
    assert _refusal(pkg, lambda: pitch([None, None], [None, t8], [one, one], n=[1, big], outs=[one.copy(), one.copy()])) == f"ptts-hip: row 1: tempo: {big} samples, a row must stay below 2^31 - 240"
    assert (_refusal(pkg, lambda: pitch([None, rt.PitchOpts(500)], [None, None], [one, one], n=[1, 1 << 30], outs=[one.copy(), one.copy()]))
            == f"ptts-hip: row 1: pitch: n {1 << 30} at pitch_permille 500 has the resampled length {1 << 31}, a row must stay below 2^31 - 240")
    assert (_refusal(pkg, lambda: pitch([None, rt.PitchOpts(1000)], [None, rt.TempoOpts(500)], [one, one], n=[1, 1 << 30], outs=[one.copy(), one.copy()]))
            == f"ptts-hip: row 1: pitch: n {1 << 30} at pitch_permille 1000 and the tempo at 500 has the final length {1 << 31}, a row must stay below 2^31 - 240")
    assert (_refusal(pkg, lambda: pitch([None, p11], [None, None], [one, one], n=[1, 1 << 33], outs=[one.copy(), one.copy()]))
            == f"ptts-hip: row 1: pitch: n {1 << 33} is not from 0 to where its lengths stay below 2^31 - 240")
    # the model serves on
    assert np.array_equal(_u32(gm.pitch_rows(x, None, t8)), _u32(rt.tempo_apply(t8, x)))


def test_a_dead_handle_is_refused_under_the_setters_name(pkg):
    rt = pkg.runtime
    ext = rt.DspExt()
    h = ext.h
    ext.free()
    assert ext.h is None
    ext.h = h                                                              # (the registry knows the handle is gone: it is not read)
    try:
        for stage, call in (("compressor", lambda: ext.set_compressor(rt.CompressorOpts())), ("limiter", lambda: ext.set_limiter(rt.LimiterOpts())),
                            ("trim", lambda: ext.set_trim(rt.TrimOpts())), ("tempo", lambda: ext.set_tempo(rt.TempoOpts(800))),
                            ("pitch", lambda: ext.set_pitch(rt.PitchOpts(1100))), ("trim", lambda: ext.set_trim(None))):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and str(ei.value) == f"ptts-hip: {stage}: ext {h:#x} is not a live handle of ptts_dsp_ext_create"
    finally:
        ext.h = None
    # a live handle refuses bad options by the stage's own check, and keeps what it had
    live = rt.DspExt(tempo=rt.TempoOpts(800))
    with pytest.raises(pkg.PttsError) as ei:
        live.set_tempo(rt.TempoOpts(2001))
    assert str(ei.value) == "ptts-hip: tempo: speed_permille 2001 is not from 500 to 2000 (1000: unchanged)"


_TRACE_CHILD = """
import sys
import ptts_amd
pkg = ptts_amd.load()
rt = pkg.runtime
gm = pkg.Model.open(sys.argv[1], device=0, max_batch=2)
gm.profile_enable(2)
d = rt.DspOpts(0, 0, 0.0, 0.0)
ext = rt.DspExt(trim=rt.TrimOpts(edges=1, threshold_db=float(sys.argv[2]), pad_ms=5.0, max_pause_ms=20.0), tempo=rt.TempoOpts(800), pitch=rt.PitchOpts(1100))
d.ext = ext.h
cfgs = [pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=s, temperature=0.0) for s in (2, 4, 3)]
res = gm.generate_joined([[3 + i % 40, 7, 11 + i % 40] for i in range(3)], cfgs, rt.JoinOpts(dsp=d))
ph = gm.profile_read()
gm.profile_enable(0)
print("frames", res.n_frames, "parts", [p.n_samples for p in res.parts], "profile", sorted(k for k in ph if k.endswith("_ms")))
gm.close()
"""


def test_the_phases_of_a_joined_call(pkg, tiny, chunks, tmp_path):
    """A joined call with a trim, pitch 1100 and speed 800, measured (profile_enable(2)) and traced, names its part stages as before: per group
    `trim`, `pitch`, `tempo` and `join`, in that order, each behind its launches.  ptts_profile_read's record has fixed times (the timed launches' total; prefill, AR
    loop, decoder) and no named phases; the names are those of the call's host trace (PTTS_TRACE=1, read once per process: hence the child)."""
    import os
    import subprocess
    import sys
    cfg, gm = tiny
    rt = pkg.runtime
    synth = pkg.synth
    tensors = synth.make_checkpoint(cfg, seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path / "tiny_quiet.safetensors")
    synth.write_safetensors(path, tensors)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", _TRACE_CHILD, path, repr(_trim_db(chunks))], capture_output=True, text=True, cwd=root, timeout=120,
                         env=dict(os.environ, PTTS_TRACE="1"))
    assert run.returncode == 0, run.stderr
    marks = re.findall(r"^\[ptts\] (.+?)\s+[0-9.]+ ms$", run.stderr, re.M)
    print("phases:", marks)
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(chunks), pad_ms=5.0, max_pause_ms=20.0)
    want = [rt.pitch_apply(rt.PitchOpts(1100), rt.TempoOpts(800), rt.trim_apply(trim, p)[0]).size for p in chunks]
    assert f"frames {sum(STEPS)} parts {want} profile ['ar_loop_ms', 'mimi_ms', 'prefill_ms', 'total_ms']" in run.stdout, run.stdout
    assert [m for m in marks if m in ("trim", "pitch", "tempo", "join")] == ["trim", "pitch", "tempo", "join"] * 2, marks   # two groups
