"""Keep the formants, on the GPU (go-pocket-tts_amd/csrc/formant.hip, dsp_device.cpp parts_launch, generate.cpp generate_joined; include/ptts.h
ptts_formant_opts): ptts_formant_rows gives ptts_formant_apply's bits (outside NaN outputs) on rows around every length at
which a kernel takes another path -- less than a whiten tile's first half, one frame and one more, less than a window and more, one DSP tile, and 21
frames, which is more than the 16 tiles of one shape wave -- at the ends of the served pitches and next to 1000, with and without a tempo; rows with
the option, with a pitch alone and with nothing mixed in one call; 260 rows, four more than a table holds; a row with a NaN and infinities; a joined
call with a trim, a pitch, the option and a gap is the host join of the host stage, streamed too; the launches are one of each formant kernel per
table of rows with the option and none without it; refusals launch nothing.

The tiny checkpoint's last convolution is scaled by 2^-6 here, as test_gpu_pitch.py does."""
import math

import numpy as np
import pytest

import _formant_ref as F
import _pitch_ref as R

pytestmark = pytest.mark.gpu

SPF = 1920
STEPS = [2, 4, 3]            # three parts, two groups at max_batch = 2
LENGTHS = (1, 119, 121, 241, 719, 721, 1920, 4801)
PITCHES = (800, 999, 1001, 1250, 1500)
FORMANT_KERNELS = ("k_formant_analyse", "k_formant_whiten", "k_formant_shape")
TEMPO_KERNELS = ("k_tempo_plan", "k_tempo_store")


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    tensors = synth.make_checkpoint(cfg, seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("formant") / "tiny_quiet.safetensors")
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


def _with(rt, trim=None, tempo=None, pitch=None, formant=None):
    """a DspOpts whose ext carries the part stages (the handle lives as long as the struct)"""
    d = rt.DspOpts(0, 0, 0.0, 0.0)
    d._ext = rt.DspExt(trim=trim, tempo=tempo, pitch=pitch, formant=formant)
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


@pytest.mark.parametrize("speed", [None, 800, 1250], ids=["alone", "tempo800", "tempo1250"])
def test_rows_are_the_host_stage_bit_for_bit(pkg, tiny, speed):
    _, gm = tiny
    rt = pkg.runtime
    keep = rt.FormantOpts(1)
    to = None if speed is None else rt.TempoOpts(speed)
    rows, po = [], []
    for n in LENGTHS:
        for p in PITCHES:
            rows.append(F.noise(n, 100 + p) if (n + p) % 2 else np.ascontiguousarray(F.vowel(*F.VOWEL_B, n=max(n, 2000))[-n:]))
            po.append(rt.PitchOpts(p))
    got = gm.formant_rows(rows, keep, po, to)
    differs = 0
    for x, p, g in zip(rows, po, got):
        want = rt.formant_apply(keep, p, to, x)
        assert g.size == want.size == rt.pitch_length(p, to, x.size), (x.size, p.pitch_permille)
        assert np.array_equal(_u32(g), _u32(want)), (x.size, p.pitch_permille, speed, int((_u32(g) != _u32(want)).sum()))
        plain = rt.pitch_apply(p, to, x)
        differs += int(not np.array_equal(_u32(plain), _u32(want)))
    assert differs >= len(rows) - len(PITCHES)                             # the option did something on (nearly) every row


def test_mixed_rows(pkg, tiny):
    """one call: rows with the option, rows with a pitch alone (no options, keep 0, or a pitch of 1000 under the option), rows with a tempo alone and
    rows with nothing"""
    _, gm = tiny
    rt = pkg.runtime
    keep, off = rt.FormantOpts(1), rt.FormantOpts(0)
    kinds = [(keep, 1250, None), (None, 1250, None), (None, None, None), (off, 800, 1250), (keep, 800, 1250), (keep, 1000, None), (None, None, 800),
             (keep, None, 800), (keep, 1500, None), (keep, 1000, 1250)]
    rows, fo, po, to = [], [], [], []
    for i in range(30):
        f, p, s = kinds[i % len(kinds)]
        rows.append(F.noise(700 + 37 * i, 300 + i))
        fo.append(f)
        po.append(None if p is None else rt.PitchOpts(p))
        to.append(None if s is None else rt.TempoOpts(s))
    rt.launch_counts(True)
    got = gm.formant_rows(rows, fo, po, to)
    counts = rt.launch_counts(False)
    assert [counts.get(k) for k in FORMANT_KERNELS] == [1, 1, 1] and counts.get("k_pitch_resample") == 1, counts
    for i, (x, f, p, t, g) in enumerate(zip(rows, fo, po, to, got)):
        if p is None:
            want = x if t is None else rt.tempo_apply(t, x)
        elif f is None:
            want = rt.pitch_apply(p, t, x)
        else:
            want = rt.formant_apply(f, p, t, x)
        assert g.size == want.size and np.array_equal(_u32(g), _u32(want)), (i, kinds[i % len(kinds)])
    # the same rows through ptts_pitch_rows: the rows without the option are the same bits from the same call
    plain = gm.pitch_rows(rows, po, to)
    for i, (f, p, g, q) in enumerate(zip(fo, po, got, plain)):
        served = f is not None and f.keep and p is not None and p.pitch_permille != 1000
        assert np.array_equal(_u32(g), _u32(q)) != served, i


def test_rows_across_the_table_boundary(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    keep = rt.FormantOpts(1)
    rows = [F.noise(481, 1000 + i) for i in range(260)]                    # four more than a table holds
    po = [rt.PitchOpts(PITCHES[i % len(PITCHES)]) for i in range(260)]
    rt.launch_counts(True)
    got = gm.formant_rows(rows, keep, po)
    counts = rt.launch_counts(False)
    assert [counts.get(k) for k in FORMANT_KERNELS] == [2, 2, 2] and counts.get("k_pitch_resample") == 2, counts
    for i in list(range(0, 260, 7)) + [255, 256, 257, 258, 259]:
        assert np.array_equal(_u32(got[i]), _u32(rt.formant_apply(keep, po[i], None, rows[i]))), i


def test_a_row_with_a_nan_and_infinities(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    keep = rt.FormantOpts(1)
    x = F.noise(4801, 77).copy()
    x[40], x[2000], x[2010], x[3000], x[3001] = np.nan, np.inf, -np.inf, 1e-42, -1e-40
    nans = 0
    for p, s in ((800, None), (1250, None), (1500, 1250)):
        po, to = rt.PitchOpts(p), None if s is None else rt.TempoOpts(s)
        want = rt.formant_apply(keep, po, to, x)
        got = gm.formant_rows(x, keep, po, to)
        assert _same(got, want), (p, s, int((_u32(got) != _u32(want)).sum()))
        nans += int(np.isnan(want).sum())
        assert np.isfinite(want).sum() > want.size // 5                    # two places of about 1000 outputs each: what they reach is bounded
    assert nans >= 100


def _trim_db(pcm):
    v = float(np.quantile(np.abs(np.concatenate(pcm)).astype(np.float64), 0.99))
    assert 0.0 < v < 1.0
    return 20.0 * math.log10(v)


def test_joined_with_trim_pitch_option_and_gap(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(chunks), pad_ms=5.0, max_pause_ms=20.0)
    keep, po = rt.FormantOpts(1), rt.PitchOpts(1250)
    trimmed = [rt.trim_apply(trim, p)[0] for p in chunks]
    assert all(0 < t.size < p.size for t, p in zip(trimmed, chunks))
    parts = [rt.formant_apply(keep, po, None, t) for t in trimmed]
    assert not any(np.array_equal(p, rt.pitch_apply(po, None, t)) for p, t in zip(parts, trimmed))   # inputs that do not exercise the feature fail
    o = rt.JoinOpts(gap_ms=37.5)
    want = rt.join(parts, o)
    got = _joined(pkg, gm, rt.JoinOpts(gap_ms=37.5, dsp=_with(rt, trim=trim, pitch=po, formant=keep)))
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    total, offs = rt.join_length([p.size for p in parts], o, offsets=True)
    assert [p.offset for p in got.parts] == [int(v) for v in offs] and [p.n_samples for p in got.parts] == [p.size for p in parts]
    assert [p.n_frames for p in got.parts] == STEPS and got.n_frames == sum(STEPS)


def test_streamed_with_a_smaller_first_group(pkg, tiny):
    """first_group = 1 at max_batch = 2: groups of 1 + 2.  The hand-overs tile the result, and the result is the host statement over the audio of
    the same groups."""
    _, gm = tiny
    rt = pkg.runtime
    toks, cfgs = _toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS]
    pcm = [np.array(r.pcm, np.float32) for lo, hi in ((0, 1), (1, 3)) for r in gm.generate_batch(toks[lo:hi], cfgs[lo:hi])]
    keep, po, to = rt.FormantOpts(1), rt.PitchOpts(1250), rt.TempoOpts(1100)
    parts = [rt.formant_apply(keep, po, to, p) for p in pcm]
    want = rt.join(parts, rt.JoinOpts(gap_ms=20.0))
    hand = []
    got = gm.generate_joined(toks, cfgs, rt.JoinOpts(gap_ms=20.0, dsp=_with(rt, pitch=po, tempo=to, formant=keep)), pcm_callback=lambda off, x: hand.append((off, x)),
                             first_group=1)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    at = 0
    for off, x in hand:
        assert off == at and x.size > 0, (off, at, x.size)
        at += x.size
    assert at == got.pcm.size and len(hand) == 2
    assert np.array_equal(_bits(np.concatenate([x for _, x in hand])), _bits(got.pcm))


def test_launch_counts(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime

    def counts_of(**kw):
        rt.launch_counts(True)
        res = _joined(pkg, gm, None if kw.pop("no_opts", False) else rt.JoinOpts(dsp=_with(rt, **kw)))
        counts = rt.launch_counts(False)
        assert counts.get("k_join") == 2, counts
        return res, counts

    keep = rt.FormantOpts(1)
    plain, none = counts_of(no_opts=True)
    empty, base = counts_of()                                              # a handle that switches nothing on: the egress of a call with options
    assert not [k for k in list(base) + list(none) if k.startswith(("k_formant", "k_pitch", "k_tempo"))], (base, none)
    assert np.array_equal(_u32(empty.pcm), _u32(plain.pcm))
    shifted, pitch_alone = counts_of(pitch=rt.PitchOpts(1250))             # exactly today's: E = 800, one launch of each per group
    assert pitch_alone.get("k_pitch_resample") == 2 and [pitch_alone.get(k) for k in TEMPO_KERNELS] == [2, 2]
    assert {k: v for k, v in pitch_alone.items() if k not in ("k_pitch_resample",) + TEMPO_KERNELS} == base, (pitch_alone, base)
    for off in (dict(pitch=rt.PitchOpts(1250), formant=rt.FormantOpts(0)),):
        same, counts = counts_of(**off)
        assert counts == pitch_alone and np.array_equal(_u32(same.pcm), _u32(shifted.pcm))
    kept, counts = counts_of(pitch=rt.PitchOpts(1250), formant=keep)       # one launch of each per group's table of rows, the resample as before
    assert [counts.get(k) for k in FORMANT_KERNELS] == [2, 2, 2], counts
    assert {k: v for k, v in counts.items() if k not in FORMANT_KERNELS} == pitch_alone, (counts, pitch_alone)
    assert kept.pcm.size == shifted.pcm.size and not np.array_equal(_u32(kept.pcm), _u32(shifted.pcm))
    assert np.array_equal(_u32(kept.pcm), _u32(np.concatenate([rt.formant_apply(keep, rt.PitchOpts(1250), None, c) for c in chunks])))
    for nothing in (dict(formant=keep), dict(pitch=rt.PitchOpts(1000), formant=keep)):   # no pitch, or 1000: nothing is computed
        same, counts = counts_of(**nothing)
        assert counts == base and np.array_equal(_u32(same.pcm), _u32(plain.pcm)), counts
    same, counts = counts_of(tempo=rt.TempoOpts(1250), formant=keep)       # the tempo alone, as before
    assert not [k for k in counts if k.startswith(("k_formant", "k_pitch"))] and [counts.get(k) for k in TEMPO_KERNELS] == [2, 2], counts


def test_refusals_launch_nothing(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    x = R.tone(4000, 200.0)
    keep = rt.FormantOpts(1)

    def refused(call, *words):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            call()
        counts = rt.launch_counts(False)
        msg = str(ei.value)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (msg, counts)
        assert all(w in msg for w in words), msg

    # the pair (option, pitch) is resolved before anything launches
    for p in (799, 1501, 667):
        refused(lambda: _joined(pkg, gm, rt.JoinOpts(dsp=_with(rt, pitch=rt.PitchOpts(p), formant=keep))), "join: formant", "keep 1", "pitch_permille %d" % p)
        refused(lambda: gm.formant_rows([x, x], keep, [rt.PitchOpts(1250), rt.PitchOpts(p)]), "row 1", "keep 1", "pitch_permille %d" % p)
    refused(lambda: gm.formant_rows([x, x], [keep, rt.FormantOpts(2)], rt.PitchOpts(1250)), "row 1", "formant: keep 2")
    refused(lambda: gm.formant_rows([x, x], [keep, rt.FormantOpts(1, reserved=(0, 1))], rt.PitchOpts(1250)), "row 1", "formant: reserved")
    refused(lambda: gm.formant_rows([x, x], keep, [rt.PitchOpts(1250), rt.PitchOpts(2001)]), "row 1", "pitch_permille 2001")
    refused(lambda: gm.formant_rows([x, x], keep, [rt.PitchOpts(1250), rt.PitchOpts(1500)], [None, rt.TempoOpts(500)]), "row 1", "speed_permille 500", "pitch_permille 1500")
    L = rt.lib()
    rt.launch_counts(True)
    assert L.ptts_formant_rows(gm.h, None, None, None, None, None, 1, None, None) == rt.PTTS_EINVAL and "formant: null argument" in L.ptts_last_error().decode()
    assert not rt.launch_counts(False)
    # every other entry point refuses the handle by the pitch's own words
    d = _with(rt, pitch=rt.PitchOpts(1100), formant=keep)
    words = ("dsp: ext: pitch changes a row's length", "ptts_generate_joined", "ptts_pitch_rows")
    refused(lambda: gm.generate_batch(_toks(1), [_cfg(pkg, 2, dsp_opts=d)]), *words)
    refused(lambda: gm.dsp_rows(x, opts=d), *words)
    # outside the range without the option, every pitch is served as before; and the model serves on
    assert np.array_equal(_u32(gm.formant_rows(x, rt.FormantOpts(0), rt.PitchOpts(2000))), _u32(rt.pitch_apply(rt.PitchOpts(2000), None, x)))
    assert np.array_equal(_u32(gm.formant_rows(x, keep, rt.PitchOpts(1250))), _u32(rt.formant_apply(keep, rt.PitchOpts(1250), None, x)))
