"""Per-part prosody for joined synthesis, on the GPU (go-pocket-tts_amd/csrc/join.hip k_join_gain, dsp_device.cpp level_launch / join_gain_launch,
generate.cpp generate_joined; include/ptts.h ptts_part_opts): ptts_join_parts_rows gives ptts_join_parts' bits at every
destination alignment, with mixed seams, with gains on none, one or both sides of a seam, across the 256-row table turn and with the level rows; a
joined call with a list is the host statement (per part trim -> pitch with or without formants -> tempo -> volume, then ptts_join_parts) for the
audio, the part records and the gains, in one piece and handed over group by group; a list of defaults is the call without a list, byte for byte and
launch for launch; refusals launch nothing; a level on the call.

The tiny checkpoint's last convolution is scaled by 2^-6 here, as test_gpu_pitch.py does (its audio peaks near 3.0 otherwise)."""
import math

import numpy as np
import pytest

import _join_parts_ref as R
import _join_ref as J

pytestmark = pytest.mark.gpu

SPF = 1920
STEPS = [2, 5, 3, 4, 1, 6]   # two groups at max_batch = 4


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    tensors = synth.make_checkpoint(synth.SynthConfig.tiny(), seed=1234)
    for k in ("mimi.decoder.model.11.conv.weight", "mimi.decoder.model.11.conv.bias"):
        tensors[k] = (tensors[k] * np.float32(2.0 ** -6)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("join_parts") / "tiny_quiet.safetensors")
    synth.write_safetensors(path, tensors)
    gm = pkg.Model.open(path, device=0, max_batch=4)
    yield gm
    gm.close()


def _cfg(pkg, steps, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, **kw)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _records(parts):
    return [(p.offset, p.n_samples, p.n_frames, p.eos_step, p.status) for p in parts]


def _rows_equal_host(rt, gm, parts, po, join=None, differs=True):
    want, g_want = rt.join_parts(parts, po, join, gains=True)
    got, g = gm.join_parts_rows(parts, po, join, gains=True)
    assert got.size == want.size and np.array_equal(_u32(got), _u32(want)), int((_u32(got) != _u32(want)).sum())
    assert np.array_equal(_u32(g), _u32(g_want)), (g, g_want)
    if differs:   # inputs that do not exercise the feature fail
        plain = rt.join(parts, join)
        assert plain.size != want.size or not np.array_equal(_u32(plain), _u32(want))
    return got, g


def test_rows_at_every_destination_alignment(pkg, tiny):
    """lengths 1 .. 9 against gaps of 0, 1, 3 and 900 samples: a part lands on every offset of the destination's 16-byte grid, with a group cut by
    the span's edge on either side; every second part has a gain"""
    rt = pkg.runtime
    rng = np.random.default_rng(1)
    for gap in (0, 1, 3, 900):
        gap_ms = (gap + 0.5) / 24.0 if gap else 0.0                          # (half a sample of room: the count truncates)
        assert J.samples(gap_ms) == gap
        for first in range(1, 10):
            lengths = [first] + [1 + (first + i) % 9 for i in range(9)] + [2000 + first]
            parts = [(0.1 * (i + 1) + 0.25 * rng.standard_normal(n)).astype(np.float32) for i, n in enumerate(lengths)]
            po = [rt.PartOpts(gain_db=(-6.0 if i % 2 else 0.0), gap_ms=gap_ms) for i in range(len(parts))]
            _rows_equal_host(rt, tiny, parts, po)


def test_rows_with_mixed_seams_and_gains_on_either_side(pkg, tiny):
    """_join_ref's orders under the cycles of _join_parts_ref: gaps and crossfades in one list, a gain on none, one or both sides of a crossfade"""
    rt = pkg.runtime
    sides = set()
    for oi, lengths in enumerate(J.ORDERS):
        parts = J.parts_for(lengths, seed=60 + oi)
        for shift in range(3):
            pairs, gains_db = R.cycle(len(lengths), shift)
            default = (37.5, 0.0) if shift == 1 else (0.0, 10.0) if shift == 2 else (0.0, 0.0)
            o = rt.JoinOpts(gap_ms=default[0], crossfade_ms=default[1])
            po = [rt.PartOpts(gain_db=db, gap_ms=g, crossfade_ms=c) for (g, c), db in zip(pairs, gains_db)]
            got, _ = _rows_equal_host(rt, tiny, parts, po, o)
            ref, _ = R.statement(parts, pairs, gains_db, default)
            assert np.array_equal(_u32(got), _u32(ref))                      # and the independent restatement
            seams = [R.seam_pair(a, b, default) for a, b in pairs]
            for i in range(len(lengths) - 1):
                if J.seam(seams[i][1], lengths[i], lengths[i + 1]) > 0:
                    sides.add((gains_db[i] != 0.0, gains_db[i + 1] != 0.0))
    assert sides == {(False, False), (False, True), (True, False), (True, True)}, sides


def test_rows_across_the_table_turn(pkg, tiny):
    """300 rows of 1 .. 7 samples: the 256-row table and the 44 rows behind it, a seam and a gain on both sides of the turn"""
    rt = pkg.runtime
    rng = np.random.default_rng(2)
    lengths = [1 + (3 * i) % 7 for i in range(300)]
    parts = [(0.01 * (i + 1) + 0.25 * rng.standard_normal(n)).astype(np.float32) for i, n in enumerate(lengths)]
    po = [rt.PartOpts(gain_db=(3.0, -6.0, 0.0)[i % 3], gap_ms=(-1.0 if i % 2 else 1.5 / 24.0), crossfade_ms=(3.5 / 24.0 if i % 2 else -1.0)) for i in range(300)]
    assert po[255].gain_db != 0.0 and po[256].gain_db != 0.0 and J.seam(3, lengths[255], lengths[256]) > 0
    rt.launch_counts(True)
    _rows_equal_host(rt, tiny, parts, po)
    counts = rt.launch_counts(False)
    assert counts == {"k_join_gain": 2}, counts
    # a table without a gain goes to k_join: the first 256 rows here have none
    po = [rt.PartOpts(gain_db=(3.0 if i >= 256 else 0.0), gap_ms=1.5 / 24.0) for i in range(300)]
    rt.launch_counts(True)
    _rows_equal_host(rt, tiny, parts, po)
    counts = rt.launch_counts(False)
    assert counts == {"k_join": 1, "k_join_gain": 1}, counts


def test_rows_with_levels(pkg, tiny):
    """the level rows of test_join_parts_cpu.py (which asserts their preconditions on the CPU): the gain the measuring kernels leave on the device is
    the host's, the ceiling and a part that passes no gate included; nothing rewrites the samples in front of the join"""
    rt = pkg.runtime
    parts = R.level_parts() + [R.level_parts()[0][:9599].copy(), J.parts_for([4801], seed=9)[0]]
    assert all(math.isfinite(rt.loudness(p)) for p in parts[:3])
    lv = R.LEVEL_TARGET
    po = [rt.PartOpts(level=lv, gap_ms=0.0), rt.PartOpts(level=lv, crossfade_ms=10.0), rt.PartOpts(level=lv, crossfade_ms=10.0), rt.PartOpts(level=lv, gap_ms=37.5),
          rt.PartOpts(gain_db=-6.0)]
    rt.launch_counts(True)
    _, g = _rows_equal_host(rt, tiny, parts, po)
    counts = rt.launch_counts(False)
    assert counts == {"k_dsp_peak": 1, "k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1, "k_join_gain": 1}, counts
    assert _u32(g)[2] == _u32(np.float32(1.0) / np.abs(parts[2]).max()) and g[0] != 1.0 and g[1] != 1.0 and g[3] == 1.0


# ---- the joined call ----

def _trim_db(pcm):
    v = float(np.quantile(np.abs(np.concatenate(pcm)).astype(np.float64), 0.99))
    assert 0.0 < v < 1.0
    return 20.0 * math.log10(v)


def _mixed_list(rt, trim):
    """one PartOpts per part of STEPS: a trim on some parts, tempo 800 and 1250, pitch 1100 with and without the formants, gains of -6 and +3 dB, a gap
    of 0, a gap of 37.5 ms, crossfades of 10 ms -- one of them across the group boundary behind part 3, where the gain changes from -6 to +3 dB --
    and the pair of the join options behind part 4"""
    keep, p11 = rt.FormantOpts(1), rt.PitchOpts(1100)
    return [rt.PartOpts(trim=trim, tempo=rt.TempoOpts(800), gain_db=-6.0, gap_ms=0.0),
            rt.PartOpts(pitch=p11, formant=keep, gap_ms=37.5),
            rt.PartOpts(pitch=p11, tempo=rt.TempoOpts(1250), gain_db=3.0, crossfade_ms=10.0),
            rt.PartOpts(trim=trim, gain_db=-6.0, crossfade_ms=10.0),
            rt.PartOpts(gain_db=3.0),
            rt.PartOpts(tempo=rt.TempoOpts(800))]


def _host_statement(rt, chunks, po, join):
    """per part trim_apply -> formant_apply / pitch_apply / tempo_apply -> (volume and join) join_parts: (audio, gains, offsets, lengths)"""
    parts = []
    for x, o in zip(chunks, po):
        trim, pitch, formant, tempo = o._borrowed
        if trim is not None:
            x = rt.trim_apply(trim, x)[0]
        if pitch is not None and formant is not None:
            x = rt.formant_apply(formant, pitch, tempo, x)
        elif pitch is not None:
            x = rt.pitch_apply(pitch, tempo, x)
        elif tempo is not None:
            x = rt.tempo_apply(tempo, x)
        parts.append(np.ascontiguousarray(x, np.float32))
    want, g = rt.join_parts(parts, po, join, gains=True)
    _, offs = rt.join_parts_length([p.size for p in parts], po, join, offsets=True)
    return want, g, [int(v) for v in offs], [p.size for p in parts]


def _batches(pkg, gm, groups):
    """the chunks' own 24 kHz audio from one generate_batch call per group"""
    toks, cfgs = _toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS]
    pcm = [np.array(r.pcm, np.float32) for lo, hi in groups for r in gm.generate_batch(toks[lo:hi], cfgs[lo:hi])]
    for p, s in zip(pcm, STEPS):
        assert p.size == s * SPF
        p.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def chunks(pkg, tiny):
    """from ONE generate_batch call (which groups as the joined call does): computed once, never written to"""
    return _batches(pkg, tiny, [(0, len(STEPS))])


def test_a_joined_call_with_a_mixed_list_is_the_host_statement(pkg, tiny, chunks):
    rt = pkg.runtime
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(chunks), pad_ms=5.0, max_pause_ms=20.0)
    po = _mixed_list(rt, trim)
    o = rt.JoinOpts(gap_ms=20.0)
    want, g, offs, lens = _host_statement(rt, chunks, po, o)
    assert lens[0] < rt.tempo_length(rt.TempoOpts(800), chunks[0].size) and lens[3] < chunks[3].size          # the trims cut something
    assert not np.array_equal(want, _host_statement(rt, chunks, [rt.PartOpts(trim=p._borrowed[0], pitch=p._borrowed[1], formant=p._borrowed[2], tempo=p._borrowed[3],
                                                                             gap_ms=p.gap_ms, crossfade_ms=p.crossfade_ms) for p in po], o)[0])   # ... and the gains change it
    got = tiny.generate_joined(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS], o, parts=po)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    assert [p.offset for p in got.parts] == offs and [p.n_samples for p in got.parts] == lens
    assert [p.n_frames for p in got.parts] == STEPS and got.n_frames == sum(STEPS)
    assert np.array_equal(_u32(got.gains), _u32(g)) and g[0] == R.fixed_gain(-6.0) and g[1] == 1.0 and g[2] == R.fixed_gain(3.0)
    assert offs[4] == offs[3] + lens[3] - 240                                 # the crossfade across the group boundary


def test_the_same_call_streamed_with_a_first_group_of_one(pkg, tiny):
    """groups of 1 + 4 + 1: the hand-overs tile the result at the documented P_g, K of each P_g the crossfade of the seam behind the group's last part,
    and the bytes are the host statement over the audio of the same groups"""
    rt = pkg.runtime
    pcm = _batches(pkg, tiny, [(0, 1), (1, 5), (5, 6)])
    trim = rt.TrimOpts(edges=1, threshold_db=_trim_db(pcm), pad_ms=5.0, max_pause_ms=20.0)
    po = _mixed_list(rt, trim)
    po[4] = rt.PartOpts(gain_db=3.0, crossfade_ms=100.0)                      # the seam behind the second group: K = 2400, more than a tile
    o = rt.JoinOpts(gap_ms=20.0)
    want, g, offs, lens = _host_statement(rt, pcm, po, o)
    hand = []
    got = tiny.generate_joined(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS], o, parts=po, pcm_callback=lambda off, x: hand.append((off, x)), first_group=1)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    assert [p.offset for p in got.parts] == offs and [p.n_samples for p in got.parts] == lens and np.array_equal(_u32(got.gains), _u32(g))
    ends = [offs[i] + lens[i] for i in (0, 4, 5)]
    p0 = rt.join_parts_stream_ready(o, po[0], ends[0])
    p1 = max(p0, rt.join_parts_stream_ready(o, po[4], ends[1]))
    assert p0 == ends[0] // SPF * SPF and p1 == (ends[1] - 2400) // SPF * SPF and p1 < rt.join_stream_ready(o, ends[1])
    assert [(off, x.size) for off, x in hand] == [(a, b - a) for a, b in ((0, p0), (p0, p1), (p1, ends[2])) if b > a]
    assert np.array_equal(_bits(np.concatenate([x for _, x in hand])), _bits(got.pcm))


def test_a_list_of_defaults_is_the_call_without_a_list(pkg, tiny):
    rt = pkg.runtime
    toks, cfgs = _toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS]
    for make in (lambda: rt.JoinOpts(), lambda: rt.JoinOpts(crossfade_ms=10.0, loudness=-2300, pcm_format=pkg.PCM_S16, sample_rate=16000)):
        rt.launch_counts(True)
        want = tiny.generate_joined(toks, cfgs, make())
        counts = rt.launch_counts(False)
        rt.launch_counts(True)
        got = tiny.generate_joined(toks, cfgs, make(), parts=[rt.PartOpts() for _ in STEPS])
        assert rt.launch_counts(False) == counts and counts.get("k_join") == 2 and "k_join_gain" not in counts, counts
        assert np.array_equal(_bits(got.pcm), _bits(want.pcm)) and got.n_frames == want.n_frames and _records(got.parts) == _records(want.parts)
        assert got.gains.tolist() == [1.0] * len(STEPS)


def test_refusals_name_the_field_and_the_part_and_launch_nothing(pkg, tiny):
    rt = pkg.runtime
    toks, cfgs = _toks(3), [_cfg(pkg, 2)] * 3
    ok = rt.PartOpts

    def refused(po, *words, join=None, **kw):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            tiny.generate_joined(toks, cfgs, join, parts=po, **kw)
        counts = rt.launch_counts(False)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (str(ei.value), counts)
        assert all(w in str(ei.value) for w in words), (words, str(ei.value))

    refused([ok(), ok(), ok(gap_ms=float("nan"))], "join: parts", "part 2", "gap_ms")
    refused([ok(), ok(crossfade_ms=2000.5), ok()], "join: parts", "part 1", "crossfade_ms")
    refused([ok(gap_ms=1.0, crossfade_ms=1.0), ok(), ok()], "part 0", "both")
    refused([ok(), ok(gain_db=24.5), ok()], "part 1", "gain_db")
    refused([ok(), ok(), ok(level=-1600, gain_db=1.0)], "part 2", "level", "gain_db")
    refused([ok(), ok(level=-50), ok()], "part 1", "level")
    refused([ok(), ok(formant=rt.FormantOpts(1)), ok()], "part 1", "formant", "pitch")
    refused([ok(), ok(), ok(pitch=rt.PitchOpts(2000), tempo=rt.TempoOpts(800))], "part 2", "800", "2000")    # the pair has no effective speed: both values
    refused([ok(), ok(pitch=rt.PitchOpts(1600), formant=rt.FormantOpts(1)), ok()], "part 1", "formant")        # the option's own range
    refused([ok(tempo=rt.TempoOpts(400)), ok(), ok()], "part 0", "speed_permille")
    refused([ok(trim=rt.TrimOpts(pad_ms=-1.0)), ok(), ok()], "part 0", "pad_ms")
    for stage in (dict(tempo=rt.TempoOpts(1100)), dict(trim=rt.TrimOpts()), dict(pitch=rt.PitchOpts(1100))):
        d = rt.DspOpts(0, 0, 0.0, 0.0)
        d._ext = rt.DspExt(**stage)
        d.ext = d._ext.h
        refused([ok(), ok(), ok()], "join: parts", next(iter(stage)), "belongs in the list", join=rt.JoinOpts(dsp=d))
    refused([ok(), ok(), ok()], "join: stream", "loudness", join=rt.JoinOpts(loudness=-2300), pcm_callback=lambda off, x: None)   # the streamed call's own, in its words
    refused([ok(), ok(), ok()], "first_group", stream=rt.JoinStreamOpts(first_group=5))
    with pytest.raises(pkg.PttsError) as ei:                                  # a list of another length never reaches the library
        tiny.generate_joined(toks, cfgs, None, parts=[ok(), ok()])
    assert "PartOpts" in str(ei.value)
    got = tiny.generate_joined(toks, cfgs, None, parts=[ok(gain_db=-6.0), ok(), ok()])   # and the model serves on
    assert got.n_frames == 6 and got.gains[0] == R.fixed_gain(-6.0)


def test_a_level_on_the_call(pkg, tiny, chunks):
    """Each part levelled to -23 LUFS on its own.  The precondition, asserted here on the host from the chunks' audio: a part of at least 5 frames
    (one whole 400 ms block) has a finite ptts_loudness and a gain other than 1.  temperature = 0 and the quiet checkpoint were kept: the check is
    this test's own assertion on the audio of the module's generate_batch call, and the tiny model's audio passes the gates as it is (observed on
    the MI355X: the parts of 5 and 6 frames measure -36.6 and -36.8 LUFS and get gains of 4.81 and 4.92, the shorter parts hold no whole block)."""
    rt = pkg.runtime
    lv = -2300
    long_parts = [i for i, s in enumerate(STEPS) if s >= 5]
    lufs = [rt.loudness(c) for c in chunks]
    print("chunk loudness:", lufs, "peaks:", [float(np.abs(c).max()) for c in chunks])
    assert long_parts and any(math.isfinite(lufs[i]) for i in long_parts), lufs
    po = [rt.PartOpts(level=lv, crossfade_ms=(10.0 if i % 2 else -1.0)) for i in range(len(STEPS))]
    want, g, offs, lens = _host_statement(rt, chunks, po, None)
    print("gains:", g.tolist())
    assert any(math.isfinite(lufs[i]) and g[i] != 1.0 for i in long_parts), (lufs, g)
    assert all(g[i] == 1.0 for i, s in enumerate(STEPS) if s < 5)             # shorter than a block: no gate passed
    rt.launch_counts(True)
    got = tiny.generate_joined(_toks(len(STEPS)), [_cfg(pkg, s) for s in STEPS], None, parts=po)
    counts = rt.launch_counts(False)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), int((_u32(got.pcm) != _u32(want)).sum())
    assert np.array_equal(_u32(got.gains), _u32(g)) and [p.offset for p in got.parts] == offs and [p.n_samples for p in got.parts] == lens
    assert not np.array_equal(_u32(want), _u32(rt.join_parts(chunks, [rt.PartOpts(crossfade_ms=p.crossfade_ms) for p in po])))
    assert counts.get("k_join_gain") == 2 and counts.get("k_loud_gate") == 2 and counts.get("k_dsp_peak") == 2 and "k_dsp_apply" not in counts, counts
