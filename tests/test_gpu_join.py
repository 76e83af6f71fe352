"""Joined synthesis on the GPU (go-pocket-tts_amd/csrc/join.hip, generate.cpp generate_joined; include/ptts.h ptts_generate_joined; DESIGN.md
section 8, N3): k_join gives ptts_join's bits for every shape and alignment; a joined call is the join of the same requests' audio from one
ptts_generate call, within a group and across groups; the chain runs once over the whole text and gives the host chain's result on the joined
audio; the egress is the egress of one row; refusals launch nothing; a cancelled chunk fails the call and is named."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import _dsp_ref as D
import _join_ref as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPF = 1920
STEPS3, STEPS6 = [2, 5, 3], [2, 5, 3, 4, 1, 6]   # six: two groups at max_batch = 4


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    path = str(tmp_path_factory.mktemp("join") / "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234))
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


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


def _joined(pkg, gm, steps, join=None):
    return gm.generate_joined(_toks(len(steps)), [_cfg(pkg, s) for s in steps], join)


def test_join_rows_is_the_host_join_bit_for_bit(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    for oi, lengths in enumerate(J.ORDERS):
        parts = J.parts_for(lengths, seed=oi)
        for mode in J.MODES:
            o = rt.JoinOpts(**mode)
            got, want = gm.join_rows(parts, o), rt.join(parts, o)
            assert got.size == want.size and np.array_equal(_u32(got), _u32(want)), (lengths, mode, int((_u32(got) != _u32(want)).sum()))
    # 300 rows of 1 .. 7 samples, a 3-sample crossfade: seams on both sides of the 256-row table boundary, one across it
    rng = np.random.default_rng(5)
    lengths = [int(v) for v in rng.integers(1, 8, 300)]
    lengths[254:258] = [7, 6, 7, 6]
    parts = J.parts_for(lengths, seed=9)
    o = rt.JoinOpts(crossfade_ms=0.13)
    assert J.samples(0.13) == 3 and J.seam(3, lengths[255], lengths[256]) == 3
    got = gm.join_rows(parts, o)
    assert np.array_equal(_u32(got), _u32(rt.join(parts, o))) and np.array_equal(_u32(got), _u32(J.join(parts, crossfade_ms=0.13)))
    # one row alone, and one empty row alone
    for n in (1, 1921, 0):
        p = J.parts_for([n], seed=2)
        for mode in (dict(), dict(gap_ms=37.5), dict(crossfade_ms=10.0)):
            assert np.array_equal(_u32(gm.join_rows(p, rt.JoinOpts(**mode))), _u32(p[0])), (n, mode)
    # destinations of every residue mod 4, with spans that begin and end inside a 16-byte group; NaN and infinity pass
    lengths = [5, 6, 7, 8, 1025, 3, 2049, 1, 1, 1, 4097]
    parts = J.parts_for(lengths, seed=4)
    parts[4][3], parts[6][2048], parts[10][0] = np.nan, np.inf, -np.inf
    _u32(parts[2])[1] = 0x7FC12345
    for mode in (dict(), dict(gap_ms=0.05), dict(gap_ms=0.13), dict(crossfade_ms=0.1)):
        offs, _ = J.offsets(lengths, **mode)
        if mode in (dict(), dict(gap_ms=0.13)):
            assert {v % 4 for v in offs} == {0, 1, 2, 3}, offs
        o = rt.JoinOpts(**mode)
        got = gm.join_rows(parts, o)
        assert np.array_equal(_u32(got), _u32(rt.join(parts, o))), mode


def test_three_chunks_are_their_concatenation(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    rt.launch_counts(True)
    got = _joined(pkg, gm, STEPS3)
    counts = rt.launch_counts(False)
    want = np.concatenate(chunks[tuple(STEPS3)])
    assert got.pcm.dtype == np.float32 and got.n_frames == 10 and np.array_equal(_u32(got.pcm), _u32(want))
    assert [p.offset for p in got.parts] == [0, 3840, 13440] and [p.n_samples for p in got.parts] == [3840, 9600, 5760]
    assert [p.n_frames for p in got.parts] == STEPS3 and all(p.status == rt.PTTS_OK and p.eos_step == -1 for p in got.parts)
    assert counts.get("k_join") == 1 and not [k for k in counts if k.startswith("k_dsp") or k == "k_resample"], counts


def test_six_chunks_in_two_groups_are_their_concatenation(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    rt.launch_counts(True)
    got = _joined(pkg, gm, STEPS6)
    counts = rt.launch_counts(False)
    want = np.concatenate(chunks[tuple(STEPS6)])
    assert got.n_frames == sum(STEPS6) and np.array_equal(_u32(got.pcm), _u32(want))
    assert [p.offset for p in got.parts] == [int(v) for v in np.cumsum([0] + STEPS6[:-1]) * SPF] and [p.n_frames for p in got.parts] == STEPS6
    assert counts.get("k_join") == 2, counts


@pytest.mark.parametrize("mode", [dict(gap_ms=37.5), dict(gap_ms=0.05), dict(crossfade_ms=10.0), dict(crossfade_ms=2000.0)], ids=lambda m: "%s=%g" % next(iter(m.items())))
def test_gap_and_crossfade_are_the_host_join_of_the_chunks(pkg, tiny, chunks, mode):
    """Six chunks: seams inside a group and the seam between the two groups, which the second group's first row fades in place."""
    _, gm = tiny
    rt = pkg.runtime
    o = rt.JoinOpts(**mode)
    got = _joined(pkg, gm, STEPS6, o)
    pcm = chunks[tuple(STEPS6)]
    want = rt.join(pcm, o)
    assert got.pcm.size == want.size and np.array_equal(_u32(got.pcm), _u32(want)), (mode, int((_u32(got.pcm) != _u32(want)).sum()))
    offs, total = J.offsets([p.size for p in pcm], **mode)
    assert [p.offset for p in got.parts] == offs and got.pcm.size == total and [p.n_samples for p in got.parts] == [p.size for p in pcm]
    assert np.array_equal(_u32(got.pcm), _u32(J.join(pcm, **mode)))


def test_the_chain_runs_once_over_the_whole_text(pkg, tiny, chunks):
    _, gm = tiny
    rt = pkg.runtime
    pcm = chunks[tuple(STEPS3)]
    whole = np.concatenate(pcm)
    peaks = [float(np.abs(p).max()) for p in pcm]
    assert min(peaks) > 0 and max(peaks) / min(peaks) > 1.0001, peaks       # the chunks' own peaks differ: per-chunk normalise is another result
    # normalise + fades: ptts_dsp_apply on the joined audio, bit for bit
    sw = dict(normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    got = _joined(pkg, gm, STEPS3, rt.JoinOpts(dsp=rt.DspOpts(1, 0, 50.0, 80.0)))
    assert np.array_equal(_u32(got.pcm), _u32(rt.dsp_apply(whole, **sw)))
    per_chunk = np.concatenate([rt.dsp_apply(p, **sw) for p in pcm])
    assert not np.array_equal(_u32(got.pcm), _u32(per_chunk))               # not the old thing
    assert abs(float(np.abs(got.pcm).max()) - 1.0) < 1e-6 and got.pcm[0] == 0.0 and got.pcm[-1] == 0.0
    assert float(np.abs(got.pcm[3840 - 100:3840 + 100]).max()) > 0.0        # no fade at a sentence boundary
    # loudness -23 LUFS: ptts_loudness_normalize on the joined audio, bit for bit
    want, measured = rt.loudness_normalize(whole, -23.0)
    print(f"the joined audio measures {measured:.2f} LUFS")
    assert np.isfinite(measured) and not np.array_equal(_u32(want), _u32(whole))   # (the gain is not 1: the comparison bites)
    got = _joined(pkg, gm, STEPS3, rt.JoinOpts(loudness=-2300))
    assert np.array_equal(_u32(got.pcm), _u32(want))
    # the limiter, through ext: ptts_limit_apply on the joined audio, bit for bit
    lim = rt.LimiterOpts(ceiling_db=-12.0, lookahead_ms=1.5, release_ms=80.0, drive_db=12.0)
    dsp = rt._dsp_opts(pkg.RuntimeGenerateConfig(limiter=lim))
    want = rt.limit_apply(lim, whole)
    assert not np.array_equal(_u32(want), _u32(whole * np.float32(10.0 ** (12.0 / 20.0))))
    got = _joined(pkg, gm, STEPS3, rt.JoinOpts(dsp=dsp))
    assert np.array_equal(_u32(got.pcm), _u32(want))
    # the DC block: ptts_dsp_apply within one f32 step at the row's peak
    want = rt.dsp_apply(whole, dc_block=True)
    got = _joined(pkg, gm, STEPS3, rt.JoinOpts(dsp=rt.DspOpts(0, 1, 0.0, 0.0)))
    err = float(np.abs(got.pcm.astype(np.float64) - want.astype(np.float64)).max())
    moved = float(np.abs(want.astype(np.float64) - whole).max())
    print(f"dc_block over the joined audio: max |gpu - host| {err:.3e}, bound {D.dc_bound(want):.3e}; the filter moves it by {moved:.3e}")
    assert err <= D.dc_bound(want) and moved > 100.0 * D.dc_bound(want)
    # ... and behind a crossfade the chain reads the crossfaded audio
    o = rt.JoinOpts(crossfade_ms=10.0, dsp=rt.DspOpts(1, 0, 5.0, 5.0))
    got = _joined(pkg, gm, STEPS3, o)
    assert np.array_equal(_u32(got.pcm), _u32(rt.dsp_apply(rt.join(pcm, rt.JoinOpts(crossfade_ms=10.0)), normalize=True, fade_in_ms=5.0, fade_out_ms=5.0)))


@pytest.mark.parametrize("rate", [0, 8000, 44100])
def test_egress_is_the_egress_of_the_joined_row(pkg, tiny, chunks, rate):
    _, gm = tiny
    rt = pkg.runtime
    joined24 = rt.join(chunks[tuple(STEPS3)], rt.JoinOpts(gap_ms=37.5))
    y = gm.resample(joined24, 24000, rate) if rate not in (0, 24000) else joined24
    for fmt, code in (("f32", pkg.PCM_F32), ("s16", pkg.PCM_S16), ("ulaw", pkg.PCM_ULAW), ("alaw", pkg.PCM_ALAW)):
        want = y if fmt == "f32" else gm.pcm_encode(y, code)
        got = _joined(pkg, gm, STEPS3, rt.JoinOpts(gap_ms=37.5, pcm_format=code, sample_rate=rate))
        assert got.pcm.dtype == want.dtype and got.pcm.size == rt.resample_length(joined24.size, 24000, rate or 24000), (fmt, rate)
        assert np.array_equal(_bits(got.pcm), _bits(want)), (fmt, rate)
        assert [p.offset for p in got.parts] == [0, 3840 + 900, 3840 + 9600 + 1800]     # parts count 24 kHz samples, whatever the egress


def _refused(pkg, gm, cfgs, join, toks=None):
    rt = pkg.runtime
    rt.launch_counts(True)
    with pytest.raises(pkg.PttsError) as ei:
        gm.generate_joined(toks or _toks(len(cfgs)), cfgs, join)
    counts = rt.launch_counts(False)
    assert ei.value.code == rt.PTTS_EINVAL and not counts, (str(ei.value), counts)
    return str(ei.value), ei.value.parts


def test_refusals_name_the_field_and_launch_nothing(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    cb = lambda off, x: None  # noqa: E731
    for kw, field in ((dict(normalize=True), "dsp"), (dict(loudness=-2300), "loudness"), (dict(sample_rate=8000), "sample_rate"), (dict(pcm16=True), "pcm_format"),
                      (dict(g711="ulaw"), "pcm_format"), (dict(pcm_callback=cb), "pcm_callback"), (dict(want_latents=True), "want_latents")):
        msg, parts = _refused(pkg, gm, [_cfg(pkg, 2), _cfg(pkg, 2, **kw), _cfg(pkg, 2)], None)
        assert f"request 1 sets {field}" in msg and "join options" in msg, (kw, msg)
        assert [p.status for p in parts] == [rt.PTTS_OK, rt.PTTS_EINVAL, rt.PTTS_OK]
    msg, _ = _refused(pkg, gm, [_cfg(pkg, 2), _cfg(pkg, 2, lsd_decode_steps=2)], None)
    assert "lsd_steps" in msg and "text order" in msg, msg
    msg, _ = _refused(pkg, gm, [_cfg(pkg, 2), _cfg(pkg, 2)], None, toks=[[3, 7], []])                  # request_error's own words
    assert "token slice must not be empty" in msg, msg
    msg, _ = _refused(pkg, gm, [_cfg(pkg, 2), _cfg(pkg, 2, temperature=float("nan"))], None)
    assert "temperature is NaN" in msg, msg
    two = [_cfg(pkg, 2), _cfg(pkg, 2)]
    for o, words in ((rt.JoinOpts(gap_ms=1.0, crossfade_ms=1.0), ("gap_ms", "crossfade_ms", "both")), (rt.JoinOpts(gap_ms=2000.5), ("gap_ms",)),
                     (rt.JoinOpts(crossfade_ms=float("nan")), ("crossfade_ms",)), (rt.JoinOpts(size=24), ("size",)), (rt.JoinOpts(pcm_format=7), ("pcm_format",)),
                     (rt.JoinOpts(sample_rate=12345), ("sample_rate", "12345")), (rt.JoinOpts(loudness=5), ("loudness",)),
                     (rt.JoinOpts(dsp=rt.DspOpts(0, 0, -1.0, 0.0)), ("dsp", "fade_in_ms")), (rt.JoinOpts(loudness=-2300, dsp=rt.DspOpts(1, 0, 0.0, 0.0)), ("loudness", "normalize"))):
        msg, _ = _refused(pkg, gm, two, o)
        assert "join" in msg and all(w in msg for w in words), (words, msg)
    # more parts than a text has
    rt.launch_counts(True)
    reqs, res, keep = (rt._Request * 4097)(), rt._Result(), []
    for r in reqs:
        gm._fill_request(r, [3, 7, 11], _cfg(pkg, 1), keep)
    rc = rt.lib().ptts_generate_joined(gm.h, reqs, 4097, C.byref(rt.JoinOpts()), C.byref(res), None)
    assert rc == rt.PTTS_EINVAL and "4096" in rt.lib().ptts_last_error().decode() and not rt.launch_counts(False)
    # the model serves on afterwards
    assert gm.generate_joined(_toks(2), two).n_frames == 4


def test_a_cancelled_chunk_fails_the_call_and_is_named(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    flag = np.ones(1, np.int32)
    for steps, at in ((STEPS3, 1), (STEPS6, 5)):
        cfgs = [_cfg(pkg, s) for s in steps]
        cfgs[at] = _cfg(pkg, steps[at], cancel=flag)
        with pytest.raises(pkg.PttsError) as ei:
            gm.generate_joined(_toks(len(steps)), cfgs)
        assert ei.value.code == rt.PTTS_ECANCELLED, str(ei.value)
        st = [p.status for p in ei.value.parts]
        assert st[at] == rt.PTTS_ECANCELLED and all(s == rt.PTTS_OK for i, s in enumerate(st) if i != at), st
        group = range(at // 4 * 4, min(len(steps), at // 4 * 4 + 4))
        assert all(ei.value.parts[i].n_frames == steps[i] for i in group if i != at)     # the chunks beside it ran; the call still fails as a whole
    assert gm.generate_joined(_toks(3), [_cfg(pkg, s) for s in STEPS3]).n_frames == 10


def test_service_synthesize_joined(pkg, tmp_path):
    blob = open(os.path.join(ROOT, "tests", "golden", "tiny_unigram.model"), "rb").read()
    tok = pkg.runtime.Tokenizer(blob)
    rt = pkg.runtime
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), n_bins=tok.vocab_size + 5)   # every piece id has an embedding row
    path = str(tmp_path / "tiny_vocab.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=99))
    gm = pkg.Model.open(path, device=0, max_batch=16)
    text = ("The quick brown fox jumps over the lazy dog while she sells sea shells by the sea shore. How much wood would a woodchuck chuck if a woodchuck "
            "could chuck wood? It was the best of times, it was the worst of times, it was the age of wisdom.")
    svc = pkg.Service(gm, tok, pkg.TTSConfig(eos_threshold=float("inf"), max_steps=3))
    plain = svc.synthesize(text)
    n_chunks = len(svc.synthesize_chunks(text))
    assert n_chunks >= 2 and plain.size == n_chunks * 3 * SPF
    got = svc.synthesize_joined(text)
    assert len(got.parts) == n_chunks and got.n_frames == 3 * n_chunks and np.array_equal(_u32(got.pcm), _u32(plain))
    got = svc.synthesize_joined(text, join=rt.JoinOpts(dsp=rt.DspOpts(1, 0, 5.0, 5.0)))
    assert np.array_equal(_u32(got.pcm), _u32(rt.dsp_apply(plain, normalize=True, fade_in_ms=5.0, fade_out_ms=5.0)))
    got = svc.synthesize_joined(text, join=rt.JoinOpts(gap_ms=100.0, pcm_format=pkg.PCM_S16))
    parts = [plain[i * 3 * SPF:(i + 1) * 3 * SPF] for i in range(n_chunks)]
    assert np.array_equal(_bits(got.pcm), _bits(gm.pcm_encode(rt.join(parts, rt.JoinOpts(gap_ms=100.0)), pkg.PCM_S16)))
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500)
    try:
        with pytest.raises(pkg.PttsError) as ei:
            pkg.Service(gm, tok, dispatcher=d).synthesize_joined(text)
        assert "dispatcher" in str(ei.value)
    finally:
        d.close()
    gm.close()
