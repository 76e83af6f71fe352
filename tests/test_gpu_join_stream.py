"""Streamed joined synthesis on the GPU (generate.cpp generate_joined, JoinStream; include/ptts.h ptts_generate_joined_streamed; DESIGN.md section 8,
N3): a joined call that hands its audio over group by group gives the bytes of the call that does not, for every chain it may carry, every join
and every egress; the hand-overs tile the result in order and their boundaries are the documented P_g; a smaller first group is the host
statement on the chunks of the same groups; without a callback the call launches what ptts_generate_joined launches; what needs the whole text
is refused by name with nothing launched; a cancelled chunk fails the call, and what was handed over before is the true beginning of the text."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import _chain_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPF = 1920
STEPS6 = [2, 5, 3, 4, 1, 6]               # two groups at max_batch = 4
STEPS9 = [3, 2, 1, 2, 4, 1, 3, 2, 1]      # first_group = 1: groups of 1 + 4 + 4
EQ2 = [(2, 300.0, 0.0, 0.707), (5, 1000.0, 4.0, 1.0)]


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    path = str(tmp_path_factory.mktemp("join_stream") / "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(synth.SynthConfig.tiny(), seed=1234))
    gm = pkg.Model.open(path, device=0, max_batch=4)
    yield gm
    gm.close()


def _cfg(pkg, steps, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, **kw)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _chain(pkg, **kw):
    kw.setdefault("compressor", pkg.runtime.CompressorOpts(threshold_db=-30.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0))
    return R.Chain(pkg, dc_block=True, eq=EQ2, fade_in_ms=50.0, fade_out_ms=80.0, **kw)


def _plain(pkg, gm, steps, join=None):
    return gm.generate_joined(_toks(len(steps)), [_cfg(pkg, s) for s in steps], join)


def _streamed(pkg, gm, steps, join=None, first_group=0, cfgs=None):
    """The streamed call: (result, hand-overs as (offset, samples) in the order they came)."""
    got = []
    res = gm.generate_joined(_toks(len(steps)), cfgs or [_cfg(pkg, s) for s in steps], join, pcm_callback=lambda off, x: got.append((off, x)), first_group=first_group)
    return res, got


def _tiles(hand, pcm):
    """The hand-overs tile the result in order, each sample once, and their concatenation is the result."""
    at = 0
    for off, x in hand:
        assert off == at and x.size > 0 and x.dtype == pcm.dtype, (off, at, x.size)
        at += x.size
    assert at == pcm.size
    assert np.array_equal(_bits(np.concatenate([x for _, x in hand])), _bits(pcm))


def _group_ends(parts, sizes):
    """A_g: the joined length behind each group."""
    out, at = [], 0
    for n in sizes:
        at += n
        out.append(parts[at - 1].offset + parts[at - 1].n_samples)
    return out


def _same_parts(a, b):
    return [(p.offset, p.n_samples, p.n_frames, p.eos_step, p.status) for p in a] == [(p.offset, p.n_samples, p.n_frames, p.eos_step, p.status) for p in b]


def _joins(pkg):
    rt = pkg.runtime
    chain = _chain(pkg)
    parts_dsp = rt.DspOpts(0, 1, 50.0, 80.0)
    parts_dsp._ext = rt.DspExt(trim=rt.TrimOpts(edges=1, threshold_db=-20.0, pad_ms=5.0), tempo=rt.TempoOpts(1100))
    parts_dsp.ext = parts_dsp._ext.h
    return {
        "plain": lambda: rt.JoinOpts(),
        "chain": lambda: rt.JoinOpts(dsp=chain.opts),
        "gap": lambda: rt.JoinOpts(gap_ms=37.5, dsp=chain.opts),
        "crossfade": lambda: rt.JoinOpts(crossfade_ms=10.0, dsp=chain.opts),
        "trim_tempo": lambda: rt.JoinOpts(crossfade_ms=10.0, dsp=parts_dsp),
    }


@pytest.mark.parametrize("name", ["plain", "chain", "gap", "crossfade", "trim_tempo"])
def test_the_streamed_call_gives_the_bytes_of_the_call_that_is_not(pkg, tiny, name):
    rt = pkg.runtime
    make = _joins(pkg)[name]
    want = _plain(pkg, tiny, STEPS6, make())
    o = make()
    got, hand = _streamed(pkg, tiny, STEPS6, o)
    assert got.pcm.dtype == np.float32 and got.n_frames == want.n_frames == sum(STEPS6) and _same_parts(got.parts, want.parts)
    assert got.pcm.size == want.pcm.size and np.array_equal(_bits(got.pcm), _bits(want.pcm)), (name, int((_bits(got.pcm) != _bits(want.pcm)).sum()))
    _tiles(hand, got.pcm)
    # f32 at 24 kHz: the boundaries are the P_g of the documented formula, from the parts' records
    a0, a1 = _group_ends(got.parts, [4, 2])
    p0 = rt.join_stream_ready(o, a0)
    assert a1 == got.pcm.size and 0 < p0 <= a0 and p0 % SPF == 0
    assert [(off, x.size) for off, x in hand] == [(0, p0), (p0, a1 - p0)], (name, [(off, x.size) for off, x in hand], p0, a0, a1)
    if name == "trim_tempo":
        assert any(p.n_samples % SPF for p in got.parts)                      # the parts' lengths left the frame grid
    if name in ("chain", "gap", "crossfade"):
        assert p0 <= a0 - SPF                                                 # the fade out's 1920 samples were held back


EGRESS = [("s16", 0, False), ("s16", 0, True), ("ulaw", 0, True), ("alaw", 0, False), ("f32", 8000, True), ("ulaw", 8000, True), ("f32", 44100, True),
          ("ulaw", 44100, False)]


@pytest.mark.parametrize("fmt,rate,chained", EGRESS, ids=["%s-%d-%s" % (f, r, "chain" if c else "plain") for f, r, c in EGRESS])
def test_every_egress_is_handed_over_in_order(pkg, tiny, fmt, rate, chained):
    rt = pkg.runtime
    code = {"f32": pkg.PCM_F32, "s16": pkg.PCM_S16, "ulaw": pkg.PCM_ULAW, "alaw": pkg.PCM_ALAW}[fmt]
    chain = _chain(pkg) if chained else None
    make = lambda: rt.JoinOpts(gap_ms=37.5, pcm_format=code, sample_rate=rate, dsp=chain.opts if chain else None)  # noqa: E731
    want = _plain(pkg, tiny, STEPS6, make())
    got, hand = _streamed(pkg, tiny, STEPS6, make())
    assert got.pcm.dtype == want.pcm.dtype and got.pcm.size == want.pcm.size == rt.resample_length(_group_ends(got.parts, [4, 2])[1], 24000, rate or 24000)
    assert np.array_equal(_bits(got.pcm), _bits(want.pcm)), (fmt, rate, chained, int((_bits(got.pcm) != _bits(want.pcm)).sum()))
    assert len(hand) > 1
    _tiles(hand, got.pcm)
    if not rate:                                                              # at 24 kHz the outputs are the samples
        assert hand[0][1].size == rt.join_stream_ready(make(), _group_ends(got.parts, [4, 2])[0])
    else:                                                                     # the filter's support holds some more back
        assert hand[0][1].size < rt.resample_length(rt.join_stream_ready(make(), _group_ends(got.parts, [4, 2])[0]), 24000, rate)


@pytest.fixture(scope="module")
def chunks9(pkg, tiny):
    """The nine chunks' own audio from three generate_batch calls over the groups 1 + 4 + 4: computed once, never written to."""
    toks, out = _toks(9), []
    for a, b in ((0, 1), (1, 5), (5, 9)):
        for r in tiny.generate_batch(toks[a:b], [_cfg(pkg, s) for s in STEPS9[a:b]]):
            p = np.array(r.pcm, np.float32)
            p.setflags(write=False)
            out.append(p)
    assert [p.size for p in out] == [s * SPF for s in STEPS9]
    return out


@pytest.mark.parametrize("mode", [dict(), dict(crossfade_ms=10.0)], ids=["plain", "crossfade"])
def test_a_first_group_of_one_is_the_host_statement(pkg, tiny, chunks9, mode):
    rt = pkg.runtime
    chain = _chain(pkg)
    o = rt.JoinOpts(dsp=chain.opts, **mode)
    got, hand = _streamed(pkg, tiny, STEPS9, o, first_group=1)
    want = chain.host(rt.join(chunks9, rt.JoinOpts(**mode)))
    assert got.pcm.size == want.size and np.array_equal(_bits(got.pcm), _bits(want)), int((_bits(got.pcm) != _bits(want)).sum())
    assert not np.array_equal(_bits(want), _bits(rt.join(chunks9, rt.JoinOpts(**mode))))
    _tiles(hand, got.pcm)
    ends = _group_ends(got.parts, [1, 4, 4])
    assert ends[0] == STEPS9[0] * SPF
    p = [rt.join_stream_ready(o, a) for a in ends[:2]]
    assert p[0] == (STEPS9[0] - 1) * SPF                                      # 80 ms of fade out (the seam's 240 samples inside them) held back: one tile
    assert [(off, x.size) for off, x in hand] == [(0, p[0]), (p[0], p[1] - p[0]), (p[1], ends[2] - p[1])]
    # without a callback the smaller first group gives the same result, all at once
    quiet = tiny.generate_joined(_toks(9), [_cfg(pkg, s) for s in STEPS9], o, first_group=1)
    assert np.array_equal(_bits(quiet.pcm), _bits(want)) and _same_parts(quiet.parts, got.parts)


def test_nothing_is_handed_over_inside_a_fade_in_that_may_still_be_clamped(pkg, tiny, chunks9):
    """The fade in is clamped by the final length, which a group that is not the last does not know: with a first part of 3 frames (5760 samples)
    and a fade in of 250 ms (6000 samples) the first group hands nothing over, and the second group's hand-over begins at 0."""
    rt = pkg.runtime
    chain = R.Chain(pkg, dc_block=True, fade_in_ms=250.0)
    o = rt.JoinOpts(dsp=chain.opts)
    got, hand = _streamed(pkg, tiny, STEPS9, o, first_group=1)
    want = chain.host(np.concatenate(chunks9))
    assert np.array_equal(_bits(got.pcm), _bits(want))
    _tiles(hand, got.pcm)
    ends = _group_ends(got.parts, [1, 4, 4])
    assert [(off, x.size) for off, x in hand] == [(0, ends[1]), (ends[1], ends[2] - ends[1])]


def test_without_a_callback_it_is_the_joined_call(pkg, tiny):
    rt = pkg.runtime
    chain = _chain(pkg)
    for make in (lambda: rt.JoinOpts(), lambda: rt.JoinOpts(gap_ms=37.5, dsp=chain.opts, pcm_format=pkg.PCM_ULAW, sample_rate=8000)):
        rt.launch_counts(True)
        want = _plain(pkg, tiny, STEPS6, make())
        counts = rt.launch_counts(False)
        rt.launch_counts(True)
        got = tiny.generate_joined(_toks(6), [_cfg(pkg, s) for s in STEPS6], make(), stream=rt.JoinStreamOpts())
        assert rt.launch_counts(False) == counts and counts.get("k_join") == 2, counts
        assert np.array_equal(_bits(got.pcm), _bits(want.pcm)) and got.n_frames == want.n_frames and _same_parts(got.parts, want.parts)


def test_refusals_name_the_field_and_launch_nothing(pkg, tiny):
    rt = pkg.runtime
    cb = lambda off, x: None  # noqa: E731
    cfgs = [_cfg(pkg, 2), _cfg(pkg, 2)]

    def refused(join, **kw):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            tiny.generate_joined(_toks(2), cfgs, join, **kw)
        counts = rt.launch_counts(False)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (str(ei.value), counts)
        assert [(p.offset, p.n_samples, p.n_frames, p.eos_step, p.status) for p in ei.value.parts] == [(0, 0, 0, -1, rt.PTTS_OK)] * 2
        return str(ei.value)

    lim = rt.LimiterOpts(ceiling_db=-12.0, lookahead_ms=1.5, release_ms=80.0, drive_db=12.0)
    for join, word in ((rt.JoinOpts(dsp=rt.DspOpts(1, 0, 0.0, 0.0)), "normalize"), (rt.JoinOpts(loudness=-2300), "loudness"),
                       (rt.JoinOpts(dsp=rt._dsp_opts(pkg.RuntimeGenerateConfig(limiter=lim))), "limiter"),
                       (rt.JoinOpts(dsp=rt._dsp_opts(pkg.RuntimeGenerateConfig(true_peak_dbtp=-1.0))), "true_peak")):
        msg = refused(join, pcm_callback=cb)
        assert "join: stream" in msg and word in msg and "pcm_callback" in msg, (word, msg)
        assert tiny.generate_joined(_toks(2), cfgs, join, first_group=1).n_frames == 4      # without a callback nothing of it is refused
    for fg in (-1, 5):
        msg = refused(rt.JoinOpts(), stream=rt.JoinStreamOpts(first_group=fg))
        assert "first_group" in msg, (fg, msg)
    assert tiny.generate_joined(_toks(2), cfgs, rt.JoinOpts(), first_group=4).n_frames == 4


def test_a_cancelled_chunk_fails_the_call_behind_a_true_beginning(pkg, tiny):
    rt = pkg.runtime
    chain = _chain(pkg)
    make = lambda: rt.JoinOpts(gap_ms=37.5, dsp=chain.opts)  # noqa: E731
    good, good_hand = _streamed(pkg, tiny, STEPS6, make())
    p0 = good_hand[0][1].size
    flag = np.zeros(1, np.int32)

    def raise_it(step, max_steps):
        flag[0] = 1

    cfgs = [_cfg(pkg, s) for s in STEPS6]
    cfgs[5] = _cfg(pkg, STEPS6[5], cancel=flag, step_callback=raise_it)         # a part of the second group
    hand = []
    n = len(STEPS6)
    reqs, parts, res, keep = (rt._Request * n)(), (rt.JoinPart * n)(), rt._Result(), []
    for i in range(n):
        tiny._fill_request(reqs[i], _toks(n)[i], cfgs[i], keep)
    o = make()
    cb = rt._PCM_CB(lambda _u, off, cnt, ptr: hand.append((int(off), np.frombuffer(C.string_at(ptr, int(cnt) * 4), dtype=np.float32))))
    so = rt.JoinStreamOpts(0, cb)
    rc = rt.lib().ptts_generate_joined_streamed(tiny.h, reqs, n, C.byref(o), C.byref(so), C.byref(res), parts)
    assert rc == rt.PTTS_ECANCELLED, rt.lib().ptts_last_error().decode()
    assert not res.pcm and not res.pcm16 and not res.pcm8 and res.n_samples == 0 and res.n_frames == 0 and res.status == rt.PTTS_ECANCELLED
    st = [p.status for p in parts]
    assert st[5] == rt.PTTS_ECANCELLED and all(s == rt.PTTS_OK for s in st[:5]), st
    assert [(off, x.size) for off, x in hand] == [(0, p0)] and np.array_equal(_bits(hand[0][1]), _bits(good.pcm[:p0]))
    assert np.array_equal(_bits(_streamed(pkg, tiny, STEPS6, make())[0].pcm), _bits(good.pcm))   # the model serves on


def test_service_synthesize_joined_streams(pkg, tmp_path):
    blob = open(os.path.join(ROOT, "tests", "golden", "tiny_unigram.model"), "rb").read()
    tok = pkg.runtime.Tokenizer(blob)
    rt = pkg.runtime
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), n_bins=tok.vocab_size + 5)   # every piece id has an embedding row
    path = str(tmp_path / "tiny_vocab.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=99))
    gm = pkg.Model.open(path, device=0, max_batch=1)             # a group per chunk
    text = ("The quick brown fox jumps over the lazy dog while she sells sea shells by the sea shore. How much wood would a woodchuck chuck if a woodchuck "
            "could chuck wood? It was the best of times, it was the worst of times, it was the age of wisdom.")
    svc = pkg.Service(gm, tok, pkg.TTSConfig(eos_threshold=float("inf"), max_steps=3))
    assert len(svc.synthesize_chunks(text)) >= 2
    chain = R.Chain(pkg, dc_block=True, eq=EQ2, fade_in_ms=50.0, fade_out_ms=80.0)
    make = lambda: rt.JoinOpts(gap_ms=100.0, pcm_format=pkg.PCM_S16, dsp=chain.opts)  # noqa: E731
    want = svc.synthesize_joined(text, join=make())
    hand = []
    got = svc.synthesize_joined(text, join=make(), pcm_callback=lambda off, x: hand.append((off, x)))
    assert got.pcm.dtype == np.int16 and np.array_equal(_bits(got.pcm), _bits(want.pcm)) and len(hand) > 1
    _tiles(hand, got.pcm)
    gm.close()
