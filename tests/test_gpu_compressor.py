"""The dynamic range compressor on the GPU (go-pocket-tts_amd/csrc/compressor.hip k_cmp_*; compressor.h):
ptts_compress_rows gives the bits of ptts_compress_apply whatever rows share the launch; a request's compressor (ptts_dsp_ext_set_compressor on
the handle of ptts_dsp_opts.ext) is ptts_compress_apply of the request's own raw audio, bit for bit, in front of the rest of the chain, which
then is the host chain of that audio; requests without a compressor launch what they launched."""
import math

import numpy as np
import pytest

import _compressor_ref as R
import _eq_ref as E
import test_gpu_dsp as TD   # the egress relations and their bounds (_check_dc, _convert), the dispatcher and raw-call helpers
import test_gpu_eq as TE    # the host statement of the chain behind the compressor
from test_gpu_loudness import tiny  # noqa: F401  (the tiny model with audible output)

pytestmark = pytest.mark.gpu

STEPS = [7, 3, 9, 6, 12, 5]
FADES = dict(fade_in_ms=50.0, fade_out_ms=80.0)
TARGET = -1600
BOOST = [(E.PEAKING, 1000.0, 18.0, 0.7)]
CMP_KERNELS = ("k_cmp_summary_p", "k_cmp_carry_p", "k_cmp_summary_s", "k_cmp_carry_s", "k_cmp_apply")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def _opts(rt, name):
    return rt.CompressorOpts(*R.DESIGNS[name])


def _for_audio(rt, pcm, **kw):
    """A compressor whose threshold lies 12 dB under the audio's own peak, inside the header's range: it engages whatever the model's level."""
    peak = float(np.abs(pcm).max())
    assert peak > 0
    kw.setdefault("attack_ms", 2.0)
    kw.setdefault("release_ms", 60.0)
    return rt.CompressorOpts(threshold_db=min(max(20.0 * math.log10(peak) - 12.0, -60.0), 0.0), ratio=4.0, knee_db=6.0, **kw)


def _bites(rt, c, pcm):
    """The compressed audio, after the assertion that the stage moved it far above one f32 step at its peak."""
    y = rt.compress_apply(c, pcm)
    moved, bound = float(np.abs(y.astype(np.float64) - pcm).max()), E.bound(pcm)
    assert moved > 1000.0 * bound, (moved, bound)
    return y


def _census(counts, prefixes=("k_cmp", "k_tp", "k_eq", "k_dsp", "k_loud")):
    return {k: v for k, v in counts.items() if k.startswith(prefixes)}


@pytest.fixture(scope="module")
def rows():
    mine = [E.signal(max(R.LENGTHS), seed=31)[:n] for n in R.LENGTHS]
    burst = R.burst(9601)
    nan = E.signal(3841, seed=4)
    nan[1930] = np.nan
    for a in mine + [burst, nan]:
        a.setflags(write=False)
    return mine, burst, nan


def test_rows_are_the_host_bits(pkg, tiny, rows):  # noqa: F811
    """Every length alone, all beside each other, and in the other order; a NaN row; the five kernels in the census."""
    _, gm = tiny
    rt = pkg.runtime
    mine, burst, nan = rows
    c = _opts(rt, "knee6")
    table = mine + [burst, nan]
    want = [rt.compress_apply(c, x) for x in table]
    assert int(np.isnan(want[-1]).sum()) == 1 and np.isnan(want[-1][1930])
    _bites(rt, c, mine[-1])
    for x, w in zip(table, want):
        got = gm.compress_rows(x, c)
        assert got.shape == w.shape and np.array_equal(_u32(got), _u32(w)), x.size
    for order in (slice(None), slice(None, None, -1)):
        rt.launch_counts(True)
        got = gm.compress_rows(table[order], c)
        assert _census(rt.launch_counts(False)) == {k: 1 for k in CMP_KERNELS}
        for g, w in zip(got, want[order]):
            assert np.array_equal(_u32(g), _u32(w)), w.size
    # rows of one tile at the most hand nothing on: no summary
    rt.launch_counts(True)
    gm.compress_rows(mine[:7], c)
    assert _census(rt.launch_counts(False)) == {"k_cmp_carry_p": 1, "k_cmp_carry_s": 1, "k_cmp_apply": 1}


def test_one_table_with_different_designs_and_a_null_row(pkg, tiny, rows):  # noqa: F811
    _, gm = tiny
    rt = pkg.runtime
    mine, burst, _ = rows
    a, b = _opts(rt, "hard"), _opts(rt, "ratio100")
    xs = [mine[8], burst, mine[7], mine[9][:30000], mine[4]]
    cs = [a, b, None, b, a]
    got = gm.compress_rows(xs, cs)
    for x, c, g in zip(xs, cs, got):
        want = x if c is None else rt.compress_apply(c, x)
        assert np.array_equal(_u32(g), _u32(want)), (x.size, c is None)
    assert not np.array_equal(_u32(rt.compress_apply(a, burst)), _u32(rt.compress_apply(b, burst)))
    with pytest.raises(pkg.PttsError) as ei:
        gm.compress_rows([mine[3], mine[3]], [a, rt.CompressorOpts(knee_db=-1.0)])
    assert ei.value.code == rt.PTTS_EINVAL and "knee_db" in str(ei.value) and "row 1" in str(ei.value)


@pytest.fixture(scope="module")
def base(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    return gm.generate_batch(_toks(len(STEPS)), [TD._cfg(pkg, s) for s in STEPS])


def test_generated_requests_are_the_host_statement(pkg, tiny, base):  # noqa: F811
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4): the compressor alone, then in front of loudness, DC block, a
    boosting equaliser, the fades and the ceiling."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    cs = [_for_audio(rt, b.pcm, makeup_db=3.0 if i % 2 else 0.0) for i, b in enumerate(base)]
    comp = [_bites(rt, c, b.pcm) for c, b in zip(cs, base)]
    # the compressor alone: ptts_compress_apply's bits, through the keyword and through a handle of the caller's
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, compressor=c) for s, c in zip(STEPS, cs)])
    for b, g, w in zip(base, got, comp):
        assert g.n_frames == b.n_frames and np.array_equal(_u32(g.pcm), _u32(w)), b.n_frames
    exts = [rt.DspExt(compressor=c) for c in cs]

    def handle(i):
        o = rt.DspOpts()
        o.ext = exts[i].h
        return o
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, dsp_opts=handle(i)) for i, s in enumerate(STEPS)])
    for g, w in zip(got, comp):
        assert np.array_equal(_u32(g.pcm), _u32(w))
    for e in exts:
        e.free()
    # a neighbour without a compressor in the same batch keeps its plain bits
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, compressor=c if i % 2 else None) for i, (s, c) in enumerate(zip(STEPS, cs))])
    for i, (b, m, w) in enumerate(zip(base, mixed, comp)):
        assert np.array_equal(_u32(m.pcm), _u32(w if i % 2 else b.pcm)), i
    # in front of loudness, a boosting equaliser, the fades and the ceiling: the host chain of the compressed audio, bit for bit, also at 8 kHz mu-law
    boost = rt.Eq(BOOST)
    pre = [TE._statement(pkg, y, boost, loudness=TARGET, **FADES) for y in comp]
    ceil = [min(max(20.0 * math.log10(float(rt.true_peak(p))) - 6.0, -60.0), 0.0) for p in pre]
    want24 = [rt.true_peak_limit(p, c)[0] for p, c in zip(pre, ceil)]
    plain24 = [rt.true_peak_limit(TE._statement(pkg, b.pcm, boost, loudness=TARGET, **FADES), c)[0] for b, c in zip(base, ceil)]
    assert all(not np.array_equal(_u32(w), _u32(p)) for w, p in zip(want24, plain24))      # the compressor is heard behind the loudness gain too
    for fmt, rate in (("f32", 0), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET, eq=boost, true_peak_dbtp=t, compressor=c, **FADES)
                                       for s, c, t in zip(STEPS, cs, ceil)])
        for b, g, w in zip(base, got, want24):
            want = TD._convert(pkg, gm, w, fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
    # ... and with the DC block: within the DC block's bounds (TD._check_dc's relations)
    pre = [TE._statement(pkg, y, boost, loudness=TARGET, dc_block=True, **FADES) for y in comp]
    host = [rt.true_peak_limit(p, c)[0] for p, c in zip(pre, ceil)]
    for fmt, rate in (("f32", 0), ("ulaw", 8000)):
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET, dc_block=True, eq=boost, true_peak_dbtp=t, compressor=c, **FADES)
                                       for s, c, t in zip(STEPS, cs, ceil)])
        for b, g, h in zip(base, got, host):
            TD._check_dc(pkg, gm, g.pcm, h, fmt, rate, f"generate compressor+loudness+dc+eq+fades+ceiling {fmt} {rate or 24000} Hz frames={b.n_frames}")
    boost.free()


def test_continuous_dispatcher_gives_the_one_shot_bits(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    boost = rt.Eq(BOOST)
    steps = [7, 6, 9, 5]
    toks = _toks(len(steps))
    own = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s) for s in steps], True)
    cs = [_for_audio(rt, o.pcm) for o in own]
    specs = [(7, "f32", 0, dict(compressor=cs[0])), (6, "ulaw", 8000, dict(compressor=cs[1], loudness=TARGET, eq=boost, fade_out_ms=80.0)), (9, "f32", 0, None),
             (5, "s16", 16000, dict(compressor=cs[3], normalize=True, fade_in_ms=50.0))]
    got = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs], True)
    shot = gm.generate_batch(toks, [TD._cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs])
    y = [_bites(rt, c, o.pcm) for c, o in zip(cs, own)]
    host = [y[0], TE._statement(pkg, y[1], boost, loudness=TARGET, fade_out_ms=80.0), own[2].pcm, rt.dsp_apply(y[3], normalize=True, fade_in_ms=50.0)]
    for i, (s, f, r, sw) in enumerate(specs):
        assert got[i].n_frames == s
        assert np.array_equal(TD._bits(got[i].pcm), TD._bits(shot[i].pcm)), (i, f, r)
        assert np.array_equal(TD._bits(got[i].pcm), TD._bits(TD._convert(pkg, gm, host[i], f, r))), (i, f, r)
    boost.free()


def test_requests_without_a_compressor_launch_what_they_launched(pkg, tiny, base):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    sw = dict(normalize=True, fade_in_ms=50.0, fade_out_ms=80.0)
    rt.launch_counts(True)
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, **sw) for s in STEPS])
    counts = rt.launch_counts(False)
    assert not _census(counts, ("k_cmp",)) and _census(counts, ("k_dsp",)), counts
    want = gm.dsp_rows([b.pcm for b in base], **sw)                       # the parent's statement of such a request
    for g, w in zip(got, want):
        assert np.array_equal(_u32(g.pcm), _u32(w))
    quiet = rt.DspExt(compressor=rt.CompressorOpts())                     # a live handle that switches nothing on: set, then cleared
    quiet.set_compressor(None)
    o = rt.DspOpts()
    o.ext = quiet.h
    rt.launch_counts(True)
    got = gm.generate_batch(toks[:2], [TD._cfg(pkg, s, dsp_opts=o) for s in STEPS[:2]])
    assert _census(rt.launch_counts(False)) == {}
    for g, b in zip(got, gm.generate_batch(toks[:2], [TD._cfg(pkg, s) for s in STEPS[:2]])):   # (a batch of two: the decoder's bits are the batch shape's)
        assert np.array_equal(_u32(g.pcm), _u32(b.pcm))
    # with one: the five kernels once for the decoded group, in front of the table's other kernels; alone, nothing else
    c = _for_audio(rt, base[0].pcm)
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, compressor=c), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == {k: 1 for k in CMP_KERNELS}
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [TD._cfg(pkg, 6, compressor=c, normalize=True), TD._cfg(pkg, 6)])
    assert _census(rt.launch_counts(False)) == dict({k: 1 for k in CMP_KERNELS}, k_dsp_peak=1, k_dsp_apply=1)
    quiet.free()


def test_refusals_name_the_field_and_the_others_run(pkg, tiny):  # noqa: F811
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm
    cb = lambda off, x: None  # noqa: E731
    c = rt.CompressorOpts()
    # streaming: refused like every other switch of ext
    rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, compressor=c, pcm_callback=cb), TD._cfg(pkg, 4)])
    assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and "ext" in msg and "pcm_callback" in msg, (rc, msg)
    assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32))
    # a handle freed between admission and delivery: PTTS_EINVAL where the row is resolved, nothing launched
    ext = rt.DspExt(compressor=c)
    o = rt.DspOpts()
    o.ext = ext.h
    assert rt.dsp_opts_error(o) == ""

    def free_it(step, max_steps):
        ext.free()
    rt.launch_counts(True)
    rc, msg, out = TD._raw_generate(pkg, gm, toks[:1], [TD._cfg(pkg, 4, dsp_opts=o, step_callback=free_it)])
    counts = rt.launch_counts(False)
    assert rc == rt.PTTS_EINVAL and "dsp: ext" in msg and "live handle" in msg, (rc, msg)
    assert _census(counts) == {}, counts
    # a handle that was never live, and the model still serves
    rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 4, dsp_opts=o), TD._cfg(pkg, 4)])
    assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and "dsp: ext" in msg
    assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32))
    assert np.array_equal(_u32(gm.generate_batch([toks[1]], [TD._cfg(pkg, 4)])[0].pcm), _u32(good))


@pytest.fixture(scope="module")
def direct(pkg, tmp_path_factory):
    """A model whose decoder stores straight into the results (test_gpu_model's sea64 in bf16: the full-width SEANet ladder, whose last residual
    block runs fused with the final conv), as the production model does.  The tiny fixture above never takes that path."""
    import dataclasses
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), n_filters=64)
    path = str(tmp_path_factory.mktemp("cmp") / "sea64_bf16.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=77), dtype="BF16")
    gm = pkg.Model.open(path, device=0, weights=1)
    yield gm
    gm.close()


def test_direct_storing_model(pkg, direct):
    """Where plain requests are stored by the decoder's last kernel: a compressor request still is ptts_compress_apply of its own audio, its
    plain neighbour keeps its bits, and an ext freed between admission and delivery is refused there too -- the decision for the direct store
    does not ask whether the handle is live."""
    gm = direct
    rt = pkg.runtime
    toks = [[10, 20, 30], [5, 6, 7]]
    steps = [3, 2]
    rt.launch_counts(True)
    base = gm.generate_batch(toks, [TD._cfg(pkg, s) for s in steps])
    counts = rt.launch_counts(False)
    assert counts.get("k_resblock+final", 0) >= 1 and not _census(counts) and "k_resample" not in counts, counts   # the fused final block, no egress launch
    c = _for_audio(rt, base[0].pcm)
    want = _bites(rt, c, base[0].pcm)
    got = gm.generate_batch(toks, [TD._cfg(pkg, steps[0], compressor=c), TD._cfg(pkg, steps[1])])
    assert np.array_equal(_u32(got[0].pcm), _u32(want)) and np.array_equal(_u32(got[1].pcm), _u32(base[1].pcm))
    for kw in (dict(compressor=c), dict(true_peak_dbtp=-1.0)):           # the compressor, and the switch ext had before it
        ext = rt.DspExt(**kw)
        o = rt.DspOpts()
        o.ext = ext.h
        rt.launch_counts(True)
        rc, msg, out = TD._raw_generate(pkg, gm, toks[:1], [TD._cfg(pkg, steps[0], dsp_opts=o, step_callback=lambda s, m, e=ext: e.free())])
        counts = rt.launch_counts(False)
        assert rc == rt.PTTS_EINVAL and "dsp: ext" in msg and "live handle" in msg, (kw, rc, msg)
        assert _census(counts) == {}, counts
    assert np.array_equal(_u32(gm.generate_batch(toks, [TD._cfg(pkg, s) for s in steps])[0].pcm), _u32(base[0].pcm))
