"""Output at 8-48 kHz and G.711 on the GPU, voice clips at any rate (k_resample, go-pocket-tts_amd/csrc/resample.hip).
What must hold: ptts_resample is the float64 checker's filter (tests/_resample_ref.py) to f32 rounding and the same bits however rows are batched;
a generated request at rate R / format F is exactly ptts_resample + ptts_pcm_encode of the same request's 24 kHz f32 audio, one-shot, ragged,
streamed or continuous; clips at other rates clone exactly as their device-resampled 24 kHz samples do."""
import dataclasses
import threading

import numpy as np
import pytest

import _resample_ref as R

pytestmark = pytest.mark.gpu

OUT_RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]
IN_RATES = [8000, 16000, 44100, 48000, 96000]
FORMATS = ["f32", "s16", "ulaw", "alaw"]


def _ckpt(pkg, tmp_path_factory, **kw):
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), **kw)
    path = str(tmp_path_factory.mktemp("rs") / "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234))
    return cfg, path


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    cfg, path = _ckpt(pkg, tmp_path_factory, speaker_proj=True, encoder=True)
    gm = pkg.Model.open(path, device=0, max_batch=16)
    yield cfg, gm
    gm.close()


def _cfg(pkg, steps, fmt="f32", rate=0, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, pcm16=fmt == "s16", g711=fmt if fmt in ("ulaw", "alaw") else "",
                                     sample_rate=rate, **kw)


def _convert(pkg, gm, pcm24, fmt, rate):   # the specification of egress: ptts_resample, then the device format conversion at that rate
    y = gm.resample(pcm24, 24000, rate) if rate not in (0, 24000) else pcm24
    return y if fmt == "f32" else gm.pcm_encode(y, {"s16": pkg.PCM_S16, "ulaw": pkg.PCM_ULAW, "alaw": pkg.PCM_ALAW}[fmt])


@pytest.mark.parametrize("rin,rout", [(24000, r) for r in OUT_RATES] + [(r, 24000) for r in IN_RATES])
def test_resample_matches_the_checker_and_batching_changes_no_bit(tiny, rin, rout):
    _, gm = tiny
    rng = np.random.default_rng(rin + rout)
    lens = [1, 1919, 1920, 1921, 10 * rin]
    rows = []
    for n in lens:
        t = np.arange(n) / rin
        rows.append((0.4 * np.sin(2 * np.pi * 0.3 * min(rin, rout) / 2 * t) + 0.2 * rng.standard_normal(n)).astype(np.float32))
    batched = gm.resample(rows, rin, rout)
    for x, y in zip(rows, batched):
        assert y.size == R.length(x.size, rin, rout)
        want = R.resample(x, rin, rout)
        assert np.abs(y - want).max() <= 3e-5 * np.abs(x).max(), np.abs(y - want).max()
        alone = gm.resample(x, rin, rout)
        assert np.array_equal(alone.view(np.uint32), y.view(np.uint32))


def test_pcm_encode_is_g711_of_pcm16_for_every_code(pkg, tiny):
    _, gm = tiny
    v = np.arange(-32768, 32768, dtype=np.int64)
    x = ((v + np.where(v >= 0, 0.5, -0.5)) / 32767.0).astype(np.float32)   # mid-step samples (and past +-1)
    s16 = R.pcm16(x)
    assert len(np.unique(s16)) == 65535                                     # every code WritePCM16Samples makes (-32767..32767)
    assert np.array_equal(gm.pcm_encode(x, pkg.PCM_ULAW), R.ulaw_encode(s16))
    assert np.array_equal(gm.pcm_encode(x, pkg.PCM_ALAW), R.alaw_encode(s16))
    assert np.array_equal(gm.pcm_encode(x, pkg.PCM_S16), pkg.runtime.op_pcm16(x))
    assert np.array_equal(gm.pcm_encode(x, pkg.PCM_F32).view(np.uint32), x.view(np.uint32))


def _noise(cfg, steps, seed):
    return np.random.default_rng(seed).standard_normal((steps, cfg.ldim)).astype(np.float32) * 0.8


@pytest.mark.parametrize("rate", OUT_RATES + [24000])
def test_generation_at_a_rate_and_format_is_the_conversion_of_the_24k_audio(pkg, tiny, rate):
    cfg, gm = tiny
    toks, steps = [5, 9, 13, 2], 7
    nz = _noise(cfg, steps, rate)
    base = gm.generate_batch([toks], [_cfg(pkg, steps, noise=nz, temperature=0.64)])[0].pcm
    for fmt in FORMATS:
        got = gm.generate_batch([toks], [_cfg(pkg, steps, fmt, rate, noise=nz, temperature=0.64)])[0]
        assert got.pcm.size == got.n_frames * 8 * rate // 100
        want = _convert(pkg, gm, base, fmt, rate)
        assert got.pcm.dtype == want.dtype and np.array_equal(got.pcm.view(np.uint8), want.view(np.uint8)), (fmt, rate)
    z = gm.generate_batch([toks], [_cfg(pkg, steps, "s16", 0, noise=nz, temperature=0.64)])[0].pcm
    w = gm.generate_batch([toks], [_cfg(pkg, steps, "s16", 24000, noise=nz, temperature=0.64)])[0].pcm
    assert np.array_equal(z, w)


def test_ragged_batch_rows_are_the_conversion_of_their_own_audio_and_one_launch_per_group(pkg, tiny):
    """Utterances ending at different steps: each converted row is the conversion of that row's 24 kHz audio in the same batch shape (zeros,
    not the padded frames of the longer rows, lie past its end), and the group takes one k_resample launch; a native group none."""
    cfg, gm = tiny
    specs = [(3, "ulaw", 8000), (9, "f32", 48000), (5, "s16", 16000), (12, "alaw", 44100), (6, "f32", 0), (4, "s16", 0), (8, "f32", 22050)]
    toks = [[3 + i, 7, 11 + i] for i in range(len(specs))]
    noise = [_noise(cfg, s, i) for i, (s, _, _) in enumerate(specs)]
    native = gm.generate_batch(toks, [_cfg(pkg, s, noise=noise[i], temperature=0.64) for i, (s, _, _) in enumerate(specs)])
    rt = pkg.runtime
    rt.launch_counts(True)
    got = gm.generate_batch(toks, [_cfg(pkg, s, f, r, noise=noise[i], temperature=0.64) for i, (s, f, r) in enumerate(specs)])
    counts = rt.launch_counts(False)
    assert counts.get("k_resample", 0) == 1, counts
    for i, (s, f, r) in enumerate(specs):
        assert got[i].n_frames == native[i].n_frames == s
        want = _convert(pkg, gm, native[i].pcm, f, r)
        assert np.array_equal(got[i].pcm.view(np.uint8), want.view(np.uint8)), specs[i]
    rt.launch_counts(True)
    gm.generate_batch(toks[4:6], [_cfg(pkg, s, f, r) for s, f, r in specs[4:6]])   # a native group: no k_resample
    counts = rt.launch_counts(False)
    assert counts.get("k_resample", 0) == 0, counts


@pytest.mark.parametrize("rate", [8000, 16000, 44100, 48000])
@pytest.mark.parametrize("stream_frames", [1, 5, 12])
def test_streamed_hand_overs_concatenate_to_the_one_shot_conversion(pkg, tiny, rate, stream_frames):
    """Row 0 streams the 24 kHz f32 audio, row 1 the same request at `rate` in each format, row 2 a shorter utterance: offsets are consecutive
    output samples, each once; the concatenation is the result buffer and the one-shot conversion of row 0's audio, bit for bit."""
    cfg, gm = tiny
    steps = [11, 11, 6]
    toks = [[4, 8, 15], [4, 8, 15], [16, 23, 42]]
    noise = [_noise(cfg, 11, 50), _noise(cfg, 11, 50), _noise(cfg, 6, 51)]
    for fmt in FORMATS:
        got = [[] for _ in toks]
        cfgs = [_cfg(pkg, steps[i], "f32" if i == 0 else fmt, 0 if i == 0 else rate, noise=noise[i], temperature=0.64, stream_frames=stream_frames,
                     pcm_callback=lambda off, x, i=i: got[i].append((off, x.copy()))) for i in range(3)]
        res = gm.generate_batch(toks, cfgs)
        for i in range(3):
            offs = [o for o, _ in got[i]]
            sizes = [x.size for _, x in got[i]]
            assert offs == [int(v) for v in np.cumsum([0] + sizes[:-1])], (offs, sizes)
            assert all(sz > 0 for sz in sizes)
            cat = np.concatenate([x for _, x in got[i]])
            assert np.array_equal(cat.view(np.uint8), res[i].pcm.view(np.uint8)), (fmt, i)
        assert res[2].pcm.size == 6 * 8 * rate // 100
        want = _convert(pkg, gm, res[0].pcm, fmt, rate)
        assert np.array_equal(res[1].pcm.view(np.uint8), want.view(np.uint8)), (fmt, rate, stream_frames)


def _g711_rank(codes, fmt):   # position of each code's decoded value among the 256 levels of the law (adjacent codes: ranks 1 apart)
    dec = R.ulaw_decode if fmt == "ulaw" else R.alaw_decode
    levels = np.unique(dec(np.arange(256)))
    return np.searchsorted(levels, dec(codes))


def _run_continuous(pkg, gm, toks, cfgs):
    d = pkg.Dispatcher([gm], max_batch=8, window_us=2000, continuous=True, cont_kv_capacity=64, cont_max_steps=32, cont_steps_per_group=3)
    n = len(toks)
    got, errs = [None] * n, [None] * n

    def client(i):
        try:
            got[i] = d.generate(toks[i], cfgs[i])
        except Exception as e:  # noqa: BLE001
            errs[i] = e
    try:
        ts = [threading.Thread(target=client, args=(i,)) for i in range(n)]
        [t.start() for t in ts]
        [t.join(300) for t in ts]
        assert not any(errs), errs
        st = d.stats()
        assert st["cont_steps"] > 0 and st["flow_cluster_fallbacks"] == 0, st
    finally:
        d.close()
    return got


def test_continuous_dispatcher_serves_mixed_rates_and_formats(pkg, tiny):
    """64 requests of mixed rates, formats and lengths through the continuous engine.  Bit-exactness against the stand-alone run is not
    possible here: the continuous engine is not bit-exact against ptts_generate for native requests either (its decoder groups and step
    kernels differ; tests/test_gpu_continuous.py holds native audio to parity 1e-4 and 2 PCM16 codes).  So the converted audio is held to
    those same bounds: f32 parity 1e-4 x max(1, max|x|), PCM16 within 2 codes, G.711 the same code or the adjacent one.  The launch count
    (process-wide: the engine converts on the dispatcher's worker thread) shows k_resample ran for the mixed traffic and never for native."""
    from _parity import parity
    cfg, gm = tiny
    rt = pkg.runtime
    rng = np.random.default_rng(7)
    n = 64
    fmts = [(FORMATS[i % 4], [0, 8000, 16000, 44100, 48000, 24000, 11025][i % 7]) for i in range(n)]
    steps = [int(rng.integers(2, 14)) for _ in range(n)]
    toks = [rng.integers(1, cfg.n_bins, size=int(rng.integers(3, 8))).astype(np.int64) for _ in range(n)]
    cfgs = [_cfg(pkg, steps[i], f, r) for i, (f, r) in enumerate(fmts)]
    want = [gm.generate_batch([toks[i]], [cfgs[i]])[0] for i in range(n)]
    rt.resample_launches(reset=True)
    got = _run_continuous(pkg, gm, toks, cfgs)
    launches = rt.resample_launches(reset=True)
    assert 0 < launches <= sum(1 for f, r in fmts if f in ("ulaw", "alaw") or r not in (0, 24000)), launches
    for i in range(n):
        f, r = fmts[i]
        assert got[i].n_frames == want[i].n_frames == steps[i]
        assert got[i].pcm.dtype == want[i].pcm.dtype and got[i].pcm.size == want[i].pcm.size == steps[i] * 8 * (r or 24000) // 100
        if f == "f32":
            parity(f"continuous {r} Hz f32 [{i}]", got[i].pcm, want[i].pcm, (1e-4, None))
        elif f == "s16":
            assert np.abs(got[i].pcm.astype(np.int32) - want[i].pcm.astype(np.int32)).max() <= 2, (i, r)
        else:
            assert np.abs(_g711_rank(got[i].pcm, f) - _g711_rank(want[i].pcm, f)).max() <= 1, (i, f, r)
    native = [i for i in range(n) if fmts[i][0] in ("f32", "s16") and fmts[i][1] in (0, 24000)]
    rt.resample_launches(reset=True)
    _run_continuous(pkg, gm, [toks[i] for i in native], [cfgs[i] for i in native])
    assert rt.resample_launches(reset=True) == 0


@pytest.mark.parametrize("rate", [8000, 48000])
@pytest.mark.parametrize("stream_frames", [1, 5])
def test_streamed_utterances_that_end_by_eos_inside_a_range(pkg, tiny, rate, stream_frames):
    """Rows 0 / 1: the same request ending by EOS (threshold -1e30: EOS at the first step, then frames_after_eos frames), streamed as 24 kHz
    f32 and at `rate` in each format; row 2 goes on to its budget, so the EOS lands inside a hand-over's range while the loop still runs.
    Row 1's hand-overs concatenate to its result, which is the one-shot conversion of row 0's audio, bit for bit."""
    cfg, gm = tiny
    toks = [[4, 8, 15], [4, 8, 15], [16, 23, 42]]
    noise = [_noise(cfg, 14, 60), _noise(cfg, 14, 60), _noise(cfg, 14, 61)]
    for fmt in FORMATS:
        got = [[] for _ in toks]
        cfgs = []
        for i in range(3):
            kw = dict(noise=noise[i], temperature=0.64, stream_frames=stream_frames, pcm_callback=lambda off, x, i=i: got[i].append((off, x.copy())))
            c = _cfg(pkg, 14, "f32" if i == 0 else fmt, 0 if i == 0 else rate, **kw)
            if i < 2:
                c = dataclasses.replace(c, eos_threshold=-1e30, frames_after_eos=6)
            cfgs.append(c)
        res = gm.generate_batch(toks, cfgs)
        assert res[0].n_frames == res[1].n_frames < 14 and res[0].eos_step == 0 and res[2].n_frames == 14
        for i in range(3):
            offs = [o for o, _ in got[i]]
            sizes = [x.size for _, x in got[i]]
            assert offs == [int(v) for v in np.cumsum([0] + sizes[:-1])] and all(sz > 0 for sz in sizes), (offs, sizes)
            cat = np.concatenate([x for _, x in got[i]])
            assert np.array_equal(cat.view(np.uint8), res[i].pcm.view(np.uint8)), (fmt, i)
        assert res[1].pcm.size == res[1].n_frames * 8 * rate // 100
        want = _convert(pkg, gm, res[0].pcm, fmt, rate)
        assert np.array_equal(res[1].pcm.view(np.uint8), want.view(np.uint8)), (fmt, rate, stream_frames)


def test_full_size_generation_at_rates_and_formats_is_the_conversion_of_the_24k_audio(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.full()
    path = str(tmp_path_factory.mktemp("rsfull") / "full.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234), dtype="BF16")
    gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_BF16, kv=pkg.KV_BF16, max_batch=8)
    try:
        toks = [[11, 220, 3051, 7], [5, 900, 41]]
        nz = [_noise(cfg, 6, 70), _noise(cfg, 6, 71)]
        base = gm.generate_batch(toks, [_cfg(pkg, 6, noise=nz[i], temperature=0.64) for i in range(2)])
        for fmt, rate in (("ulaw", 8000), ("alaw", 8000), ("s16", 16000), ("s16", 44100), ("f32", 48000), ("f32", 22050)):
            got = gm.generate_batch(toks, [_cfg(pkg, 6, fmt, rate, noise=nz[i], temperature=0.64) for i in range(2)])
            for i in range(2):
                assert got[i].pcm.size == got[i].n_frames * 8 * rate // 100
                want = _convert(pkg, gm, base[i].pcm, fmt, rate)
                assert np.array_equal(got[i].pcm.view(np.uint8), want.view(np.uint8)), (fmt, rate, i)
    finally:
        gm.close()


@pytest.mark.parametrize("rate", [48000, 44100, 16000])
def test_cloning_from_clips_at_their_own_rate(pkg, tiny, rate):
    _, gm = tiny
    n = int(1.3 * rate)
    t = np.arange(n) / rate
    x = (0.3 * np.sin(2 * np.pi * 180 * t) + 0.05 * np.random.default_rng(rate).standard_normal(n)).astype(np.float32)
    x24 = gm.resample(x, rate, 24000)
    a = gm.voice_state_from_audio(x, sample_rate=rate)
    b = gm.voice_state_from_audio(x24)
    assert a.offset == b.offset
    for layer in range(gm.info.n_layers):
        assert np.array_equal(a.read_state(layer), b.read_state(layer))
    assert np.array_equal(gm.encode_audio(x, sample_rate=rate), gm.encode_audio(x24))
    ea, eb = gm.voice_from_audio(x, sample_rate=rate), gm.voice_from_audio(x24)   # (another rate: the encoder, then the projection on its latents)
    assert tuple(ea.shape) == tuple(eb.shape) and np.array_equal(ea.data, eb.data)
    a.close()
    b.close()
    c = gm.voice_state_from_audio(x24, sample_rate=24000)
    d = gm.voice_state_from_audio(x24)
    assert np.array_equal(c.read_state(0), d.read_state(0))
    c.close()
    d.close()


def test_a_clip_over_the_cap_after_resampling_is_refused_with_its_resampled_length(pkg, tiny):
    _, gm = tiny
    cap = 512 * 1920
    n = (cap + 4000) * 2                         # at 48 kHz: over the cap once resampled
    with pytest.raises(pkg.PttsError) as ei:
        gm.voice_state_from_audio(np.zeros(n, np.float32), sample_rate=48000)
    assert ei.value.code == pkg.runtime.PTTS_EINVAL and str(R.length(n, 48000, 24000)) in str(ei.value), str(ei.value)
    ok = gm.encode_audio(np.zeros(cap * 2, np.float32) + 0.01, sample_rate=48000)   # exactly the cap after resampling
    assert ok.shape[0] == 512


def test_bad_rates_and_formats_are_refused(pkg, tiny):
    cfg, gm = tiny
    for bad in (7999, 8010, 48025, 50000, -8000, 47975):
        with pytest.raises(pkg.PttsError) as ei:
            gm.generate_batch([[1, 2, 3]], [_cfg(pkg, 3, "f32", bad)])
        assert ei.value.code == pkg.runtime.PTTS_EINVAL and str(bad) in str(ei.value), str(ei.value)
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500, continuous=True, cont_kv_capacity=64, cont_max_steps=32)
    try:
        with pytest.raises(pkg.PttsError) as ei:
            d.generate([1, 2, 3], _cfg(pkg, 3, "ulaw", 7999))
        assert ei.value.code == pkg.runtime.PTTS_EINVAL and "7999" in str(ei.value)
    finally:
        d.close()
    with pytest.raises(pkg.PttsError):
        gm.resample(np.zeros(10, np.float32), 24000, 8010)
