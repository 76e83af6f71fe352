"""Loudness normalisation on the GPU (go-pocket-tts_amd/csrc/dsp.hip, scan_block.h): the device computes the bits of
the host's blocked BS.1770 evaluation -- sub-block energies, loudness, gain and normalised samples -- whatever rows share the launch; a request's
`loudness` is ptts_loudness_normalize of that request's own 24 kHz audio, in front of `dsp` and the egress; requests without it run what they ran
before."""
import math

import numpy as np
import pytest

import _dsp_ref as D
import _loudness_ref as L
import test_gpu_dsp as TD   # the egress relations and their bounds (_check_dc, _convert), the dispatcher and raw-call helpers

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 479, 480, 1920, 1921, 9599, 9600, 9601, 122880, 122881, 240000, 487680]   # 122880 = 64 tiles: one chunk of the carry kernel
FILL = [100 + 997 * i for i in range(64)]        # the 64 other rows of a shared launch: ragged, 100 .. 62911 samples
DC_FADES = dict(dc_block=True, fade_in_ms=50.0, fade_out_ms=80.0)
STEPS = [7, 3, 9, 6, 12, 5]                       # frames of 1920 samples: 3 is under one 400 ms block (gain 1), the others are measured
TARGET = -1600


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    """The tiny synthetic model, its decoder's last (linear) convolution scaled so that the audio sits near -25 LUFS if it came out under -40."""
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    ck = synth.make_checkpoint(cfg, seed=1234)
    tmp = tmp_path_factory.mktemp("loudness")
    path = str(tmp / "tiny.safetensors")
    synth.write_safetensors(path, ck)
    gm = pkg.Model.open(path, device=0, max_batch=4)
    pcm = gm.generate_batch([[3, 7, 11]], [TD._cfg(pkg, 12)])[0].pcm
    level = pkg.runtime.loudness(pcm)
    print(f"tiny checkpoint: plain audio at {level:.2f} LUFS, peak {float(np.abs(pcm).max()):.3e}")
    if not level > -40.0:
        gm.close()
        rms = float(np.sqrt(np.mean(pcm.astype(np.float64) ** 2)))
        k = np.float32(0.05 / max(rms, 1e-30))
        for suffix in (".weight", ".bias"):
            ck["mimi.decoder.model.11.conv" + suffix] = (ck["mimi.decoder.model.11.conv" + suffix] * k).astype(np.float32)
        path = str(tmp / "tiny_scaled.safetensors")
        synth.write_safetensors(path, ck)
        gm = pkg.Model.open(path, device=0, max_batch=4)
    yield cfg, gm
    gm.close()


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_lufs(a, b):
    return (a == b) or (math.isnan(a) and math.isnan(b))


def _check_rows(pkg, gm, rows, tag):
    """The device's energies, loudness and normalised samples of `rows`, measured in one launch sequence, against the host function row by row."""
    rt = pkg.runtime
    en = gm.loudness_energies(rows)
    lu = gm.loudness_rows(rows)
    for target in (-23.0, -16.0):
        outs, meas = gm.loudness_normalize_rows(rows, target)
        for i, x in enumerate(rows):
            want, m = rt.loudness_normalize(x, target)
            assert outs[i].size == x.size and np.array_equal(_u32(outs[i]), _u32(want)), (tag, i, x.size, target)
            assert _same_lufs(float(meas[i]), m), (tag, i, x.size, float(meas[i]), m)
    for i, x in enumerate(rows):
        host = rt.loudness_energies(x)
        nan = np.isnan(host)                                   # (a NaN's sign and payload are the processor's: a NaN is held to being one)
        assert en[i].size == x.size // 480 and np.array_equal(np.isnan(en[i]), nan), (tag, i, x.size)
        assert np.array_equal(_u64(en[i])[~nan], _u64(host)[~nan]) and (np.isfinite(x).all() <= (not nan.any())), (tag, i, x.size)
        assert _same_lufs(float(lu[i]), rt.loudness(x)), (tag, i, x.size, float(lu[i]), rt.loudness(x))


@pytest.mark.parametrize("n", LENGTHS)
def test_energies_loudness_and_gain_are_the_host_bits(pkg, tiny, n):
    """A row alone, among 64 others, and with the rows in another order."""
    _, gm = tiny
    rt = pkg.runtime
    x = L.ragged(n)
    others = [L.ragged(m, seed=3) for m in FILL]
    _check_rows(pkg, gm, [x], f"alone n={n}")
    _check_rows(pkg, gm, others[:20] + [x] + others[20:], f"among 64 n={n}")
    _check_rows(pkg, gm, (others[:20] + [x] + others[20:])[::-1], f"reversed n={n}")
    single, m = gm.loudness_normalize_rows(x, -23.0)          # (the single-array form)
    assert np.array_equal(_u32(single), _u32(rt.loudness_normalize(x, -23.0)[0]))
    if n >= 9600:                                               # the case bites: the row is measured, moved, and lands on the target
        assert math.isfinite(m) and not np.array_equal(_u32(single), _u32(x))
        assert abs(L.loudness(single) - -23.0) <= 1e-4 and abs(m - L.loudness(x)) <= 1e-6
    else:
        assert m == -math.inf and np.array_equal(_u32(single), _u32(x))


def test_special_rows(pkg, tiny):
    _, gm = tiny
    rt = pkg.runtime
    quiet = (L.ragged(48000) * 1e-4).astype(np.float32)
    nan = L.ragged(24000).copy()
    nan[100] = np.nan
    rows = [np.zeros(30000, np.float32), quiet, nan, L.gated_noise(), L.sine(997.0, 1.0, 10.0)]
    _check_rows(pkg, gm, rows, "special")
    lu = gm.loudness_rows(rows)
    assert lu[0] == lu[1] == lu[2] == -math.inf and abs(lu[4] - -3.01) <= 0.1
    assert abs(lu[3] - L.loudness(rows[3])) <= 1e-6
    for bad in (-70.5, -0.5, float("nan")):
        with pytest.raises(pkg.PttsError) as ei:
            gm.loudness_normalize_rows(rows, bad)
        assert ei.value.code == rt.PTTS_EINVAL and "loudness" in str(ei.value)


def test_the_ceiling_is_peak_normalisation(pkg, tiny):
    """-1 LUFS is out of an ordinary signal's reach: the gain stops at 1 / peak and the output is `normalize`'s, bit for bit."""
    _, gm = tiny
    rows = [L.ragged(240000), L.ragged(9601), L.gated_noise(), D.signal(48000, seed=1)]
    outs, _ = gm.loudness_normalize_rows(rows, -1.0)
    want = gm.dsp_rows(rows, normalize=True)
    for x, y, w in zip(rows, outs, want):
        assert L.loudness(x) + 20.0 * math.log10(1.0 / float(np.abs(x).max())) < -1.0       # the ceiling binds
        assert np.array_equal(_u32(y), _u32(w)) and not np.array_equal(_u32(y), _u32(x)), x.size


def _toks(n):
    return [[3 + i, 7, 11 + i] for i in range(n)]


def test_generated_requests_are_the_host_function_of_their_plain_audio(pkg, tiny):
    """One-shot ptts_generate, mixed lengths, more requests than max_batch (4)."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    base = gm.generate_batch(toks, [TD._cfg(pkg, s) for s in STEPS])
    levels = [rt.loudness(b.pcm) for b in base]
    print("plain results measure", [f"{v:.2f}" for v in levels], "LUFS")
    assert all(v > -60.0 for s, v in zip(STEPS, levels) if s >= 5), levels          # the case cannot pass vacuously
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, loudness=TARGET) for s in STEPS])
    moved = 0
    for b, g, s in zip(base, got, STEPS):
        want, _ = rt.loudness_normalize(b.pcm, TARGET / 100.0)
        assert g.n_frames == b.n_frames == s and np.array_equal(_u32(g.pcm), _u32(want)), s
        moved += not np.array_equal(_u32(g.pcm), _u32(b.pcm))
    assert moved == sum(s >= 5 for s in STEPS)
    # a loudness request beside plain ones: the plain ones keep their bits
    mixed = gm.generate_batch(toks, [TD._cfg(pkg, s, loudness=TARGET if i % 2 else 0) for i, s in enumerate(STEPS)])
    for i, (b, g, m) in enumerate(zip(base, got, mixed)):
        assert np.array_equal(_u32(m.pcm), _u32(g.pcm if i % 2 else b.pcm)), i
    # with the DC block and the fades: the host chain in that order, within the DC block's one-f32-step bound
    got = gm.generate_batch(toks, [TD._cfg(pkg, s, loudness=TARGET, **DC_FADES) for s in STEPS])
    for b, g in zip(base, got):
        host = rt.dsp_apply(rt.loudness_normalize(b.pcm, TARGET / 100.0)[0], **DC_FADES)
        TD._check_dc(pkg, gm, g.pcm, host, "f32", 0, f"generate loudness+dc+fades frames={b.n_frames}")


@pytest.mark.parametrize("rate", [0, 8000, 16000, 48000])
def test_generated_requests_leave_through_the_existing_egress(pkg, tiny, rate):
    cfg, gm = tiny
    rt = pkg.runtime
    toks = _toks(len(STEPS))
    base = gm.generate_batch(toks, [TD._cfg(pkg, s) for s in STEPS])
    for fmt in TD.FORMATS:
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET) for s in STEPS])
        for b, g in zip(base, got):
            want = TD._convert(pkg, gm, rt.loudness_normalize(b.pcm, TARGET / 100.0)[0], fmt, rate)
            assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(TD._bits(g.pcm), TD._bits(want)), (fmt, rate, b.n_frames)
        got = gm.generate_batch(toks, [TD._cfg(pkg, s, fmt, rate, loudness=TARGET, **DC_FADES) for s in STEPS])
        for b, g in zip(base, got):
            host = rt.dsp_apply(rt.loudness_normalize(b.pcm, TARGET / 100.0)[0], **DC_FADES)
            TD._check_dc(pkg, gm, g.pcm, host, fmt, rate, f"generate loudness+dc+fades {fmt} {rate or 24000} Hz frames={b.n_frames}")


@pytest.mark.parametrize("continuous", [True, False])
def test_dispatcher_serves_loudness_requests(pkg, tiny, continuous):
    """Four callers at once, loudness and plain requests mixed: each result is ptts_loudness_normalize of the same request served the same way
    without `loudness`, through its egress, bit for bit; the plain request keeps its bits; and ptts_generate gives the same bits for the same
    requests."""
    cfg, gm = tiny
    rt = pkg.runtime
    specs = [(7, "f32", 0, TARGET), (6, "ulaw", 8000, TARGET), (9, "f32", 0, 0), (5, "s16", 16000, -2300)]
    toks = _toks(len(specs))
    got = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r, loudness=t) for s, f, r, t in specs], continuous)
    off = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s, f, r) for s, f, r, _ in specs], continuous)
    own = TD._run_dispatcher(pkg, gm, toks, [TD._cfg(pkg, s) for s, _, _, _ in specs], continuous)
    one = gm.generate_batch(toks, [TD._cfg(pkg, s) for s, _, _, _ in specs])
    gen = gm.generate_batch(toks, [TD._cfg(pkg, s, f, r, loudness=t) for s, f, r, t in specs])   # the same requests through ptts_generate
    for i, (s, f, r, t) in enumerate(specs):
        print(f"dispatcher continuous={continuous} [{i}]: max |dispatcher - generate| of the plain audio {float(np.abs(own[i].pcm - one[i].pcm).max()):.3e}")
        assert got[i].n_frames == s
        if not t:
            assert np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i
            continue
        assert rt.loudness(own[i].pcm) > -60.0
        want = TD._convert(pkg, gm, rt.loudness_normalize(own[i].pcm, t / 100.0)[0], f, r)
        assert got[i].pcm.dtype == want.dtype and np.array_equal(TD._bits(got[i].pcm), TD._bits(want)), (i, f, r)
        assert not np.array_equal(TD._bits(got[i].pcm), TD._bits(off[i].pcm)), i
        assert np.array_equal(TD._bits(got[i].pcm), TD._bits(gen[i].pcm)), i                      # ... give these bits


def test_refusals_name_the_field_and_the_others_run(pkg, tiny):
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [TD._cfg(pkg, 6)])[0].pcm
    cb = lambda off, x: None  # noqa: E731
    bad = [dict(normalize=True, loudness=TARGET), dict(pcm_callback=cb, loudness=TARGET), dict(loudness=-50), dict(loudness=5),
           dict(loudness=-7001), dict(loudness=1600)]
    for kw in bad:
        rc, msg, out = TD._raw_generate(pkg, gm, toks, [TD._cfg(pkg, 6, **kw), TD._cfg(pkg, 6)])
        assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and "loudness" in msg, (kw, rc, msg)
        assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32)), kw
    for ok in (-7000, -100):
        rc, msg, out = TD._raw_generate(pkg, gm, toks[:1], [TD._cfg(pkg, 6, loudness=ok)])
        assert rc == rt.PTTS_OK and out[0][0] == rt.PTTS_OK, (ok, msg)
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500, continuous=True, cont_kv_capacity=64, cont_max_steps=32)
    try:
        with pytest.raises(pkg.PttsError) as ei:
            d.generate(toks[0], TD._cfg(pkg, 4, loudness=-50))
        assert ei.value.code == rt.PTTS_EINVAL and "loudness" in str(ei.value)
    finally:
        d.close()


def test_plain_and_dsp_requests_launch_what_they_launched(pkg, tiny):
    """No loudness request in the batch: the launch census of the parent -- no loudness kernel, and for plain requests no DSP kernel and no
    k_resample either.  With one: the four loudness launches, the peak and the apply, once each for the group."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [5, 9, 13]]
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6), TD._cfg(pkg, 6, "s16")])
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith("k_loud") or k.startswith("k_dsp") or k == "k_resample"], counts
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, **TD.ALL4), TD._cfg(pkg, 6, fade_in_ms=5.0)])
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith("k_loud")], counts
    assert {k: v for k, v in counts.items() if k.startswith("k_dsp") or k == "k_resample"} == \
        {"k_dsp_peak": 1, "k_dsp_summary": 1, "k_dsp_carry": 1, "k_dsp_apply": 1, "k_resample": 1}, counts
    rt.launch_counts(True)
    gm.generate_batch(toks, [TD._cfg(pkg, 6, loudness=TARGET), TD._cfg(pkg, 6)])
    counts = rt.launch_counts(False)
    assert {k: v for k, v in counts.items() if k.startswith("k_loud") or k.startswith("k_dsp") or k == "k_resample"} == \
        {"k_dsp_peak": 1, "k_loud_summary": 1, "k_loud_carry": 1, "k_loud_energy": 1, "k_loud_gate": 1, "k_dsp_apply": 1, "k_resample": 1}, counts
    rt.launch_counts(True)
    gm.loudness_rows([L.ragged(24000)])
    counts = rt.launch_counts(False)
    assert not [k for k in counts if k.startswith("k_dsp")] and counts.get("k_loud_gate") == 1, counts
