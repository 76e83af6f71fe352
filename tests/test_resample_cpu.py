"""The resampler's specification, G.711 and the host-only entry points (no GPU): include/ptts.h ptts_resample_length, ptts_wav_header."""
import ctypes as C
import io

import numpy as np
import pytest

import _resample_ref as R

OUT_RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]
IN_RATES = [8000, 16000, 44100, 48000, 96000]


def _tone_amp(y, f, rate, lo, hi):   # least-squares amplitude of a tone of f Hz over y[lo:hi]
    t = np.arange(lo, hi) / rate
    a = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    c = np.linalg.lstsq(a, y[lo:hi], rcond=None)[0]
    return float(np.hypot(*c))


@pytest.mark.parametrize("rin,rout", [(24000, r) for r in OUT_RATES] + [(r, 24000) for r in IN_RATES])
def test_the_checker_filter_passes_and_stops_what_it_should(rin, rout):
    L, M, fc, W, A = R.filter_params(rin, rout)
    for p in range(0, L, max(1, L // 7)):   # DC gain of every phase
        d = np.arange(int(-W) - 2, int(W) + 3)
        t = p / L - d
        assert abs(R.proto(t, fc, W).sum() - 1.0) < 1e-3, (p, R.proto(t, fc, W).sum())
    nyq = min(rin, rout) / 2
    n = rin // 4
    for frac, want_db in ((0.2, 0.0), (0.8, 0.0)):
        f = frac * nyq
        y = R.resample(np.sin(2 * np.pi * f * np.arange(n) / rin), rin, rout)
        amp = _tone_amp(y, f, rout, len(y) // 4, 3 * len(y) // 4)
        assert abs(20 * np.log10(amp) - want_db) < 0.1, (f, amp)
    if rout < rin:
        for frac in (1.1, 1.5):
            f = frac * rout / 2
            if f >= 0.98 * rin / 2:   # (a tone the input cannot carry)
                continue
            y = R.resample(np.sin(2 * np.pi * f * np.arange(n) / rin), rin, rout)
            lo, hi = len(y) // 4, 3 * len(y) // 4
            assert 20 * np.log10(np.abs(y[lo:hi]).max() + 1e-30) < -60, (f, np.abs(y[lo:hi]).max())


@pytest.mark.parametrize("rin,rout", [(24000, 8000), (24000, 16000), (24000, 44100), (24000, 48000), (48000, 24000), (44100, 24000), (16000, 24000)])
def test_the_checker_agrees_with_scipy_resample_poly_on_tones(rin, rout):
    signal = pytest.importorskip("scipy.signal")
    L, M = R.pair(rin, rout)
    n = rin // 2
    x = np.sin(2 * np.pi * 0.3 * min(rin, rout) / 2 * np.arange(n) / rin) + 0.5 * np.sin(2 * np.pi * 0.1 * min(rin, rout) / 2 * np.arange(n) / rin)
    a = R.resample(x, rin, rout)
    b = signal.resample_poly(x, L, M, window=("kaiser", 8.6))
    k = min(a.size, b.size)
    lo, hi = k // 5, 4 * k // 5
    snr = 10 * np.log10(np.sum(a[lo:hi] ** 2) / np.sum((a[lo:hi] - b[lo:hi]) ** 2))
    assert snr >= 60, snr


def test_g711_known_answers_and_round_trip():
    assert R.ulaw_encode(0) == 0xFF and R.alaw_encode(0) == 0xD5
    assert R.ulaw_encode(32767) == 0x80 and R.ulaw_encode(-32768) == 0x00
    assert R.alaw_encode(32767) == 0xAA and R.alaw_encode(-32768) == 0x2A
    v = np.arange(-32768, 32768, dtype=np.int64)
    for enc, dec, shift in ((R.ulaw_encode, R.ulaw_decode, 0), (R.alaw_encode, R.alaw_decode, 0)):
        c = enc(v)
        back = dec(c)
        seg = ((c.astype(np.int64) ^ (0xFF if enc is R.ulaw_encode else 0x55)) & 0x70) >> 4
        step = 1 << (np.maximum(seg, 1) + 3)
        assert np.all(np.abs(back - np.clip(v, -32635, 32635)) <= step), int(np.abs(back - v).max())
        same = c != 0x7F if enc is R.ulaw_encode else np.ones(c.shape, bool)   # (mu-law's 0x7F is "-0": it decodes to 0, which encodes as 0xFF)
        assert np.array_equal(enc(back)[same], c[same])                         # decoded values are fixed points of the encoder
    assert len(np.unique(R.ulaw_encode(v))) == 256 and len(np.unique(R.alaw_encode(v))) == 256


def test_resample_length_matrix_and_refusals(pkg):
    rt = pkg.runtime
    for rout in OUT_RATES:
        assert rt.resample_length(1920, 24000, rout) == rout * 8 // 100   # 0.08 x rate per frame
        for n in (0, 1, 1919, 1920, 1921, 240000):
            assert rt.resample_length(n, 24000, rout) == R.length(n, 24000, rout)
    for rin in IN_RATES + [192000, 8025]:
        for n in (1, 1919, 1921, 441000):
            assert rt.resample_length(n, rin, 24000) == R.length(n, rin, 24000)
    assert rt.resample_length(7, 24000, 24000) == 7
    for bad in (0, 7999, 8010, 48025, -1):
        assert rt.resample_length(100, 24000, bad) == -rt.PTTS_EINVAL, bad
        assert str(bad) in rt.lib().ptts_last_error().decode()
    assert rt.resample_length(100, 192025, 24000) < 0 and rt.resample_length(100, 24000, 47975) < 0   # rate / a tap table beyond the bound
    assert "47975" in rt.lib().ptts_last_error().decode() and "24000" in rt.lib().ptts_last_error().decode()
    assert rt.resample_length(-1, 24000, 8000) < 0


def _hdr(tag, rate, bits, n, fmt_len):
    import struct
    bpb = bits // 8
    data = 0xFFFFFFFF if n < 0 else n * bpb
    body = struct.pack("<HHIIHH", tag, 1, rate, rate * bpb, bpb, bits)
    if fmt_len == 18:
        body += struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, 0xFFFFFFFF if n < 0 else n)
    total = 12 + 8 + len(body) + 8
    riff = 0xFFFFFFFF if n < 0 else total - 8 + data
    return b"RIFF" + struct.pack("<I", riff) + b"WAVE" + b"fmt " + struct.pack("<I", fmt_len) + body + b"data" + struct.pack("<I", data)


def test_wav_headers(pkg):
    rt = pkg.runtime
    assert rt.wav_header(24000, rt.PCM_S16, -1) == bytes(rt.wav_header_streaming())
    assert rt.wav_header(0, rt.PCM_S16, -1) == bytes(rt.wav_header_streaming())
    for rate in (8000, 16000, 44100, 48000):
        for n in (-1, 0, 12345):
            assert rt.wav_header(rate, rt.PCM_S16, n) == _hdr(1, rate, 16, n, 16)
            assert rt.wav_header(rate, rt.PCM_F32, n) == _hdr(3, rate, 32, n, 18)
            assert rt.wav_header(rate, rt.PCM_ALAW, n) == _hdr(6, rate, 8, n, 18)
            assert rt.wav_header(rate, rt.PCM_ULAW, n) == _hdr(7, rate, 8, n, 18)
    assert len(rt.wav_header(8000, rt.PCM_ULAW, 10)) == 58
    for bad in ((7999, rt.PCM_S16), (24000, 9)):
        with pytest.raises(rt.PttsError):
            rt.wav_header(bad[0], bad[1], 10)
    wavfile = pytest.importorskip("scipy.io.wavfile")
    x = (0.5 * np.sin(np.arange(1000) / 7.0)).astype(np.float32)
    for fmt, data in ((rt.PCM_F32, x), (rt.PCM_S16, (x * 32767).astype(np.int16))):
        blob = rt.wav_header(16000, fmt, x.size) + data.tobytes()
        rate, back = wavfile.read(io.BytesIO(blob))
        assert rate == 16000 and back.dtype == data.dtype and np.array_equal(back, data)


def test_abi_sizes_symbols_and_no_hooks(pkg):
    rt = pkg.runtime
    assert C.sizeof(rt._Request) == 176 and C.sizeof(rt._Result) == 56   # the sizes of ABI 0.2: the new fields took reserved ones
    assert rt._Request.sample_rate.offset == rt._Request.stream_frames.offset + 4
    assert rt._Result.pcm8.offset == rt._Result.pcm16.offset + 8
    L = rt.lib()
    for s in ("ptts_resample_length", "ptts_resample", "ptts_pcm_encode", "ptts_mimi_encode_rates", "ptts_voice_from_audio_rates", "ptts_wav_header"):
        assert s in rt.ABI_SYMBOLS and hasattr(L, s), s
    assert not [s for s in rt.HOOK_SYMBOLS if hasattr(L, s)]
    L.ptts_version.restype = C.c_char_p
    assert L.ptts_version().decode().startswith("ptts-hip 0.3")
