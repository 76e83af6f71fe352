"""The post-processing chain of ptts_dsp_apply (go-pocket-tts_amd/csrc/dsp.cpp; internal/audio/dsp.go:12-78, order of cmd/pockettts/synth.go:361-390)
restated in numpy: float32 steps where dsp.cpp uses float32, the biquad sequential in float64.  The yardstick of the device chain's tests."""
import math

import numpy as np

RATE = 24000
LENGTHS = [1, 29, 1919, 1920, 1921, 48000, 122880, 122881, 240000]   # 122880 = 64 tiles: one chunk of the carry kernel, then one tile over it


def signal(n, seed=0, offset=0.3):
    """A DC offset (so that a skipped filter shows), a tone and noise."""
    t = np.arange(n) / RATE
    rng = np.random.default_rng(seed + n)
    return (offset + 0.35 * np.sin(2 * np.pi * 180.0 * t + 0.3) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def peak_normalize(x):
    x = np.asarray(x, np.float32)
    a = np.abs(x)
    a = a[~np.isnan(a)]
    peak = np.float32(a.max()) if a.size else np.float32(0)
    if peak == 0:
        return x.copy()
    gain = np.float32(1.0) / peak
    return (x * gain).astype(np.float32)


def dc_coeffs(rate=RATE):
    w0 = 2.0 * math.pi * 20.0 / float(rate)
    q = 0.707
    cw, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    a0 = 1.0 + alpha
    b0 = (1.0 + cw) / 2.0 / a0
    return b0, -(1.0 + cw) / a0, b0, -2.0 * cw / a0, (1.0 - alpha) / a0


def dc_block(x, rate=RATE):
    b0, b1, b2, a1, a2 = dc_coeffs(rate)
    z1 = z2 = 0.0
    out = np.empty(len(x), np.float64)
    for i, xi in enumerate(np.asarray(x, np.float32).astype(np.float64).tolist()):
        y = b0 * xi + z1
        z1 = b1 * xi - a1 * y + z2
        z2 = b2 * xi - a2 * y
        out[i] = y
    return out.astype(np.float32)


def _fade(ms, n):
    return min(int(ms / 1000.0 * RATE), n)


def fade_in(x, ms):
    x = np.asarray(x, np.float32).copy()
    f = _fade(ms, x.size)
    if f > 0:
        x[:f] = x[:f] * (np.arange(f).astype(np.float32) / np.float32(f))
    return x


def fade_out(x, ms):
    x = np.asarray(x, np.float32).copy()
    n = x.size
    f = _fade(ms, n)
    if f > 0:
        x[n - f:] = x[n - f:] * ((n - 1 - np.arange(n - f, n)).astype(np.float32) / np.float32(f))
    return x


def apply(x, normalize=False, dc=False, fade_in_ms=0.0, fade_out_ms=0.0):
    x = np.asarray(x, np.float32).reshape(-1).copy()
    if normalize:
        x = peak_normalize(x)
    if dc:
        x = dc_block(x)
    if fade_in_ms > 0:
        x = fade_in(x, fade_in_ms)
    if fade_out_ms > 0:
        x = fade_out(x, fade_out_ms)
    return x


def dc_bound(host):
    """Both sides are float64 evaluations of the same linear system rounded once to f32: they differ by at most one f32 step at the row's peak."""
    host = np.asarray(host, np.float32)
    return float(np.spacing(np.float32(np.abs(host).max()))) if host.size else 0.0
