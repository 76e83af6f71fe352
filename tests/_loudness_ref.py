"""ITU-R BS.1770-4 integrated loudness (mono), restated sequentially in float64 numpy: the yardstick of ptts_loudness and of the device kernels
(go-pocket-tts_amd/csrc/scan_block.h, dsp.hip).  K-weighting by the bilinear forms that reproduce the standard's
48 kHz table, evaluated for the sample rate; 400 ms blocks every 100 ms; the gates in the logarithmic domain, as the standard words them."""
import math

import numpy as np

try:
    from scipy.signal import lfilter as _lfilter
except ImportError:   # the plain recurrence (direct form II transposed)
    _lfilter = None

FS = 24000
ABS_GATE_LUFS = -70.0


def kweighting(fs):
    """(b, a) of the high shelf and of the high-pass."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, hp


def _filter(b, a, x):
    if _lfilter is not None:
        return _lfilter(b, a, x)
    y = np.empty_like(x)
    z1 = z2 = 0.0
    for i, xi in enumerate(x):
        yi = b[0] * xi + z1
        z1 = b[1] * xi - a[1] * yi + z2
        z2 = b[2] * xi - a[2] * yi
        y[i] = yi
    return y


def kweighted(x, fs=FS):
    y = np.asarray(x, np.float64).reshape(-1)
    for b, a in kweighting(fs):
        y = _filter(b, a, y)
    return y


def block_loudness(x, fs=FS):
    """Loudness of every whole 400 ms block (hop 100 ms), in LUFS (-inf for a silent block)."""
    y = kweighted(x, fs)
    blk, hop = int(0.4 * fs), int(0.1 * fs)
    nb = (y.size - blk) // hop + 1 if y.size >= blk else 0
    z = np.array([float(np.mean(y[j * hop: j * hop + blk] ** 2)) for j in range(nb)], np.float64)
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def gates(x, fs=FS):
    """(block mean squares, block loudness, absolute-gate mask, relative threshold in LUFS or None)."""
    z, l = block_loudness(x, fs)
    m_abs = l > ABS_GATE_LUFS
    if not m_abs.any():
        return z, l, m_abs, None
    rel = -0.691 + 10.0 * math.log10(float(np.mean(z[m_abs]))) - 10.0
    return z, l, m_abs, rel


def loudness(x, fs=FS):
    """Integrated loudness in LUFS; -inf when no block passes the gates."""
    z, l, m_abs, rel = gates(x, fs)
    if rel is None:
        return -math.inf
    m = m_abs & (l > rel)
    if not m.any():
        return -math.inf
    return -0.691 + 10.0 * math.log10(float(np.mean(z[m])))


def gate_margin(x, fs=FS):
    """The smallest distance, in LU, of a block's loudness from the gate that decides it (inf: no block)."""
    z, l, m_abs, rel = gates(x, fs)
    fin = np.isfinite(l)
    d = [np.abs(l[fin] - ABS_GATE_LUFS)]
    if rel is not None:
        d.append(np.abs(l[m_abs] - rel))
    d = np.concatenate(d) if d else np.zeros(0)
    return float(d.min()) if d.size else math.inf


def sine(freq, amp, seconds, fs=FS):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return (amp * np.sin(2.0 * math.pi * freq * t)).astype(np.float32)


def gated_noise(n=240000, seed=5, fs=FS):
    """Gaussian noise at 0.1 with a 2.5 s stretch scaled by 1e-4: the blocks that straddle the stretch's edges pass the absolute gate and some
    of them fail the relative one; the blocks inside it fail the absolute gate."""
    x = np.random.default_rng(seed).standard_normal(n) * 0.1
    a = int(3.0 * fs)
    x[a: a + int(2.5 * fs)] *= 1e-4
    return x.astype(np.float32)


def ragged(n, seed=11):
    """Speech-like test audio of any length: a few partials under a slow envelope, plus noise."""
    rng = np.random.default_rng(seed + n % 1000)
    t = np.arange(n, dtype=np.float64) / FS
    x = 0.2 * np.sin(2 * math.pi * 220.0 * t) + 0.1 * np.sin(2 * math.pi * 1330.0 * t + 0.3) + 0.05 * np.sin(2 * math.pi * 3100.0 * t)
    x *= 0.6 + 0.4 * np.sin(2 * math.pi * 1.7 * t)
    x += 0.02 * rng.standard_normal(n)
    return x.astype(np.float32)
