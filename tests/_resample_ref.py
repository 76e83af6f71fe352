"""Float64 restatement of the resampler (include/ptts.h) and of G.711 encode / decode, for the tests.

For (R_in, R_out): g = gcd, L = R_out / g, M = R_in / g, rho = min(1, L / M), fc = 0.45 rho, W = 24 / (2 fc), Kaiser beta 8.6;
h(t) = 2 fc sinc(2 fc t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W.  y[j] = sum over |j M / L - i| < W of x[i] h(j M / L - i),
x zero outside [0, n); n_out = ceil(n L / M).  The support test is the exact integer one: 3 |p - d L| < 80 max(L, M) (p = j M mod L,
i = floor(j M / L) + d)."""
from math import gcd

import numpy as np

BETA, Z = 8.6, 24


def pair(rin, rout):
    g = gcd(rin, rout)
    return rout // g, rin // g


def length(n, rin, rout):
    L, M = pair(rin, rout)
    return -(-n * L // M)


def filter_params(rin, rout):
    L, M = pair(rin, rout)
    rho = min(1.0, L / M)
    fc = 0.5 * rho * 0.9
    return L, M, fc, Z / (2 * fc), 80 * max(L, M)


def proto(t, fc, W):
    t = np.asarray(t, np.float64)
    r = np.clip(1.0 - (t / W) ** 2, 0.0, None)
    return np.where(np.abs(t) < W, 2 * fc * np.sinc(2 * fc * t) * np.i0(BETA * np.sqrt(r)) / np.i0(BETA), 0.0)


def resample(x, rin, rout):
    """float64 y of float64-widened x."""
    x = np.asarray(x, np.float64)
    n = x.size
    if rin == rout:
        return x.copy()
    L, M, fc, W, A = filter_params(rin, rout)
    n_out = length(n, rin, rout)
    dlo = -(A // (3 * L)) - 1
    dhi = -(-(3 * (L - 1) + A) // (3 * L))
    d = np.arange(dlo, dhi + 1)
    out = np.zeros(n_out)
    xp = np.concatenate([np.zeros(d.size), x, np.zeros(d.size)])
    for j0 in range(0, n_out, 65536):
        j = np.arange(j0, min(n_out, j0 + 65536))
        base, p = (j * M) // L, (j * M) % L
        dd = d[None, :]
        sup = 3 * np.abs(p[:, None] - dd * L) < A
        h = np.where(sup, proto(p[:, None] / L - dd, fc, W), 0.0)
        xs = xp[base[:, None] + dd + d.size]
        out[j] = (xs * h).sum(1)
    return out


def pcm16(x):
    """audio.WritePCM16Samples: int16(clamp(s, -1, 1) * 32767), truncation, NaN -> 0."""
    x = np.asarray(x, np.float32).astype(np.float64)
    v = np.trunc(np.clip(x, -1.0, 1.0) * 32767.0)
    return np.where(np.isnan(x), 0, v).astype(np.int16)


def _seg(v, first):
    s = np.zeros_like(v)
    for k in range(8):
        s += (v >= (first << k)).astype(v.dtype)
    return s


def ulaw_encode(v):
    v = np.asarray(v, np.int64)
    mask = np.where(v < 0, 0x7F, 0xFF)
    a = np.minimum(np.abs(v), 32635) + 0x84
    seg = _seg(a, 0x100)
    u = np.where(seg >= 8, 0x7F, (seg << 4) | ((a >> np.minimum(seg + 3, 15)) & 0xF))
    return ((u ^ mask) & 0xFF).astype(np.uint8)


def alaw_encode(v):
    v = np.asarray(v, np.int64) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    a = np.where(v >= 0, v, -v - 1)
    seg = _seg(a, 0x20)
    q = np.where(seg < 2, a >> 1, a >> np.minimum(seg, 15)) & 0xF
    c = np.where(seg >= 8, 0x7F, (seg << 4) | q)
    return ((c ^ mask) & 0xFF).astype(np.uint8)


def ulaw_decode(c):
    u = (~np.asarray(c, np.int64)) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw_decode(c):
    a = np.asarray(c, np.int64) ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 0x0F) << 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t)
