"""Numpy restatement of the pitch of a joined call's parts (include/ptts.h ptts_pitch_opts), for the tests: the integer parts exactly (lengths, the
effective speed, supports, q, r), the sums in float64.

The stage on x[0, n) with p = pitch_permille and s the tempo's speed_permille (1000 without one): resample at step p / 1000 to
n_r = (n * 1000 + p - 1) / p samples, then the tempo (_tempo_ref.py) at E = (1000 * s + p / 2) / p.  The resample: R = 256, fc = 0.45,
W = 80 / 3, Kaiser beta 8.6; h[q] = f32(2 fc sinc(2 fc q / R) I0(beta sqrt(1 - (q / (R W))^2)) / I0(beta)) where 3 q < 80 R, else 0, 6828
entries; hd[q] = h[q + 1] - h[q] in f32; D = max(1000, p), g = f32(1000 / D); out[j] = g * sum over 3 |c - 1000 i| < 80 D (c = j p) of
x[i] * (hd[q] * frac + h[q]) with a = |c - 1000 i|, q = a R // D, r = a R % D, frac = f32(r) / f32(D)."""
import numpy as np

R, FC, BETA = 256, 0.45, 8.6
ENTRIES = 6828
RATE = 24000
LIMIT = (1 << 31) - 240

PITCHES = (500, 501, 707, 943, 999, 1000, 1001, 1250, 1999, 2000)
SPEEDS = (500, 800, 1000, 1250, 2000)
LENGTHS = (0, 1, 2, 479, 480, 481, 1920, 24000, 240001)


def proto(t):
    """the prototype in float64 at t input samples (D == 1000), 0 at and beyond W"""
    t = np.abs(np.asarray(t, np.float64))
    W = 80.0 / 3.0
    r = np.clip(1.0 - (t / W) ** 2, 0.0, None)
    return np.where(t < W, 2 * FC * np.sinc(2 * FC * t) * np.i0(BETA * np.sqrt(r)) / np.i0(BETA), 0.0)


def table64():
    """the float64 formula at the table's entries, [ENTRIES + 1]; entries with 3 q >= 80 R are 0"""
    q = np.arange(ENTRIES + 1)
    return np.where(3 * q < 80 * R, proto(q / R), 0.0)


def table():
    """(h, hd) as f32, [ENTRIES] each"""
    h = table64().astype(np.float32)
    return h[:-1].copy(), (h[1:] - h[:-1]).astype(np.float32)


def resample_length(n, p):
    return (n * 1000 + p - 1) // p if n > 0 else 0


def speed(s, p):
    """E, whether or not it is served"""
    return (1000 * s + p // 2) // p


def served(s, p):
    return 500 <= speed(s, p) <= 2000


def tempo_length(n, s):
    return (n * 1000) // s if n > 0 else 0


def length(n, s, p):
    return tempo_length(resample_length(n, p), speed(s, p))


def support(j, p):
    """the first and the last input of output j's support (either may lie outside the row)"""
    D = max(1000, p)
    c = j * p
    return (3 * c - 80 * D) // 3000 + 1, (3 * c + 80 * D - 1) // 3000


def resample(x, p, tab=None):
    """(y, S, A, taps): the statement in float64 on the f32 row x, with per output S = g * sum |x_i coef_i|, A = g * sum |x_i| and the count of
    the support's inputs inside the row.  The integer parts and frac are the statement's own; the sums are float64."""
    x32 = np.ascontiguousarray(x, np.float32)
    x64 = x32.astype(np.float64)
    n = x64.size
    h, hd = tab if tab is not None else table()
    h64, hd64 = h.astype(np.float64), hd.astype(np.float64)
    D = max(1000, p)
    g = float(np.float32(1000.0 / D))
    n_r = resample_length(n, p)
    y, S, A, taps = np.zeros(n_r), np.zeros(n_r), np.zeros(n_r), np.zeros(n_r, np.int64)
    K = (160 * D) // 3000 + 2
    pad = np.concatenate([np.zeros(K + 2), x64, np.zeros(2 * K + 2)])
    for j0 in range(0, n_r, 32768):
        j = np.arange(j0, min(n_r, j0 + 32768), dtype=np.int64)
        c = j * p
        lo = (3 * c - 80 * D) // 3000 + 1
        i = lo[:, None] + np.arange(K, dtype=np.int64)[None, :]
        a = np.abs(c[:, None] - 1000 * i)
        sup = 3 * a < 80 * D
        inside = sup & (i >= 0) & (i < n)
        num = np.where(sup, a, 0) * R
        q, r = num // D, num % D
        assert q.max(initial=0) <= ENTRIES - 2
        frac = (r.astype(np.float32) / np.float32(D)).astype(np.float64)
        coef = hd64[q] * frac + h64[q]
        xs = np.where(inside, pad[np.clip(i + K + 2, 0, pad.size - 1)], 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            prod = np.where(inside, xs * coef, 0.0)
            y[j] = prod.sum(1) * g
            S[j] = np.abs(prod).sum(1) * g
            A[j] = np.abs(xs).sum(1) * g
        taps[j] = inside.sum(1)
    return y, S, A, taps


def noise(n, seed=5, amp=0.5):
    return (np.random.default_rng(seed + n).standard_normal(n) * amp).astype(np.float32)


def tone(n, hz, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(n) / RATE)).astype(np.float32)


def fit_tone(y, hz, span=0.005, steps=101):
    """(the relative frequency offset, the amplitude) of the sinusoid near hz that fits y best in the least-squares sense, searched over
    hz * (1 +- span)"""
    y = np.asarray(y, np.float64)
    t = np.arange(y.size) / RATE
    best = None
    for d in np.linspace(-span, span, steps):
        w = 2.0 * np.pi * hz * (1.0 + d) * t
        M = np.stack([np.sin(w), np.cos(w)], 1)
        co, res = np.linalg.lstsq(M, y, rcond=None)[:2]
        err = float(res[0]) if res.size else float(((M @ co - y) ** 2).sum())
        if best is None or err < best[0]:
            best = (err, float(d), float(np.hypot(co[0], co[1])))
    return best[1], best[2]
