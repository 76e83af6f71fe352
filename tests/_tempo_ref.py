"""The statement of the tempo change (include/ptts.h ptts_tempo_opts) in numpy, written from the header's text and not from csrc/tempo.cpp: the
quantised view as one array, a hop's 481 sums from a sliding window over it, the choice by three successive selections (least S, least |d|, the
negative one), the blend as separate float32 array operations.  And the crafted rows the CPU and the GPU tests share."""
import numpy as np

HS, D = 480, 240
RATE = 24000
LENGTHS = (0, 1, 2, 479, 480, 481, 959, 961, 1920, 1921, 4801, 7777)
SPEEDS = (500, 501, 999, 1000, 1001, 1250, 1999, 2000)


def length(n, s):
    return (n * 1000) // s if n > 0 else 0


def hops(n_out):
    return (n_out + HS - 1) // HS


def quantise(x):
    """int32 [n]: 0 for a NaN, else trunc(clamp(x, -1, 1) * 32767) with the product in float32"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    nan = np.isnan(x)
    c = np.clip(np.where(nan, np.float32(0), x), np.float32(-1), np.float32(1)).astype(np.float32)
    v = c * np.float32(32767.0)
    assert v.dtype == np.float32
    return np.trunc(v).astype(np.int32)


def _read(a, start, count):
    """a[start, start + count) with zeros outside the array"""
    out = np.zeros(count, a.dtype)
    lo, hi = max(start, 0), min(start + count, a.size)
    if hi > lo:
        out[lo - start:hi - start] = a[lo:hi]
    return out


def plan(x, s):
    """(positions int64 [F], lags int64 [F] (0 for hop 0), continues bool [F])"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    F = hops(length(x.size, s))
    q = quantise(x).astype(np.int64)
    p = np.zeros(F, np.int64)
    lag = np.zeros(F, np.int64)
    cont = np.ones(F, bool)
    for k in range(1, F):
        a = (k * HS * s) // 1000
        c = int(p[k - 1]) + HS
        tmpl = _read(q, c, HS)
        win = np.lib.stride_tricks.sliding_window_view(_read(q, a - D, 2 * D + HS), HS)   # [481][480]: row i is the lag i - D
        S = np.abs(win - tmpl[None, :]).sum(axis=1)
        assert S.max() < 2 ** 31
        d = np.arange(-D, D + 1)
        best = d[S == S.min()]
        best = best[np.abs(best) == np.abs(best).min()]
        lag[k] = best.min()                        # of -|d| and +|d| the negative one
        p[k] = a + lag[k]
        cont[k] = p[k] == c
    return p, lag, cont


def apply(x, s, positions=None):
    """the time-scaled row, float32 [length(n, s)]"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n_out = length(x.size, s)
    out = np.zeros(n_out, np.float32)
    p = plan(x, s)[0] if positions is None else positions
    j = np.arange(HS)
    w_out = (HS - j).astype(np.float32) / np.float32(HS)
    w_in = j.astype(np.float32) / np.float32(HS)
    for k in range(hops(n_out)):
        m0 = k * HS
        cnt = min(HS, n_out - m0)
        new = _read(x, int(p[k]), HS)
        c = int(p[k - 1]) + HS if k else 0
        if k == 0 or int(p[k]) == c:
            seg = new                              # the samples' own 32 bits
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                pa = _read(x, c, HS) * w_out
                pb = new * w_in
                seg = pa + pb
            assert seg.dtype == np.float32
        out.view(np.uint32)[m0:m0 + cnt] = seg.view(np.uint32)[:cnt]
    return out


# ---- crafted rows ----
def tone(n, hz, amp=0.5):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(n) / RATE)).astype(np.float32)


def noise(n, amp=0.2, seed=11):
    return (amp * np.random.default_rng(seed + n).standard_normal(n)).astype(np.float32)


def contents(n):
    return {
        "noise": noise(n),
        "tone137": tone(n, 137.0),
        "tone200": tone(n, 200.0),
        "zero": np.zeros(n, np.float32),                       # every lag ties: the least |d| decides
        "tiny": noise(n, 1e-6),                                # everything quantises to 0, the samples are not 0
        "loud": (tone(n, 137.0, 3.0) + noise(n, 0.05)).astype(np.float32),   # the search clamps, the output does not
    }


def special(n):
    """noise with NaN (one with a payload), both infinities, -0 and a denormal in it"""
    x = noise(n, 0.2, seed=23)
    at = [i for i in (3, 100, 479, 480, 700, 1500, 1919, 1920, 3000, n - 1) if 0 <= i < n]
    values = [np.nan, np.inf, -np.inf, np.nan, -0.0, 1e-40, np.inf, np.nan, -np.inf, np.nan]
    for i, v in zip(at, values):
        x[i] = v
    if n > 250:
        x.view(np.uint32)[250] = 0x7FC12345
    return x


# At these speeds the continuation stays inside the search window for the whole of these rows (the target drifts by less than half a sample a
# hop), and on noise it is the one perfect match: every hop continues, and every NaN and infinity goes through a copy.  (Where a blend read one,
# the bits of the result would be those of the processor's NaN rules, which the statement does not fix.)
SPECIAL_SPEEDS = (999, 1000, 1001)
SPECIAL_LENGTHS = (481, 1921, 4801, 7777)


def cases():
    """[(name, row, speed_permille)]"""
    out = []
    for n in LENGTHS:
        for cn, x in contents(n).items():
            for s in SPEEDS:
                out.append((f"n{n}-{cn}-s{s}", x, s))
    for n in SPECIAL_LENGTHS:
        x = special(n)
        for s in SPECIAL_SPEEDS:
            out.append((f"n{n}-special-s{s}", x, s))
    return out


def many_rows():
    """325 rows of 481 samples, speeds mixed, every fifth row without a tempo: 260 rows go to the device, four more than one table holds.
    (rows, speeds or None)"""
    rows, speeds = [], []
    for i in range(325):
        rows.append(noise(481, 0.2, seed=100 + i) if i % 2 else tone(481, 90.0 + 3.0 * i))
        speeds.append(None if i % 5 == 4 else (500, 800, 1000, 1250, 2000, 667, 1500)[i % 7])
    return rows, speeds


# ---- what the property test measures ----
def crossing_frequency(y):
    """Hz, from the positive-going zero crossings of y (linear interpolation between the two samples of a crossing)"""
    y = np.asarray(y, np.float64)
    i = np.flatnonzero((y[:-1] < 0.0) & (y[1:] >= 0.0))
    t = i + y[i] / (y[i] - y[i + 1])
    return (t.size - 1) / (t[-1] - t[0]) * RATE
