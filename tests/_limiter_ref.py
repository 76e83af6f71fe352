"""The look-ahead peak limiter of include/ptts.h (ptts_limit_*; go-pocket-tts_amd/csrc/limiter.{h,cpp}) restated independently: the hold with
numpy's sliding window, the release sample by sample in float64 (a loop over the samples -- not the blocked form the library evaluates), the
required gain rounded to f32 with r[0] in front of the row, the box sum from its first term backwards, math.pow and math.exp for the design.
The yardstick of the limiter's tests."""
import math

import numpy as np

# (ceiling_db, lookahead_ms, release_ms, drive_db)
DESIGNS = {
    "gentle": (-1.0, 1.5, 80.0, 0.0),
    "fast": (-6.0, 5.0, 5.0, 0.0),
    "driven": (0.0, 0.25, 500.0, 12.0),
}


def ahead(design):
    """L, the look-ahead in samples (Python's round is lrint's: half to even)"""
    return int(round(design[1] * 24.0))


def ceiling(design):
    return math.pow(10.0, design[0] / 20.0)


def lengths(L):
    """124801: 65 tiles of 1920 and one sample, where the carry kernel's loop over 64 tiles wraps"""
    return [0, 1, 29, 30, 31, L, L + 1, 1919, 1920, 1921, 1920 + L, 3841, 124801]


def gains(x, design):
    """(r, g): the required gain of every sample (f32) and the smoothed gain (f64)"""
    x = np.asarray(x, np.float32)
    n = x.size
    c, d, L = ceiling(design), math.pow(10.0, design[3] / 20.0), ahead(design)
    rho = math.exp(-1.0 / (design[2] * 24.0))
    a = np.abs(x.astype(np.float64)) * d
    a[np.isnan(a)] = 0.0
    m = np.lib.stride_tricks.sliding_window_view(np.concatenate([a, np.zeros(L)]), L + 1).max(axis=1)
    p = 0.0
    r = np.ones(n, np.float32)
    for i, mi in enumerate(m.tolist()):
        q = rho * p
        p = mi if mi > q else q
        if p > c:
            r[i] = np.float32(c / p)
    rr = np.concatenate([np.full(L, r[0] if n else 1.0, np.float64), r.astype(np.float64)])
    s = rr[L:].copy()                      # r[i] first, then r[i-1], ... r[i-L]: the order of the definition
    for k in range(1, L + 1):
        s = s + rr[L - k:L - k + n]
    return r, s * (1.0 / (L + 1))


def apply(x, design):
    """The limiter over f32 samples, rounded once to f32."""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return x.copy()
    d = math.pow(10.0, design[3] / 20.0)
    return ((x.astype(np.float64) * d) * gains(x, design)[1]).astype(np.float32)
