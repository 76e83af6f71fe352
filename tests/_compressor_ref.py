"""The dynamic range compressor of include/ptts.h (ptts_compress_*; go-pocket-tts_amd/csrc/compressor.{h,cpp}) restated independently: the two
level recurrences sample by sample in float64 (a loop over the samples -- not the blocked form the library evaluates), the soft-knee curve of
Giannoulis, Massberg and Reiss with numpy's log10 and power (not the library's own log2 and exp2), one rounding to f32.  The yardstick of the
compressor's tests."""
import math

import numpy as np

# 124801: 65 tiles of 1920 and one sample, where the carry kernels' loop over 64 tiles wraps
LENGTHS = [0, 1, 29, 30, 31, 1919, 1920, 1921, 3841, 124801]

# (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db)
DESIGNS = {
    "hard": (-24.0, 4.0, 0.0, 5.0, 120.0, 0.0),
    "knee6": (-24.0, 4.0, 6.0, 5.0, 120.0, 0.0),
    "ratio100": (-30.0, 100.0, 12.0, 1.0, 50.0, 6.0),
}


def curve_db(level_db, threshold_db, ratio, knee_db, makeup_db):
    """The static curve: gain in dB at a level in dB (arrays or scalars; -inf is a level)."""
    L = np.asarray(level_db, np.float64)
    over = L - threshold_db
    slope = 1.0 / ratio - 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        quad = slope * (over + knee_db / 2.0) ** 2 / (2.0 * knee_db) if knee_db > 0.0 else np.zeros_like(L)
        g = np.where(2.0 * over > knee_db, slope * over, np.where(2.0 * over < -knee_db, 0.0, quad))
    return g + makeup_db


def level(x, attack_ms, release_ms):
    """s[n]: the peak detector with release, then the attack smoothing, sample by sample.  A NaN never wins."""
    rho = math.exp(-1.0 / (release_ms * 24.0))
    alpha = math.exp(-1.0 / (attack_ms * 24.0))
    beta = 1.0 - alpha
    p = s = 0.0
    out = [0.0] * len(x)
    for i, a in enumerate(np.abs(np.asarray(x, np.float32).astype(np.float64)).tolist()):
        r = rho * p
        p = a if a > r else r
        s = alpha * s + beta * p
        out[i] = s
    return np.asarray(out, np.float64)


def gain_db(x, design):
    t, r, w, at, rel, mk = design
    with np.errstate(divide="ignore"):
        return curve_db(20.0 * np.log10(level(x, at, rel)), t, r, w, mk)


def apply(x, design):
    """The compressor over f32 samples, rounded once to f32.  A prefix of the result is the result of the prefix (it is causal)."""
    x = np.asarray(x, np.float32)
    return (x.astype(np.float64) * np.power(10.0, gain_db(x, design) / 20.0)).astype(np.float32)


def burst(n):
    """A loud burst of a quarter of a second, then a quiet tail: the release is what the tail hears."""
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(5)
    env = np.where(t < 0.25, 0.8, 0.01)
    return (env * (np.sin(2 * np.pi * 220.0 * t) + 0.1 * rng.standard_normal(n))).astype(np.float32)
