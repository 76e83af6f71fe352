"""The de-esser of include/ptts.h (ptts_deess_*; go-pocket-tts_amd/csrc/deesser.{h,cpp}) restated independently: the side chain's high-pass as
_eq_ref's sequential section rounded to f32, the two level recurrences sample by sample (_compressor_ref.level -- not the blocked form the library
evaluates), the soft-knee curve with numpy's log10 and power (not the library's own log2 and exp2), the floor, and the band's gain.  The
yardstick of the de-esser's tests, with the inputs they share."""
import numpy as np

import _compressor_ref as CR
import _eq_ref as E

TILE = 1920
# the lengths of the issue: the run and the tile, one off either side, and a row that ends inside its sixth tile
LENGTHS = [0, 1, 29, 30, 1919, 1920, 1921, 5 * TILE + 77]
# ... and for the device two tiles exactly and 66 tiles and 31 samples, which crosses the carry kernels' batch of 64 tiles
GPU_LENGTHS = LENGTHS[:-1] + [3840, 5 * TILE + 77, 66 * TILE + 31]

# (freq_hz, q, threshold_db, ratio, knee_db, attack_ms, release_ms, max_reduction_db)
DESIGNS = {
    "soft": (5000.0, 0.7071, -30.0, 4.0, 6.0, 1.0, 60.0, 12.0),
    "hard": (7000.0, 1.2, -36.0, 10.0, 0.0, 0.2, 25.0, 24.0),
}

BURST_AT, BURST_LEN, BURST_EVERY = 600, 1440, 4800   # samples: the first burst crosses the first tile boundary


def in_burst(n):
    i = np.arange(n)
    return (i >= BURST_AT) & ((i - BURST_AT) % BURST_EVERY < BURST_LEN)


def engagement(n, seed=7):
    """A 200 Hz tone at 0.3 plus bursts of seeded noise high-passed at 6 kHz, at about 0.3: sibilants on a vowel.  A prefix of the row for n
    is the row for the prefix's length only up to the noise's scale; the tests cut prefixes from one row."""
    t = np.arange(n) / E.RATE
    rng = np.random.default_rng(seed)
    hiss = np.asarray(E.section_f64(rng.standard_normal(n).tolist(), E.design(E.HIGHPASS, 6000.0, 0.0, 0.7071)), np.float64)
    hiss *= 0.3 / max(float(np.abs(hiss).max()), 1e-30)
    return (0.3 * np.sin(2 * np.pi * 200.0 * t) + np.where(in_burst(n), hiss, 0.0)).astype(np.float32)


def band(x, design):
    return E.apply(x, [(E.HIGHPASS, design[0], 0.0, design[1])])


def gain_db(x, design):
    f, q, thr, ratio, knee, attack, release, floor = design
    with np.errstate(divide="ignore"):
        level_db = 20.0 * np.log10(CR.level(band(x, design), attack, release))
    return np.maximum(CR.curve_db(level_db, thr, ratio, knee, 0.0), -floor)


def apply(x, design):
    """The de-esser over f32 samples, sample by sample: y = x where the gain is 0 dB, else x + (g - 1) b rounded once to f32."""
    x = np.asarray(x, np.float32)
    G = gain_db(x, design)
    y = (x.astype(np.float64) + (np.power(10.0, G / 20.0) - 1.0) * band(x, design).astype(np.float64)).astype(np.float32)
    return np.where(G == 0.0, x, y)


def lib_exp2(v):
    """csrc/compressor.h cmp_exp2 restated operation by operation in float64 (Python floats: IEEE doubles, nothing contracted)."""
    k = int(v - 0.5) if v < 0.0 else int(v + 0.5)
    if k < -1020:
        return 0.0
    z = (v - float(k)) * 0.69314718055994529
    q = 1.0 / 39916800.0
    for c in (1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        q = q * z + c
    return q * 2.0 ** k


LOG2_PER_DB = 0.16609640474436813   # log2(10) / 20, csrc/compressor.h kCmpLog2PerDb
