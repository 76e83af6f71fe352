"""The equaliser of include/ptts.h (ptts_eq_*; go-pocket-tts_amd/csrc/eq.cpp) restated: the published RBJ cookbook sections in their Q form as
float64 formulas, and the cascade as the plain sequential recurrence (direct form II transposed, float64 state, a loop over the samples -- not
the blocked form the library evaluates), rounded once to f32.  The yardstick of the equaliser's tests."""
import math

import numpy as np

RATE = 24000.0
LOWPASS, HIGHPASS, LOWSHELF, HIGHSHELF, PEAKING = 1, 2, 3, 4, 5
TYPES = [LOWPASS, HIGHPASS, LOWSHELF, HIGHSHELF, PEAKING]
FREQ, Q, GAIN = (10.0, 11000.0), (0.1, 10.0), (-24.0, 24.0)      # the parameter box of the header
# 122881: 65 tiles of 1920, where the carry kernel's loop over 64 tiles wraps; 245761: 129 tiles
LENGTHS = [0, 1, 29, 30, 31, 1919, 1920, 1921, 3840, 122880, 122881, 245761]

# the cascades the apply tests run, (type, freq_hz, gain_db, q) per section: one to four sections, then the corner of the box with the slowest
# decay (poles closest to the unit circle)
CASCADES = {
    "s1": [(HIGHPASS, 300.0, 0.0, 0.7071)],
    "s2": [(HIGHPASS, 300.0, 0.0, 0.7071), (LOWPASS, 3400.0, 0.0, 0.7071)],
    "s3": [(LOWSHELF, 200.0, -6.0, 0.8), (PEAKING, 2500.0, 5.0, 1.5), (HIGHSHELF, 6000.0, 4.0, 0.7071)],
    "s4": [(HIGHPASS, 80.0, 0.0, 0.7071), (PEAKING, 400.0, -4.0, 2.0), (PEAKING, 3000.0, 6.0, 1.0), (HIGHSHELF, 8000.0, 3.0, 0.7071)],
    "corner": [(PEAKING, 10.0, 24.0, 10.0)],
}


def gains(kind):
    return (0.0,) if kind in (LOWPASS, HIGHPASS) else (GAIN[0], 0.0, GAIN[1])


def box(kind):
    """The corners and the centre of the parameter box of one type."""
    pts = [(f, g, q) for f in FREQ for g in ((0.0,) if kind in (LOWPASS, HIGHPASS) else GAIN) for q in Q]
    return pts + [((FREQ[0] + FREQ[1]) / 2.0, 0.0 if kind in (LOWPASS, HIGHPASS) else 6.0, (Q[0] + Q[1]) / 2.0)]


def design(kind, freq_hz, gain_db, q):
    """b0, b1, b2, a1, a2, normalised by a0."""
    w0 = 2.0 * math.pi * freq_hz / RATE
    cw, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    if kind in (LOWPASS, HIGHPASS):
        a0, a1, a2 = 1.0 + alpha, -2.0 * cw, 1.0 - alpha
        if kind == LOWPASS:
            b0, b1 = (1.0 - cw) / 2.0, 1.0 - cw
        else:
            b0, b1 = (1.0 + cw) / 2.0, -(1.0 + cw)
        b2 = b0
    else:
        A = math.pow(10.0, gain_db / 40.0)
        if kind == PEAKING:
            b0, b1, b2 = 1.0 + alpha * A, -2.0 * cw, 1.0 - alpha * A
            a0, a1, a2 = 1.0 + alpha / A, -2.0 * cw, 1.0 - alpha / A
        else:
            sq, p, m = 2.0 * math.sqrt(A) * alpha, A + 1.0, A - 1.0
            if kind == LOWSHELF:
                b0, b1, b2 = A * (p - m * cw + sq), 2.0 * A * (m - p * cw), A * (p - m * cw - sq)
                a0, a1, a2 = p + m * cw + sq, -2.0 * (m + p * cw), p + m * cw - sq
            else:
                b0, b1, b2 = A * (p + m * cw + sq), -2.0 * A * (m + p * cw), A * (p + m * cw - sq)
                a0, a1, a2 = p - m * cw + sq, 2.0 * (m - p * cw), p - m * cw - sq
    return b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0


def response_db(sections, freq_hz):
    w = 2.0 * math.pi * freq_hz / RATE
    z1, z2 = complex(math.cos(w), -math.sin(w)), complex(math.cos(2 * w), -math.sin(2 * w))
    db = 0.0
    for s in sections:
        b0, b1, b2, a1, a2 = design(*s)
        db += 20.0 * math.log10(abs(b0 + b1 * z1 + b2 * z2) / abs(1.0 + a1 * z1 + a2 * z2))
    return db


def section_f64(x, c):
    """One section over float64 samples, sample by sample."""
    b0, b1, b2, a1, a2 = c
    z1 = z2 = 0.0
    out = [0.0] * len(x)
    for i, xi in enumerate(x):
        y = b0 * xi + z1
        z1 = b1 * xi - a1 * y + z2
        z2 = b2 * xi - a2 * y
        out[i] = y
    return out


def apply(x, sections):
    """The cascade over f32 samples: float64 between the sections, one rounding to f32 at the end.  A prefix of the result is the result of
    the prefix (the filter is causal)."""
    v = np.asarray(x, np.float32).astype(np.float64).tolist()
    for s in sections:
        v = section_f64(v, design(*s))
    return np.asarray(v, np.float64).astype(np.float32)


def signal(n, seed=0):
    """An offset, two tones and noise: content in every band the test cascades move."""
    t = np.arange(n) / RATE
    rng = np.random.default_rng(seed)
    return (0.2 + 0.3 * np.sin(2 * np.pi * 180.0 * t + 0.3) + 0.15 * np.sin(2 * np.pi * 2900.0 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def bound(ref):
    """Both sides are float64 evaluations of one linear system rounded once to f32: one f32 step at the row's peak (the DC block's bound)."""
    ref = np.asarray(ref, np.float32)
    return float(np.spacing(np.float32(np.abs(ref).max()))) if ref.size else 0.0
