"""Volume plus join with a seam of its own behind every part (include/ptts.h ptts_part_opts), restated in numpy float32, independent of the C code.

Part i is first scaled: with a gain g_i (an f32) every sample becomes the f32 product x * g_i, rounded once; without one its bits stay.  The seam
behind part i has G_i zeros or a crossfade of K_i = min(K_i, n_i // 2, n_(i+1) // 2) samples whose a and b are the SCALED samples:
    out = a[n_i - K_i + j] * (f32(K_i - 1 - j) / f32(K_i)) + b[j] * (f32(j) / f32(K_i))
every operation rounded once to f32.  A seam's pair (gap_ms, crossfade_ms): both negative is the default pair of the join options, otherwise a
negative field reads as 0.  A level is not restated here bit for bit: the caller hands in the part as ptts_loudness_normalize left it, with no gain."""
import numpy as np

import _join_ref as J

RATE = J.RATE


def seam_pair(gap_ms, crossfade_ms, default=(0.0, 0.0)):
    """(G, K) in samples of one seam."""
    if gap_ms < 0 and crossfade_ms < 0:
        gap_ms, crossfade_ms = default
    return J.samples(max(gap_ms, 0.0)), J.samples(max(crossfade_ms, 0.0))


def fixed_gain(gain_db):
    """The f32 gain of gain_db: (float)pow(10, gain_db / 20), the power in float64."""
    return np.float32(10.0 ** (np.float64(gain_db) / 20.0))


def offsets(lengths, seams):
    """(part offsets, joined length); seams[i] = (G, K) of the seam behind part i."""
    offs, off = [], 0
    for i, n in enumerate(lengths):
        if i:
            G, K = seams[i - 1]
            off += lengths[i - 1] + G - J.seam(K, lengths[i - 1], n)
        offs.append(off)
    return offs, (offs[-1] + lengths[-1]) if lengths else 0


def join_parts(parts, seams, gains):
    """parts: f32 arrays; seams[i] = (G, K) behind part i; gains[i]: None (the bits move) or an f32."""
    scaled = []
    for p, g in zip(parts, gains):
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        scaled.append(p if g is None else (p * np.float32(g)).astype(np.float32))   # f32 * f32 -> f32, rounded once
    lengths = [p.size for p in scaled]
    offs, total = offsets(lengths, seams)
    out = np.full(total, np.nan, np.float32)
    written = np.zeros(total, np.int32)
    for i, (p, off) in enumerate(zip(scaled, offs)):
        G, K = seams[i - 1] if i else (0, 0)
        k = J.seam(K, lengths[i - 1], p.size) if i else 0
        k_next = J.seam(seams[i][1], p.size, lengths[i + 1]) if i + 1 < len(scaled) else 0
        if i and G:
            out[off - G:off] = 0.0
            written[off - G:off] += 1
        if k:
            j = np.arange(k, dtype=np.int64)
            kf = np.float32(k)
            wa = (k - 1 - j).astype(np.float32) / kf
            wb = j.astype(np.float32) / kf
            pa = scaled[i - 1][lengths[i - 1] - k:] * wa
            pb = p[:k] * wb
            out[off:off + k] = pa + pb
            written[off:off + k] += 1
        body = p[k:p.size - k_next]
        out[off + k:off + k + body.size].view(np.uint32)[:] = body.view(np.uint32)
        written[off + k:off + k + body.size] += 1
    assert (written == 1).all()
    return out


# the seams and the volumes the tests cycle through, part after part: (gap_ms, crossfade_ms) with the default pair, a plain cut, gaps, crossfades and
# a negative field beside a set one; gain_db with none, both signs and both ends of the range
SEAM_CYCLE = [(-1.0, -1.0), (0.0, -1.0), (37.5, -1.0), (-1.0, 10.0), (0.05, 0.0), (-5.0, 2000.0), (0.0, 0.1), (2000.0, -3.0)]
GAIN_CYCLE = [0.0, -6.0, 3.0, 0.0, 0.0, -60.0, 24.0, 0.5]


def cycle(rows, shift=0):
    """(seam pairs, gain_db values) for a list of `rows` parts."""
    return ([SEAM_CYCLE[(i + shift) % len(SEAM_CYCLE)] for i in range(rows)], [GAIN_CYCLE[(i + 2 * shift) % len(GAIN_CYCLE)] for i in range(rows)])


def statement(parts, pairs, gains_db, default=(0.0, 0.0)):
    """The restatement for fixed gains: (joined audio, f32 gains as the C functions report them)."""
    seams = [seam_pair(g, c, default) for g, c in pairs]
    gains = [None if db == 0.0 else fixed_gain(db) for db in gains_db]
    return join_parts(parts, seams, gains), np.array([1.0 if g is None else g for g in gains], np.float32)


# the level rows: 0.6 s tones (14400 samples, three 400 ms blocks) at amplitude 0.05, 0.3 and 0.9, target -16 LUFS.  gain = min(sqrt(T / M), 1 / peak),
# and whether the ceiling is the smaller of the two does not depend on the amplitude of a tone but on its frequency alone (both terms scale with
# 1 / amplitude): a tone in the K-weighting's pass band measures about 20 log10(A) - 3.7 LUFS, so reaching -16 LUFS takes less than 1 / peak; far below
# the K-weighting's 38 Hz high-pass a tone measures so little that sqrt(T / M) exceeds 1 / peak.  So the 0.9 row is a 10 Hz tone (the ceiling) and the
# other two are 440 Hz tones (sqrt(T / M)): the tests assert both facts from ptts_loudness before they look at a gain.
LEVEL_TARGET = -1600   # 0.01 LUFS
LEVEL_ROWS = [(0.05, 440.0), (0.3, 440.0), (0.9, 10.0)]


def level_parts():
    t = np.arange(int(0.6 * RATE), dtype=np.float64) / RATE
    return [(a * np.sin(2.0 * np.pi * f * t)).astype(np.float32) for a, f in LEVEL_ROWS]
