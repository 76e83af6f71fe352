"""The join of a text's parts (include/ptts.h ptts_join_opts), restated in numpy float32, independent of the C code.

Parts x_0 .. x_(R-1) at 24 kHz.  G = int(gap_ms / 1000 * 24000) zeros between consecutive parts, or a crossfade of K = int(crossfade_ms / 1000
* 24000) samples: at the seam between parts i and i+1, K_i = min(K, n_i // 2, n_(i+1) // 2) and, for j in [0, K_i),
    out = a[n_i - K_i + j] * (f32(K_i - 1 - j) / f32(K_i)) + b[j] * (f32(j) / f32(K_i))
every operation rounded once to f32.  Every other sample is copied bit for bit."""
import numpy as np

RATE = 24000
LENGTHS = [0, 1, 3, 5, 1920, 1921, 4801]
# orders of LENGTHS: as listed, reversed, empty parts at both ends and in the middle, short beside long on either side of a seam
ORDERS = [LENGTHS, LENGTHS[::-1], [4801, 0, 1, 1921, 0, 3, 1920, 5], [0, 0, 1920, 1, 4801, 3, 1921, 5, 0], [5, 4801, 3, 1920, 1, 1921]]
MODES = [dict()] + [dict(gap_ms=g) for g in (0.05, 37.5, 2000.0)] + [dict(crossfade_ms=c) for c in (0.1, 10.0, 2000.0)]


def samples(ms):
    return int(float(ms) / 1000.0 * RATE)


def seam(K, na, nb):
    return min(K, na // 2, nb // 2)


def offsets(lengths, gap_ms=0.0, crossfade_ms=0.0):
    """(part offsets, joined length)"""
    G, K = samples(gap_ms), samples(crossfade_ms)
    offs, off = [], 0
    for i, n in enumerate(lengths):
        if i:
            off += lengths[i - 1] + G - seam(K, lengths[i - 1], n)
        offs.append(off)
    return offs, (offs[-1] + lengths[-1]) if lengths else 0


def join(parts, gap_ms=0.0, crossfade_ms=0.0):
    parts = [np.ascontiguousarray(p, np.float32).reshape(-1) for p in parts]
    lengths = [p.size for p in parts]
    G, K = samples(gap_ms), samples(crossfade_ms)
    offs, total = offsets(lengths, gap_ms, crossfade_ms)
    out = np.full(total, np.nan, np.float32)
    written = np.zeros(total, np.int32)
    for i, (p, off) in enumerate(zip(parts, offs)):
        k = seam(K, lengths[i - 1], p.size) if i else 0
        k_next = seam(K, p.size, lengths[i + 1]) if i + 1 < len(parts) else 0
        if i and G:
            out[off - G:off] = 0.0
            written[off - G:off] += 1
        if k:
            j = np.arange(k, dtype=np.int64)
            kf = np.float32(k)
            wa = (k - 1 - j).astype(np.float32) / kf          # f32 / f32 -> f32, rounded once
            wb = j.astype(np.float32) / kf
            a = parts[i - 1][lengths[i - 1] - k:]
            pa = a * wa                                        # f32 products
            pb = p[:k] * wb
            out[off:off + k] = pa + pb                         # one f32 sum
            written[off:off + k] += 1
        body = p[k:p.size - k_next]
        out[off + k:off + k + body.size].view(np.uint32)[:] = body.view(np.uint32)   # the bits: NaN payloads included
        written[off + k:off + k + body.size] += 1
    assert (written == 1).all()                                # every sample once
    return out


def parts_for(lengths, seed=0):
    """One part per length: noise around an offset that differs from part to part, so that a sample taken from the wrong part shows."""
    rng = np.random.default_rng(seed)
    return [(0.1 * (i + 1) + 0.25 * rng.standard_normal(n)).astype(np.float32) for i, n in enumerate(lengths)]
