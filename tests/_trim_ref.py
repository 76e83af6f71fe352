"""The statement of the silence control (include/ptts.h ptts_trim_opts) in numpy, written from the header's text and not from csrc/trim.cpp: a
per-sample boolean keep mask built from np.flatnonzero of the loud mask.  And the crafted rows the CPU and the GPU tests share: the smallest
shapes at which tile (T = 1920), run (R = 30) or table (256 rows, 16 designs) logic can go wrong."""
import math

import numpy as np

T, R = 1920, 30
RATE = 24000
MS_M = {480: 20.0, 481: 20.05}   # max_pause_ms -> M: one even, one odd


def samples(ms):
    return int(ms / 1000.0 * 24000.0)


def threshold(db):
    return np.float32(math.pow(10.0, db / 20.0))


assert all(samples(ms) == m for m, ms in MS_M.items()) and samples(0.05) == 1 and samples(2.0) == 48 and samples(500.0) == 12000


def plan(x, edges=1, threshold_db=-50.0, pad_ms=30.0, max_pause_ms=0.0):
    """(keep mask [n], (lo, hi, n_out, cuts, speech))"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = x.size
    t, H, M = threshold(threshold_db), samples(pad_ms), samples(max_pause_ms)
    with np.errstate(invalid="ignore"):
        loud = np.abs(x) > t          # a NaN compares false, an infinity true, |x| == t false
    L = np.flatnonzero(loud)
    keep = np.ones(n, bool)
    if L.size == 0:
        return keep, (0, n, n, 0, 0)
    lo = max(0, int(L[0]) - H) if edges else 0
    hi = min(n, int(L[-1]) + 1 + H) if edges else n
    keep[:lo] = False
    keep[hi:] = False
    cuts, gone = 0, 0
    if M > 0:
        for u, v in zip(L[:-1].tolist(), L[1:].tolist()):
            q = v - u - 1
            if q > M:
                keep[u + 1 + (M - M // 2):v - M // 2] = False
                cuts += 1
                gone += q - M
    n_out = int(keep.sum())
    assert n_out == hi - lo - gone
    return keep, (lo, hi, n_out, cuts, 1)


def apply(x, **kw):
    """(the trimmed row -- the kept samples' own 32 bits, in order --, (lo, hi, n_out, cuts, speech))"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    keep, info = plan(x, **kw)
    return x[keep].copy(), info


# ---- crafted rows ----
THR_DB = -40.0   # t = 0.01: the quiet floor below lies under it, the loud samples far above


def quiet(n):
    """n quiet samples, every one of a window of 1021 distinct (a sample that lands in the wrong place is seen), signs alternating"""
    i = np.arange(n)
    return (np.float32(1e-3) * (1.0 + (i % 1021) / 2048.0) * np.where(i % 2, -1.0, 1.0)).astype(np.float32)


def row(n, loud_at):
    x = quiet(n)
    for i in loud_at:
        x[i] = (0.5 + 0.01 * (i % 7)) * (-1.0 if i % 3 == 0 else 1.0)
    return x


def cases():
    """[(name, row, options as keywords of TrimOpts / plan)]"""
    out = []
    both = dict(edges=1, threshold_db=THR_DB, pad_ms=0.0, max_pause_ms=20.0)
    # lengths x loud patterns
    for n in (0, 1, 2, 29, 30, 31, 1919, 1920, 1921, 3840, 3841, 5 * 1920 + 7):
        pats = {"none": [], "all": list(range(n))}
        for at in (0, n - 1, 1919, 1920):
            if 0 <= at < n:
                pats[f"one{at}"] = [at]
        for pn, loud_at in pats.items():
            out.append((f"n{n}-{pn}", row(n, loud_at), both))
            out.append((f"n{n}-{pn}-pad1", row(n, loud_at), dict(both, pad_ms=0.05)))
    # pauses of M - 1 .. M + 2 samples, for an even and an odd M, with and without the edges
    for M, ms in MS_M.items():
        for q in (M - 1, M, M + 1, M + 2):
            half_a, half_b = M - M // 2, M // 2
            places = {
                "in-tile": [100, 100 + q + 1],
                "across-edge": [T - 200, T - 200 + q + 1],
                "two-silent-tiles": [T - 20, T - 20 + 2 * T + q + 1],                   # the pause is 2 T + q samples
                "cut-starts-on-tile": [T - 1 - half_a, T - 1 - half_a + q + 1],          # u + 1 + ceil(M / 2) = T
                "cut-ends-on-tile": [2 * T + half_b - q - 1, 2 * T + half_b],            # v - floor(M / 2) = 2 T
                "cut-starts-on-run": [R * 20 - 1 - half_a, R * 20 - 1 - half_a + q + 1],
                "cut-ends-on-run": [R * 40 + half_b - q - 1, R * 40 + half_b],
                "two-cuts-in-tile": [10, 10 + q + 1, 10 + 2 * (q + 1)],
            }
            for pn, loud_at in places.items():
                n = loud_at[-1] + 57
                x = row(n, loud_at)
                out.append((f"M{M}-q{q}-{pn}-pauses-only", x, dict(edges=0, threshold_db=THR_DB, pad_ms=0.0, max_pause_ms=ms)))
                out.append((f"M{M}-q{q}-{pn}-both", x, dict(edges=1, threshold_db=THR_DB, pad_ms=0.05, max_pause_ms=ms)))
    # pads: 0, 1 sample, larger than the row, reaching past a tile edge on either side; edges without pauses
    x = row(3 * T + 11, [T + 30, T + 80, 2 * T - 20])
    for pad in (0.0, 0.05, 2.0, 500.0):
        out.append((f"pad{pad}-edges-only", x, dict(edges=1, threshold_db=THR_DB, pad_ms=pad, max_pause_ms=0.0)))
        out.append((f"pad{pad}-both", x, dict(edges=1, threshold_db=THR_DB, pad_ms=pad, max_pause_ms=20.0)))
    # special values
    n = 2 * T + 100
    x = row(n, [50, T + 700])                      # one long pause across the tile edge
    keep, _ = plan(x, edges=0, threshold_db=THR_DB, pad_ms=0.0, max_pause_ms=20.0)
    gone, stay = int(np.flatnonzero(~keep)[5]), 60
    assert keep[stay] and not keep[gone]
    x[gone] = np.nan
    x[stay] = np.nan
    x[70] = -0.0
    x[80] = 1e-40                                  # a denormal
    x.view(np.uint32)[90] = 0x7FC12345             # a NaN with a payload: moved as its 32 bits
    out.append(("nan-in-a-pause", x, dict(edges=1, threshold_db=THR_DB, pad_ms=0.0, max_pause_ms=20.0)))
    out.append(("nan-alone", np.full(T + 5, np.nan, np.float32), dict(edges=1, threshold_db=THR_DB, pad_ms=0.0, max_pause_ms=20.0)))
    y = quiet(T + 40)
    y[[7, 1000, T + 1]] = np.nan
    out.append(("nan-and-quiet", y, both))
    z = quiet(2 * T)
    z[300], z[T + 900] = np.inf, -np.inf
    out.append(("infinities-are-loud", z, both))
    t = threshold(THR_DB)
    w = np.zeros(T + 31, np.float32)
    w[100], w[200], w[T + 3] = t, -t, t            # |x| == t: quiet
    out.append(("at-the-threshold", w.copy(), both))
    w[1500] = np.nextafter(t, np.float32(1.0))     # one step above: loud
    out.append(("one-step-above", w.copy(), both))
    d = np.full(700, 1e-40, np.float32)            # denormals under the lowest threshold (t = 1e-6) ...
    out.append(("denormals", d.copy(), dict(edges=1, threshold_db=-120.0, pad_ms=0.0, max_pause_ms=20.0)))
    d[600] = 2e-6                                  # ... and one sample just over it
    out.append(("just-over-minus-120", d, dict(edges=1, threshold_db=-120.0, pad_ms=0.0, max_pause_ms=20.0)))
    # more distinct designs than one table holds (16)
    x = row(T + 50, [400, 400 + 700, T + 20])
    for k in range(20):
        out.append((f"design{k}", x, dict(edges=k % 2, threshold_db=THR_DB - k, pad_ms=0.05 * k, max_pause_ms=20.0 + k)))
    return out


def many_rows(seed=5):
    """300 rows of 1 .. 7 samples (the 256-row table boundary), every third without a trim: (rows, options or None)"""
    rng = np.random.default_rng(seed)
    rows, opts = [], []
    for i, n in enumerate(rng.integers(1, 8, 300).tolist()):
        loud_at = [j for j in range(n) if rng.random() < 0.4]
        rows.append(row(n, loud_at))
        opts.append(None if i % 3 == 1 else dict(edges=1, threshold_db=THR_DB, pad_ms=0.05 * (i % 2), max_pause_ms=0.0))
    return rows, opts
