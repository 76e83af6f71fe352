"""Numpy restatement of "keep the formants" around the pitch of a joined call's parts (include/ptts.h ptts_formant_opts), for the tests: the same
integers and the same frame rules, the sums in float64.

On x[0, n) at 24 kHz (samples outside read as 0): K = ceil(n / 240) frames, frame f looks at x[240 f - 240 + j], j in [0, 720).  Per frame, float64:
v = x * w, w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / 720); r[l] = sum v[j] v[j - l], l = 0 .. 24; r[0] not finite or not > 0: the identity; r[l] *=
exp(-0.5 (2 pi 60 l / 24000)^2), r[0] *= 1.0001; Levinson-Durbin (a k that is not finite or has |k| >= 1, or an E that is not > 0: the identity);
a[k] * 0.99^k.  The pair of a source time tau: b = tau - 120, f0 = floor(b / 240), rho = b - 240 f0, fa, fb = f0, f0 + 1 clamped to [0, K - 1],
u = f32(rho) / f32(240); mix(A, B) = A (1 - u) + B u.  Whiten: E_f[i] = x[i] + sum a_f[k] x[i - k]; e[i] = mix(E_fa[i], E_fb[i]) at tau = i.
Resample: _pitch_ref.resample.  Shape: output j in tile t = j // 240; Y_f[m] = e'[m] - sum a_f[k] Y_f[m - k] from zero state at 240 t - 720;
out[j] = mix(Y_fa[j], Y_fb[j]) at tau = (j p) // 1000.  Tempo: _tempo_ref."""
import numpy as np

HOP, WIN, ORDER, WARM, SLOTS = 240, 720, 24, 720, 4
GAMMA, LAG_HZ, WHITE = 0.99, 60.0, 1.0001
RATE = 24000
MIN_PITCH, MAX_PITCH = 800, 1500

W = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(WIN) + 0.5) / WIN)
LAG = np.exp(-0.5 * (2.0 * np.pi * LAG_HZ * np.arange(ORDER + 1) / RATE) ** 2)
G = GAMMA ** np.arange(ORDER + 1)


def frames(n):
    return -(-n // HOP) if n > 0 else 0


def levinson(r):
    """a[1 .. 24] of the lags r[0 .. 24] in float64, or None where the recursion leaves the stable region"""
    a = np.zeros(ORDER + 1)
    E = r[0]
    for i in range(1, ORDER + 1):
        acc = r[i] + np.dot(a[1:i], r[i - 1:0:-1])
        k = -acc / E
        if not np.isfinite(k) or abs(k) >= 1.0:
            return None
        a[1:i] = a[1:i] + k * a[i - 1:0:-1]
        a[i] = k
        E = E * (1.0 - k * k)
        if not E > 0.0:
            return None
    return a[1:]


def analyse(x):
    """[K, 24] float64: a[k] 0.99^k per frame (not rounded to f32)"""
    x = np.ascontiguousarray(x, np.float32).astype(np.float64)
    n = x.size
    K = frames(n)
    pad = np.concatenate([np.zeros(HOP), x, np.zeros(WIN)])
    out = np.zeros((K, ORDER))
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(K):
            v = pad[HOP * f:HOP * f + WIN] * W
            r = np.array([np.dot(v[l:], v[:WIN - l]) for l in range(ORDER + 1)])
            if not np.isfinite(r[0]) or not r[0] > 0.0:
                continue
            r = r * LAG
            r[0] *= WHITE
            a = levinson(r)
            if a is not None:
                out[f] = a * G[1:]
    return out


def pair(tau, K):
    """(fa, fb, u, 1 - u) of the source times tau (an int64 array): u and 1 - u as the statement's f32 values"""
    b = np.asarray(tau, np.int64) - HOP // 2
    f0 = b // HOP
    rho = b - HOP * f0
    u = rho.astype(np.float32) / np.float32(HOP)
    return np.clip(f0, 0, K - 1), np.clip(f0 + 1, 0, K - 1), u.astype(np.float64), (np.float32(1.0) - u).astype(np.float64)


def whiten(coeffs, x):
    """e[0, n) in float64 from the coefficients [K, 24] (whatever their precision) and the f32 row x"""
    x = np.ascontiguousarray(x, np.float32).astype(np.float64)
    c = np.asarray(coeffs, np.float64).reshape(-1, ORDER)
    n = x.size
    K = frames(n)
    if n == 0:
        return np.zeros(0)
    pad = np.concatenate([np.zeros(ORDER), x])
    i = np.arange(n, dtype=np.int64)
    back = pad[(i[:, None] + ORDER) - np.arange(1, ORDER + 1)[None, :]]          # [n, 24]: x[i - k]
    fa, fb, u, wa = pair(i, K)
    with np.errstate(invalid="ignore", over="ignore"):
        A = x + (c[fa] * back).sum(1)
        B = x + (c[fb] * back).sum(1)
        return A * wa + B * u


def shape(coeffs, n, p, er):
    """out[0, n_r) in float64 from the coefficients [K, 24] of the part of n samples, the pitch p and the resampled residual er (f32)"""
    er = np.ascontiguousarray(er, np.float32).astype(np.float64)
    c = np.asarray(coeffs, np.float64).reshape(-1, ORDER)
    n_r = er.size
    K = frames(n)
    if n_r == 0:
        return np.zeros(0)
    T = -(-n_r // HOP)
    t = np.arange(T, dtype=np.int64)
    f_lo = pair((t * HOP * p) // 1000, K)[0]
    f = np.minimum(f_lo[:, None] + np.arange(SLOTS)[None, :], K - 1)             # [T, 4]
    a = c[f]                                                                      # [T, 4, 24]
    pad = np.concatenate([np.zeros(WARM), er, np.zeros(HOP)])
    hist = np.zeros((T, SLOTS, ORDER))                                            # [..., k - 1]: Y[m - k]
    Y = np.zeros((T, SLOTS, HOP))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(WARM + HOP):
            acc = pad[t * HOP + s][:, None] - (a * hist).sum(2)
            hist = np.concatenate([acc[:, :, None], hist[:, :, :-1]], 2)
            if s >= WARM:
                Y[:, :, s - WARM] = acc
        j = np.arange(n_r, dtype=np.int64)
        fa, fb, u, wa = pair((j * p) // 1000, K)
        tj, rj = j // HOP, j % HOP
        assert (fb - f_lo[tj]).max() < SLOTS and (fa - f_lo[tj]).min() >= 0
        return Y[tj, fa - f_lo[tj], rj] * wa + Y[tj, fb - f_lo[tj], rj] * u


def noise(n, seed=11, amp=0.25):
    return (np.random.default_rng(seed + n).standard_normal(n) * amp).astype(np.float32)


LENGTHS = (1, 119, 121, 241, 719, 721, 4801)
VOWEL_A = (120.0, ((700, 80), (1200, 100), (2600, 140)))
VOWEL_B = (160.0, ((350, 90), (2100, 140), (2900, 200)))


def parity_rows(n):
    """{name: row of n samples}: noise, the tail of a vowel, and noise with a NaN, both infinities and denormals in it"""
    special = noise(n, 3).copy()
    for at, val in ((0, np.nan), (n // 3, np.inf), (n // 2, -np.inf), (n - 1, 1e-42), (n // 5, -1e-40)):
        if n > 5 or at == 0:
            special[min(at, n - 1)] = val
    return {"noise": noise(n), "vowel": np.ascontiguousarray(vowel(*VOWEL_A, n=max(n, 2000))[-n:]), "special": special}


def resonators(x, formants):
    """x through a cascade of two-pole resonators (hz, bandwidth): y[i] = x[i] + 2 r cos(w) y[i - 1] - r^2 y[i - 2], r = exp(-pi bw / 24000)"""
    y = np.asarray(x, np.float64)
    for hz, bw in formants:
        r = np.exp(-np.pi * bw / RATE)
        c1, c2 = 2.0 * r * np.cos(2.0 * np.pi * hz / RATE), -r * r
        out = np.zeros(y.size)
        y1 = y2 = 0.0
        for i, v in enumerate(y):
            y0 = v + c1 * y1 + c2 * y2
            out[i] = y0
            y2, y1 = y1, y0
        y = out
    return y


def response_db(formants, hz):
    """|H| of that cascade at the frequencies hz, in dB"""
    z = np.exp(-2j * np.pi * np.asarray(hz, np.float64) / RATE)
    h = np.ones(z.size, np.complex128)
    for f, bw in formants:
        r = np.exp(-np.pi * bw / RATE)
        h = h / (1.0 - 2.0 * r * np.cos(2.0 * np.pi * f / RATE) * z + r * r * z * z)
    return 20.0 * np.log10(np.abs(h))


def vowel(f0, formants, n=24000, peak=0.5):
    """a pulse train (a 1.0 at int(t) for t = 0, T, 2 T ..., T = 24000 / f0) through the cascade, scaled to the peak"""
    x = np.zeros(n)
    T = RATE / f0
    t = 0.0
    while int(t) < n:
        x[int(t)] = 1.0
        t += T
    y = resonators(x, formants)
    return (y * (peak / np.abs(y).max())).astype(np.float32)


def harmonics_db(y, f0):
    """(the harmonics k f0 up to 4 kHz, their amplitudes in dB) on the middle half of y, Hann-windowed: the projection on each harmonic's frequency"""
    y = np.asarray(y, np.float64)
    mid = y[y.size // 4:y.size // 4 + y.size // 2]
    w = np.hanning(mid.size)
    hz = f0 * np.arange(1, int(4000.0 / f0) + 1)
    t = np.arange(mid.size) / RATE
    amp = np.abs(np.exp(-2j * np.pi * hz[:, None] * t[None, :]) @ (mid * w))
    return hz, 20.0 * np.log10(np.maximum(amp, 1e-300))


def envelope_errors(y, f0_out, formants, ratio):
    """(kept, moved): the RMS deviation in dB, means removed, of y's harmonic amplitudes from the cascade's |H| at the harmonics' own frequencies and
    at those frequencies / ratio (where the envelope lies when it moved with the pitch)"""
    hz, db = harmonics_db(y, f0_out)
    db = db - db.mean()

    def err(at):
        want = response_db(formants, at)
        return float(np.sqrt(np.mean((db - (want - want.mean())) ** 2)))
    return err(hz), err(hz / ratio)


def fundamental(y, lo=60.0, hi=400.0):
    """the fundamental of y in Hz: the autocorrelation's peak on the middle half, refined by a parabola"""
    y = np.asarray(y, np.float64)
    mid = y[y.size // 4:y.size // 4 + y.size // 2]
    mid = mid - mid.mean()
    spec = np.fft.rfft(mid, 2 * mid.size)
    ac = np.fft.irfft(np.abs(spec) ** 2)[:mid.size]
    a, b = int(RATE / hi), int(RATE / lo)
    k = a + int(np.argmax(ac[a:b]))
    d = 0.5 * (ac[k - 1] - ac[k + 1]) / (ac[k - 1] - 2.0 * ac[k] + ac[k + 1])
    return RATE / (k + d)
