"""The true-peak meter of include/ptts.h (ptts_true_peak; go-pocket-tts_amd/csrc/true_peak.h) restated in float64 numpy: the oversampled signal
sample by sample -- y[8 i + p] = sum over k of x[i + dlo + k] h[p][k], zeros outside the row -- on the library's own f32 taps (the hook
ptts_debug_true_peak_taps), which are first checked against a float64 statement of the design formula.  The yardstick of the true-peak tests."""
import numpy as np

L, K, DLO = 8, 54, -26
FC, BETA, ZEROS = 0.45, 8.6, 24          # cutoff in cycles per input sample, Kaiser beta, zero crossings on each side
EPS = 2.0 ** -24                          # the unit roundoff of f32


def design():
    """The taps [L][K] in float64: h(t) = 2 fc sinc(2 fc t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W = ZEROS / (2 fc), t = p / L - d."""
    W = ZEROS / (2.0 * FC)
    h = np.zeros((L, K), np.float64)
    for p in range(L):
        for k in range(K):
            t = p / L - (DLO + k)
            if abs(t) < W:
                h[p, k] = 2.0 * FC * np.sinc(2.0 * FC * t) * np.i0(BETA * np.sqrt(max(0.0, 1.0 - (t / W) ** 2))) / np.i0(BETA)
    return h


_taps = None


def taps(pkg):
    """The library's f32 taps, checked: shape (8, 54), dlo -26, each within one f32 spacing of the float64 formula."""
    global _taps
    if _taps is None:
        h, dlo = pkg.runtime.true_peak_taps()
        want = design()
        assert h.shape == (L, K) and h.dtype == np.float32 and dlo == DLO, (h.shape, h.dtype, dlo)
        assert np.all(np.abs(h.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)), "taps differ from the formula"
        assert np.abs(h).max() > 0.8                                       # the centre tap of phase 0 is 2 fc = 0.9
        _taps = h
    return _taps


def gain_sum(h):
    """S = max over the phases of sum |h[p][k]|: |y| <= S max |x|."""
    return float(np.abs(h.astype(np.float64)).sum(axis=1).max())


def oversample(x, h):
    """y [8 n] in float64 from f32 samples x [n] and taps h [L][K]."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if x.size == 0:
        return np.zeros(0, np.float64)
    pad = np.concatenate([np.zeros(-DLO), x, np.zeros(K - 1 + DLO)])
    win = np.lib.stride_tricks.sliding_window_view(pad, K)                 # win[i][k] = x[i + dlo + k]
    return (win @ h.astype(np.float64).T).reshape(-1)


def true_peak(x, h):
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return 0.0
    return max(float(np.abs(x.astype(np.float64)).max()), float(np.abs(oversample(x, h)).max()))


def y_bound(x, h):
    """|f32 fmaf chain - float64 sum| for one output: K products, each rounded into the running sum, (K + 1) eps S max |x|."""
    return (K + 1) * EPS * gain_sum(h) * float(np.abs(np.asarray(x, np.float64)).max()) if len(x) else 0.0


def tone(freq_hz, phase, amp=0.5, n=24000, taper=2400):
    """A tone of amplitude amp under a raised-cosine taper at each end (an abrupt start has a real inter-sample overshoot)."""
    t = np.arange(n)
    w = np.ones(n)
    r = 0.5 - 0.5 * np.cos(np.pi * np.arange(taper) / taper)
    w[:taper], w[n - taper:] = r, r[::-1]
    return (amp * w * np.sin(2.0 * np.pi * freq_hz * t / 24000.0 + phase)).astype(np.float32)


def burst(n, at, length=40, amp=0.7, floor=0.05, seed=0):
    """Low noise with a 6 kHz burst at phase pi / 4 over [at, at + length): every burst sample is amp / sqrt(2), the crest between them amp."""
    rng = np.random.default_rng(seed)
    x = floor * rng.uniform(-1.0, 1.0, n)
    i = np.arange(at, min(at + length, n))
    x[i] = amp * np.sin(np.pi / 2.0 * i + np.pi / 4.0)
    return x.astype(np.float32)
