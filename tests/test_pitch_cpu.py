"""CPU-side checks of the pitch of a joined call's parts (include/ptts.h ptts_pitch_opts, ptts_pitch_*; go-pocket-tts_amd/csrc/pitch.{h,cpp};
DESIGN.md section 8, N3): the struct's layout from a C99 program; the symbols; the prototype table against the float64 formula; lengths and the
effective speed against the numpy statement of _pitch_ref.py, the refused pairs included; the resample against that statement and against the
exact filter of _resample_ref.py, within bounds computed from the operands; that the rows take every branch; tones; ptts_pitch_apply as
ptts_tempo_apply over ptts_pitch_resample; refusals that name their field; and a stand-alone program over pitch.cpp and tempo.cpp alone under
the address and undefined-behaviour sanitizers.

The bounds.  Every f32 operation of the statement rounds once: a relative error of at most u = 2^-24, or 2^-150 absolute where the result is
subnormal.  Output j is a chain of `taps` fused multiply-adds and one product over exact operands, so with S = g sum |x_i coef_i| its distance
from the exact sum of the same products is at most (taps + 3) u S (the classical bound of a recursive sum, gamma_(taps + 1), with room for the
second order).  coef itself is one fused multiply-add of the table's entries and frac = f32(r) / f32(D): frac carries at most u (it is below 1)
and coef's rounding u |coef|, so coef is within u max|hd| + u |coef| of the exact interpolation, which adds g sum |x_i| u max|hd| + u S.
(_pitch_ref.py interpolates with the statement's own f32 frac, so the first part is room, not need.)  Subnormal results add (taps + 2) 2^-149."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _pitch_ref as R
import _resample_ref as X
import _tempo_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
U = 2.0 ** -24
SYMBOLS = ("ptts_pitch_speed", "ptts_pitch_resample_length", "ptts_pitch_resample", "ptts_pitch_length", "ptts_pitch_apply", "ptts_pitch_table",
           "ptts_pitch_rows", "ptts_dsp_ext_set_pitch")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in SYMBOLS:
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    O = rt.PitchOpts
    assert C.sizeof(O) == 16 and [getattr(O, f).offset for f in ("size", "pitch_permille", "reserved")] == [0, 4, 8]
    assert O().size == 16 and O().pitch_permille == 1000
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#define O(f) offsetof(ptts_pitch_opts, f)\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_pitch_opts), O(size), O(pitch_permille), O(reserved), sizeof(((ptts_pitch_opts*)0)->reserved));\n'
                   'return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [16, 0, 4, 8, 8]


@pytest.fixture(scope="module")
def tab(pkg):
    h, hd = pkg.runtime.pitch_table()
    h.setflags(write=False)
    hd.setflags(write=False)
    return h, hd


def test_the_table(tab):
    h, hd = tab
    assert h.dtype == hd.dtype == np.float32 and h.size == hd.size == R.ENTRIES == 6828
    want = R.table64()
    step = np.spacing(np.abs(want[:-1]).astype(np.float32)).astype(np.float64)            # one f32 step at each entry
    assert (np.abs(h.astype(np.float64) - want[:-1]) <= step).all()
    q = np.arange(R.ENTRIES)
    assert (h[3 * q >= 80 * R.R] == 0.0).all() and (3 * q >= 80 * R.R).sum() == 1 and h[0] == np.float32(0.9)
    nxt = np.concatenate([h[1:], np.zeros(1, np.float32)])
    assert np.array_equal(_u32(hd), _u32(nxt - h))
    assert (h.size + hd.size) * 4 == 54624                                                  # the 54.6 KB of both


def test_lengths_and_the_effective_speed(pkg):
    rt = pkg.runtime
    L = rt.lib()
    refused = 0
    for p in R.PITCHES:
        po = rt.PitchOpts(p)
        for n in R.LENGTHS:
            assert rt.pitch_resample_length(po, n) == R.resample_length(n, p) == (-(-n * 1000 // p))
        for s in R.SPEEDS:
            for to in ((None, rt.TempoOpts(s)) if s == 1000 else (rt.TempoOpts(s),)):
                E = R.speed(s, p)
                if not R.served(s, p):
                    refused += 1
                    for call in (lambda: rt.pitch_speed(po, to), lambda: rt.pitch_length(po, to, 480), lambda: rt.pitch_apply(po, to, np.zeros(8, np.float32))):
                        with pytest.raises(pkg.PttsError) as ei:
                            call()
                        msg = str(ei.value)
                        assert ei.value.code == rt.PTTS_EINVAL and all(w in msg for w in ("speed_permille %d" % s, "pitch_permille %d" % p, str(E))), msg
                    continue
                assert rt.pitch_speed(po, to) == E
                for n in R.LENGTHS:
                    got = rt.pitch_length(po, to, n)
                    assert got == R.length(n, s, p) == T.length(R.resample_length(n, p), E), (n, s, p)
                    if n >= 24000:                                                          # the duration stays what the speed alone gives
                        want = (n * 1000) // s
                        assert abs(got - want) <= want / 1000.0, (n, s, p, got, want)
    assert refused >= 10
    # what the header says about the served pairs
    assert all(R.served(1000, p) for p in range(500, 2001))
    assert R.served(500, 1001) and not R.served(500, 1002) and R.served(2000, 1000) and not R.served(2000, 999)
    assert L.ptts_pitch_speed(None, None) == -rt.PTTS_EINVAL


def _bound(S, A, taps, hd_max):
    return (taps + 3) * U * S + A * U * hd_max + U * S + (taps + 2) * 2.0 ** -149


def _rows():
    """[(name, row)]: noise, two tones, zeros, a denormal, 3.0, and a row with a NaN and an infinity"""
    n = 700
    two = (R.tone(n, 200.0, 0.4).astype(np.float64) + R.tone(n, 3100.0, 0.3)).astype(np.float32)
    den = np.zeros(n, np.float32)
    den[::7] = np.float32(1e-41)
    den[3] = np.float32(-3e-39)
    special = R.noise(n, 11)
    special[40] = np.nan
    special[500] = np.inf
    special[650] = -np.inf
    return [("noise", R.noise(n)), ("tones", two), ("zeros", np.zeros(n, np.float32)), ("denormal", den), ("3.0", np.full(n, 3.0, np.float32)),
            ("special", special), ("short", R.noise(37)), ("one", np.full(1, 0.75, np.float32))]


@pytest.fixture(scope="module")
def refs(tab):
    """{(name, p): (row, the float64 statement, S, A, taps)}: computed once, never written to"""
    out = {}
    for name, x in _rows():
        for p in R.PITCHES:
            if p == 1000:
                continue
            y, S, A, taps = R.resample(x, p, tab)
            for a in (x, y, S, A, taps):
                a.setflags(write=False)
            out[(name, p)] = (x, y, S, A, taps)
    return out


def test_the_rows_take_every_branch(refs):
    seen = dict(head=0, tail=0, both=0, whole=0, below=0, above=0, nan=0, inf=0)
    for (name, p), (x, y, S, A, taps) in refs.items():
        j = np.arange(y.size)
        lo, hi = R.support(j, p)
        assert y.size == R.resample_length(x.size, p) and (taps == np.minimum(hi, x.size - 1) - np.maximum(lo, 0) + 1).all()
        seen["head"] += int(((lo < 0) & (hi < x.size)).sum())
        seen["tail"] += int(((lo >= 0) & (hi >= x.size)).sum())
        seen["both"] += int(((lo < 0) & (hi >= x.size)).sum())
        seen["whole"] += int(((lo >= 0) & (hi < x.size)).sum())
        seen["below" if p < 1000 else "above"] += 1
        seen["nan"] += int(np.isnan(y).sum())
        seen["inf"] += int(np.isinf(y).sum())
        assert taps.max() <= (54 if p <= 1000 else (160 * p) // 3000 + 1)
    print("outputs whose support is cut by the head / the tail / both / not at all; rows below / above 1000; NaN / infinite outputs:", seen)
    assert all(v >= 1 for v in seen.values()), seen


def test_resample_is_the_numpy_statement_within_the_computed_bound(pkg, tab, refs):
    rt = pkg.runtime
    hd_max = float(np.abs(tab[1]).max())
    worst = 0.0
    for (name, p), (x, y, S, A, taps) in refs.items():
        got = rt.pitch_resample(rt.PitchOpts(p), x)
        assert got.dtype == np.float32 and got.size == y.size, (name, p)
        fin = np.isfinite(y)
        assert np.array_equal(np.isnan(got), np.isnan(y)) and np.array_equal(got[np.isinf(y)], y[np.isinf(y)].astype(np.float32)), (name, p)
        err = np.abs(got[fin].astype(np.float64) - y[fin])
        tol = _bound(S[fin], A[fin], taps[fin], hd_max)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max(initial=0.0)))
        assert (err <= tol).all(), (name, p, float(err.max()), int((err > tol).sum()))
        if name == "zeros":
            assert not got.any()
    print(f"the largest error is {worst:.3f} of its bound")


def test_resample_is_the_exact_filter_within_the_table_error(pkg, tab, refs):
    """Against the exact filter (_resample_ref.resample(x, p, 1000): the same prototype evaluated where the statement interpolates the table).
    eps_tab, the table's linear-interpolation error, is measured here from the float64 formula at 8 sub-positions per step."""
    rt = pkg.runtime
    h, hd = (a.astype(np.float64) for a in tab)
    k = np.arange(8) / 8.0
    lin = h[:, None] + hd[:, None] * k[None, :]
    eps_tab = float(np.abs(lin - R.proto((np.arange(R.ENTRIES)[:, None] + k[None, :]) / R.R)).max())
    print(f"eps_tab = {eps_tab:.3e}")
    assert 0.0 < eps_tab < 1e-5
    hd_max = float(np.abs(tab[1]).max())
    for name in ("noise", "tones", "3.0", "denormal", "short"):
        for p in R.PITCHES:
            if p == 1000:
                continue
            x, _, S, A, taps = refs[(name, p)]
            want = X.resample(x, p, 1000)
            got = rt.pitch_resample(rt.PitchOpts(p), x).astype(np.float64)
            assert want.size == got.size == X.length(x.size, p, 1000)
            err = np.abs(got - want)
            tol = A * eps_tab + _bound(S, A, taps, hd_max)
            assert (err <= tol).all(), (name, p, float(err.max()), float(tol[err.argmax()]))
    # the prototype run's figure: a tone of amplitude 0.5 stays within 3e-6 of the exact filter
    x = R.tone(4800, 1000.0)
    for p in (707, 1250):
        assert np.abs(rt.pitch_resample(rt.PitchOpts(p), x).astype(np.float64) - X.resample(x, p, 1000)).max() <= 3e-6


TONE_PITCHES = (500, 707, 943, 1001, 1250, 1999, 2000)


@pytest.mark.parametrize("hz", [200.0, 1000.0, 3000.0])
def test_tones_move_by_the_ratio_and_keep_their_level(pkg, hz):
    rt = pkg.runtime
    x = R.tone(4800, hz)
    for p in TONE_PITCHES:
        y = rt.pitch_resample(rt.PitchOpts(p), x)
        assert y.size == R.resample_length(4800, p)
        d, amp = R.fit_tone(y[200:-200], hz * p / 1000.0)
        db = 20.0 * np.log10(amp / 0.5)
        print(f"{hz:.0f} Hz at {p}: frequency off by {d * 100:.4f} %, level {db:+.5f} dB")
        assert abs(d) <= 0.001 and abs(db) <= 0.01, (hz, p, d, db)


def test_a_tone_that_would_alias_is_removed(pkg):
    rt = pkg.runtime
    y = rt.pitch_resample(rt.PitchOpts(2000), R.tone(4800, 9000.0))
    down = -20.0 * np.log10(float(np.abs(y[200:-200]).max()) / 0.5)
    print(f"9 kHz at 2000: {down:.1f} dB down")
    assert down >= 90.0
    dc = rt.pitch_resample(rt.PitchOpts(1250), np.full(4800, 0.5, np.float32))[200:-200]
    assert 0.49998 <= dc.min() and dc.max() <= 0.50001


def test_apply_is_the_tempo_over_the_resample(pkg):
    rt = pkg.runtime
    x = R.noise(5000, 3, 0.3)
    pairs = [(p, s) for p in (500, 707, 999, 1000, 1001, 1250, 2000) for s in (None, 800, 1000, 1250) if R.served(s or 1000, p)]
    assert len(pairs) >= 20
    ran = dict(both=0, resample=0, tempo=0, neither=0)
    for p, s in pairs:
        po, to = rt.PitchOpts(p), None if s is None else rt.TempoOpts(s)
        E = rt.pitch_speed(po, to)
        z = rt.pitch_resample(po, x)
        want = rt.tempo_apply(rt.TempoOpts(E), z)
        got = rt.pitch_apply(po, to, x)
        assert got.size == want.size == rt.pitch_length(po, to, x.size) and np.array_equal(_u32(got), _u32(want)), (p, s)
        ran["both" if p != 1000 and E != 1000 else "resample" if p != 1000 else "tempo" if E != 1000 else "neither"] += 1
        if E == 1000:
            assert np.array_equal(_u32(got), _u32(z))
    assert all(v >= 1 for v in ran.values()), ran
    for row in (x, np.zeros(0, np.float32), np.array([np.nan, -0.0, np.inf, 1e-42], np.float32)):   # the identity moves the bits
        assert np.array_equal(_u32(rt.pitch_apply(rt.PitchOpts(1000), None, row)), _u32(row))
        assert np.array_equal(_u32(rt.pitch_resample(rt.PitchOpts(1000), row)), _u32(row))
    # nothing behind the result is written
    out = np.full(4100, 7.0, np.float32)
    po = rt.PitchOpts(1250)
    assert rt.lib().ptts_pitch_resample(C.byref(po), rt._fp(x), 5000, rt._fp(out)) == rt.PTTS_OK
    assert np.array_equal(_u32(out[:4000]), _u32(rt.pitch_resample(po, x))) and (out[4000:] == 7.0).all()


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 16), ("tail", C.c_uint8 * 16)]


def test_refusals_name_the_field(pkg):
    rt = pkg.runtime
    L = rt.lib()
    x = np.zeros(8, np.float32)
    ext = rt.DspExt()
    for v in (499, 2001, 0, -1000):
        o = rt.PitchOpts(v)
        for call in (lambda: rt.pitch_apply(o, None, x), lambda: rt.pitch_resample(o, x), lambda: rt.pitch_resample_length(o, 8), lambda: rt.pitch_length(o, None, 8),
                     lambda: rt.pitch_speed(o), lambda: ext.set_pitch(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and "pitch_permille" in str(ei.value), (v, str(ei.value))
    for reserved in ((1, 0), (0, -1)):
        o = rt.PitchOpts(1250, reserved=reserved)
        for call in (lambda: rt.pitch_apply(o, None, x), lambda: ext.set_pitch(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and "reserved" in str(ei.value)
    for o in (rt.PitchOpts(1250, size=8), rt.PitchOpts(1250, size=0)):
        with pytest.raises(pkg.PttsError) as ei:
            rt.pitch_apply(o, None, x)
        assert ei.value.code == rt.PTTS_EINVAL and "size" in str(ei.value)
    with pytest.raises(pkg.PttsError) as ei:                             # the tempo's own fields are the tempo's to refuse
        rt.pitch_apply(rt.PitchOpts(1250), rt.TempoOpts(2001), x)
    assert "speed_permille" in str(ei.value)
    with pytest.raises(pkg.PttsError) as ei:                             # the effective speed names both fields and both values
        rt.pitch_speed(rt.PitchOpts(2000), rt.TempoOpts(500))
    assert all(w in str(ei.value) for w in ("speed_permille 500", "pitch_permille 2000", "250"))
    # a larger struct: zeros beyond what the library knows are "off", anything else is refused
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.PitchOpts(2000, size=32)), 16)
    as_opts = C.cast(C.byref(wide), C.POINTER(rt.PitchOpts))
    assert L.ptts_pitch_resample_length(as_opts, 960) == 480
    for at in (0, 15):
        wide.tail[at] = 1
        assert L.ptts_pitch_resample_length(as_opts, 960) == -rt.PTTS_EINVAL and "size" in L.ptts_last_error().decode()
        wide.tail[at] = 0
    # lengths at the 2^31 limit: the resampled and the final length stay below 2^31 - 240
    lim = R.LIMIT
    o = rt.PitchOpts(500)
    assert L.ptts_pitch_resample_length(C.byref(o), lim // 2) == -rt.PTTS_EINVAL and "2^31" in L.ptts_last_error().decode()
    assert L.ptts_pitch_resample_length(C.byref(o), lim // 2 - 1) == lim - 2
    o = rt.PitchOpts(2000)
    assert L.ptts_pitch_resample_length(C.byref(o), 2 * lim - 1) == -rt.PTTS_EINVAL
    assert L.ptts_pitch_resample_length(C.byref(o), 2 * lim - 2) == lim - 1
    t = rt.TempoOpts(1000)                                               # E = 500: the final length is twice the resampled one
    assert L.ptts_pitch_length(C.byref(o), C.byref(t), lim) == -rt.PTTS_EINVAL and "final length" in L.ptts_last_error().decode()
    assert L.ptts_pitch_length(C.byref(o), C.byref(t), lim - 2) == lim - 2
    assert L.ptts_pitch_length(C.byref(o), None, -1) == -rt.PTTS_EINVAL and L.ptts_pitch_resample_length(C.byref(o), -1) == -rt.PTTS_EINVAL
    # pointers
    o = rt.PitchOpts(1250)
    y = np.zeros(8, np.float32)
    assert L.ptts_pitch_apply(C.byref(o), None, rt._fp(x), 8, None) == rt.PTTS_EINVAL and L.ptts_pitch_apply(C.byref(o), None, None, 8, rt._fp(y)) == rt.PTTS_EINVAL
    assert L.ptts_pitch_apply(C.byref(o), None, rt._fp(x), 8, rt._fp(x)) == rt.PTTS_EINVAL and "out is in" in L.ptts_last_error().decode()
    assert L.ptts_pitch_resample(C.byref(o), rt._fp(x), 8, rt._fp(x)) == rt.PTTS_EINVAL and "out is in" in L.ptts_last_error().decode()
    assert L.ptts_pitch_apply(C.byref(o), None, rt._fp(x), -1, rt._fp(y)) == rt.PTTS_EINVAL
    assert L.ptts_pitch_apply(None, None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_EINVAL and "null options" in L.ptts_last_error().decode()
    assert L.ptts_pitch_apply(C.byref(o), None, None, 0, None) == rt.PTTS_OK
    ext.free()


def test_the_setter_wants_a_live_handle(pkg):
    rt = pkg.runtime
    L = rt.lib()
    o = rt.PitchOpts(1100)
    ext = rt.DspExt(pitch=o)
    d = rt.DspOpts()
    d.ext = ext.h
    assert rt.dsp_opts_error(d) == ""                            # the options themselves are well formed; who may serve them is the entry point's to say
    ext.set_pitch(None)
    ext.set_pitch(o)
    h = ext.h
    ext.free()
    for dead in (h, None, 7):
        for p in (C.byref(o), None):
            rc = L.ptts_dsp_ext_set_pitch(C.c_void_p(dead), p)
            msg = L.ptts_last_error().decode(errors="replace")
            assert rc == rt.PTTS_EINVAL and "ext" in msg and "not a live handle" in msg, (dead, msg)
    with pytest.raises(pkg.PttsError) as ei:                     # the options are checked where the handle is made, and nothing leaks a handle
        rt.DspExt(pitch=rt.PitchOpts(2001))
    assert "pitch_permille" in str(ei.value)


SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "pitch.h"
namespace ptts {
static std::string g_err;
std::string strfmt(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
void set_last_error(const std::string& m) { g_err = m; }
}
using namespace ptts;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (%s)\n", __LINE__, #c, ptts::g_err.c_str()); return 1; } } while (0)
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static ptts_pitch_opts opts(int pitch) {
    ptts_pitch_opts p;
    std::memset(&p, 0, sizeof p);
    p.size = sizeof p; p.pitch_permille = pitch;
    return p;
}
static ptts_tempo_opts tempo(int speed) {
    ptts_tempo_opts t;
    std::memset(&t, 0, sizeof t);
    t.size = sizeof t; t.speed_permille = speed;
    return t;
}

// rows and outputs in blocks of exactly their size: a read or a write one element too far is reported
static int rows() {
    const long sizes[9] = {0, 1, 2, 53, 54, 107, 108, 481, 3000};
    const int pitches[9] = {500, 501, 707, 999, 1000, 1001, 1250, 1999, 2000};
    const int speeds[3] = {0, 800, 1250};   // 0: no tempo
    for (int pitch : pitches) {
        const ptts_pitch_opts p = opts(pitch);
        for (int speed : speeds) {
            const ptts_tempo_opts t = tempo(speed ? speed : 1000);
            const ptts_tempo_opts* tp = speed ? &t : nullptr;
            const int E = ptts_pitch_speed(&p, tp);
            if (E < 0) { CHECK(has(g_err, "speed_permille") && has(g_err, "pitch_permille")); continue; }
            CHECK(E == (1000 * (speed ? speed : 1000) + pitch / 2) / pitch);
            for (long n : sizes) {
                for (int pattern = 0; pattern < 3; pattern++) {   // zeros; a tone above full scale; a sawtooth with a NaN and an infinity
                    const long n_r = (long)ptts_pitch_resample_length(&p, n), n_f = (long)ptts_pitch_length(&p, tp, n);
                    CHECK(n_r == (n * 1000 + pitch - 1) / pitch && n_f == (n_r * 1000) / E);
                    float* x = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
                    float* z = static_cast<float*>(std::malloc(n_r ? (size_t)n_r * sizeof(float) : 1));
                    float* y = static_cast<float*>(std::malloc(n_f ? (size_t)n_f * sizeof(float) : 1));
                    float* w = static_cast<float*>(std::malloc(n_f ? (size_t)n_f * sizeof(float) : 1));
                    CHECK(x && y && z && w);
                    for (long i = 0; i < n; i++) x[i] = pattern == 0 ? 0.0f : pattern == 1 ? 1.5f * std::sin(0.05f * (float)i) : (float)(i % 97) / 97.0f - 0.5f;
                    if (pattern == 2 && n > 300) { x[7] = NAN; x[300] = INFINITY; }
                    CHECK(ptts_pitch_resample(&p, n ? x : nullptr, n, n_r ? z : nullptr) == PTTS_OK);
                    CHECK(ptts_pitch_apply(&p, tp, n ? x : nullptr, n, n_f ? y : nullptr) == PTTS_OK);
                    const ptts_tempo_opts te = tempo(E);
                    CHECK(ptts_tempo_apply(&te, n_r ? z : nullptr, n_r, n_f ? w : nullptr) == PTTS_OK);
                    if (pattern < 2) CHECK(n_f == 0 || std::memcmp(y, w, (size_t)n_f * sizeof(float)) == 0);
                    if (pitch == 1000) CHECK(n == n_r && (n == 0 || std::memcmp(x, z, (size_t)n * sizeof(float)) == 0));
                    if (pattern == 0) for (long i = 0; i < n_r; i++) CHECK(z[i] == 0.0f);
                    std::free(x);
                    std::free(z);
                    std::free(y);
                    std::free(w);
                }
            }
        }
    }
    return 0;
}

static int refusals() {
    float x[8] = {0}, y[16];
    ptts_pitch_opts p = opts(1250);
    CHECK(ptts_pitch_apply(&p, nullptr, nullptr, 4, y) == PTTS_EINVAL && has(g_err, "null"));
    CHECK(ptts_pitch_apply(&p, nullptr, x, -1, y) == PTTS_EINVAL);
    CHECK(ptts_pitch_apply(&p, nullptr, x, 8, x) == PTTS_EINVAL && has(g_err, "out is in"));
    CHECK(ptts_pitch_apply(nullptr, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "null options"));
    CHECK(ptts_pitch_resample_length(&p, ((int64_t)1 << 33)) == -PTTS_EINVAL && has(g_err, "2^31"));
    p = opts(499);
    CHECK(ptts_pitch_apply(&p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "pitch_permille"));
    p = opts(2001);
    CHECK(ptts_pitch_length(&p, nullptr, 8) == -PTTS_EINVAL && has(g_err, "pitch_permille"));
    p = opts(1250);
    p.reserved[1] = 3;
    CHECK(ptts_pitch_apply(&p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "reserved"));
    p = opts(1250);
    p.size = 8;
    CHECK(ptts_pitch_apply(&p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "size"));
    p = opts(2000);
    const ptts_tempo_opts t = tempo(500);
    CHECK(ptts_pitch_speed(&p, &t) == -PTTS_EINVAL && has(g_err, "speed_permille 500") && has(g_err, "pitch_permille 2000") && has(g_err, "250"));
    const float *h = nullptr, *hd = nullptr;
    int32_t k = 0;
    CHECK(ptts_pitch_table(&h, &hd, &k) == PTTS_OK && k == kPitchEntries && h[0] == 0.9f && h[k - 1] == 0.0f && hd[k - 1] == 0.0f && hd[0] == h[1] - h[0]);
    CHECK(ptts_pitch_table(nullptr, nullptr, nullptr) == PTTS_OK);
    const PitchScan d = pitch_design(opts(1250));
    CHECK(d.p == 1250 && d.D == 1250 && d.g == 0.8f && pitch_design(opts(800)).D == 1000 && pitch_design(opts(800)).g == 1.0f);
    CHECK(pitch_first(0, 1000) == -26 && pitch_last(0, 1000) == 26 && pitch_first(80000, 1000) == 54 && pitch_last(80000, 1000) == 106);
    return 0;
}

int main() {
    if (rows() || refusals()) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/pitch.cpp and csrc/tempo.cpp alone, built with g++ -fsanitize=address,undefined and run as a subprocess.
    Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "pitch_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "pitch_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), os.path.join(CSRC, "pitch.cpp"), os.path.join(CSRC, "tempo.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
