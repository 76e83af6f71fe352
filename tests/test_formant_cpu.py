"""CPU-side checks of "keep the formants" around the pitch of a joined call's parts (include/ptts.h ptts_formant_opts, ptts_formant_*;
go-pocket-tts_amd/csrc/formant.{h,cpp}): the struct's layout from a C99 program; the symbols; frames and lengths; the three
host statements against the float64 numpy restatement of _formant_ref.py; the properties the option is for, measured on synthetic vowels; exactness
and the bounds of what a NaN reaches; refusals that name their field; and a stand-alone program over formant.cpp, pitch.cpp and tempo.cpp alone
under the address and undefined-behaviour sanitizers.

The parity bounds.  The host statement rounds every operation to f32 (float64 in the analysis) and the restatement sums in float64, so they differ
by rounding alone, amplified by the conditioning of Levinson's recursion (analysis) and by the gain of the all-pole recursion over 960 samples
(shape).  Neither factor has a useful closed bound, so the bounds are 8 x the worst deviation observed over every case below
(profiles/formant_parity_observed.jsonl has each case; tools/formant_parity.py writes it from these rows), and never above 1e-4 for a coefficient or 1e-3 of the row's peak for a sample: beyond the
caps the statement or the restatement is wrong, whatever was observed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _formant_ref as F
import _pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
SYMBOLS = ("ptts_formant_frames", "ptts_formant_analyse", "ptts_formant_whiten", "ptts_formant_shape", "ptts_formant_apply", "ptts_formant_rows",
           "ptts_dsp_ext_set_formant")
# the worst deviations observed (the last line of profiles/formant_parity_observed.jsonl): coefficients absolute, samples relative to the row's peak
OBSERVED = {"coeffs": 5.94e-8, "whiten": 2.88e-7, "shape": 6.40e-6}
CAPS = {"coeffs": 1e-4, "whiten": 1e-3, "shape": 1e-3}
BOUND = {k: min(8.0 * v, CAPS[k]) for k, v in OBSERVED.items()}
SHAPE_PITCHES = (800, 1250, 1500)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in SYMBOLS:
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    O = rt.FormantOpts
    assert C.sizeof(O) == 16 and [getattr(O, f).offset for f in ("size", "keep", "reserved")] == [0, 4, 8]
    assert O().size == 16 and O().keep == 1 and O(0).keep == 0
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#define O(f) offsetof(ptts_formant_opts, f)\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_formant_opts), O(size), O(keep), O(reserved), sizeof(((ptts_formant_opts*)0)->reserved));\n'
                   'return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [16, 0, 4, 8, 8]


def test_frames_and_lengths(pkg):
    rt = pkg.runtime
    L = rt.lib()
    assert [rt.formant_frames(n) for n in (0, 1, 240, 241)] == [0, 1, 1, 2] == [F.frames(n) for n in (0, 1, 240, 241)]
    assert all(rt.formant_frames(n) == F.frames(n) for n in F.LENGTHS + (24000, 240001))
    assert L.ptts_formant_frames(-1) == -rt.PTTS_EINVAL and L.ptts_formant_frames(R.LIMIT) == -rt.PTTS_EINVAL
    assert L.ptts_formant_frames(R.LIMIT - 1) == F.frames(R.LIMIT - 1)
    keep = rt.FormantOpts(1)
    for p in (800, 999, 1001, 1250, 1500):
        for s in (None, 800, 1250):
            po, to = rt.PitchOpts(p), None if s is None else rt.TempoOpts(s)
            for n in F.LENGTHS:
                y = rt.formant_apply(keep, po, to, F.noise(n))
                assert y.size == rt.pitch_length(po, to, n) == R.length(n, 1000 if s is None else s, p), (n, p, s)


@pytest.fixture(scope="module")
def parity(pkg):
    """per (row kind, n): the row, the library's coefficients and residual, and per pitch the library's resample of that residual: made once"""
    rt = pkg.runtime
    out = {}
    for n in F.LENGTHS:
        for name, x in F.parity_rows(n).items():
            c = rt.formant_analyse(x)
            e = rt.formant_whiten(c, x)
            er = {p: rt.pitch_resample(rt.PitchOpts(p), e) for p in SHAPE_PITCHES}
            for a in (x, c, e, *er.values()):
                a.setflags(write=False)
            out[(name, n)] = (x, c, e, er)
    return out


def _peak(x):
    fin = np.isfinite(x)
    return max(float(np.abs(x[fin]).max(initial=0.0)), 1e-30)


def _deviation(got, want, scale):
    """the largest |got - want| / scale where the restatement is finite; the two are finite in the same places"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float(np.abs(got.astype(np.float64)[fin] - want[fin]).max(initial=0.0)) / scale


def test_analyse_is_the_numpy_statement(pkg, parity):
    worst = 0.0
    active = 0
    for (name, n), (x, c, e, er) in parity.items():
        assert c.shape == (F.frames(n), F.ORDER) and np.isfinite(c).all()
        want = F.analyse(x)
        d = _deviation(c, want, 1.0)
        print("coeffs", name, n, "%.3e" % d)
        worst = max(worst, d)
        active += int((np.abs(want).sum(1) > 0).sum())
        assert np.array_equal(np.abs(c).sum(1) == 0, np.abs(want).sum(1) == 0), (name, n)          # the same frames are the identity
    print("coeffs worst %.3e bound %.3e" % (worst, BOUND["coeffs"]))
    assert active >= 60 and worst <= BOUND["coeffs"], worst


def test_whiten_is_the_numpy_statement(pkg, parity):
    worst, nans = 0.0, 0
    for (name, n), (x, c, e, er) in parity.items():
        want = F.whiten(c, x)
        d = _deviation(e, want, _peak(x))
        print("whiten", name, n, "%.3e" % d)
        worst = max(worst, d)
        nans += int((~np.isfinite(want)).sum())
    print("whiten worst %.3e bound %.3e" % (worst, BOUND["whiten"]))
    assert nans >= 100 and worst <= BOUND["whiten"], worst


def test_shape_is_the_numpy_statement(pkg, parity):
    rt = pkg.runtime
    worst = 0.0
    for (name, n), (x, c, e, er) in parity.items():
        for p in SHAPE_PITCHES:
            got = rt.formant_shape(c, n, p, er[p])
            want = F.shape(c, n, p, er[p])
            assert got.size == R.resample_length(n, p)
            d = _deviation(got, want, _peak(want))
            print("shape", name, n, p, "%.3e" % d)
            worst = max(worst, d)
    print("shape worst %.3e bound %.3e" % (worst, BOUND["shape"]))
    assert worst <= BOUND["shape"], worst


@pytest.fixture(scope="module")
def vowels():
    out = {}
    for f0, formants in (F.VOWEL_A, F.VOWEL_B):
        x = F.vowel(f0, formants)
        assert x.size == 24000 and abs(float(np.abs(x).max()) - 0.5) < 1e-6
        x.setflags(write=False)
        out[f0] = (x, formants)
    return out


# the float64 prototype's ratios, for the record; the cap on every one of them is 0.7
PROPERTY_CASES = [(120.0, 800, 0.60), (120.0, 1250, 0.40), (160.0, 800, 0.35), (160.0, 1250, 0.16), (160.0, 1500, 0.14)]


@pytest.mark.parametrize("f0,p,prototype", PROPERTY_CASES)
def test_the_pitch_moves_and_the_envelope_stays(pkg, vowels, f0, p, prototype):
    rt = pkg.runtime
    x, formants = vowels[f0]
    ratio = p / 1000.0
    kept_out = rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(p), None, x)
    plain_out = rt.pitch_apply(rt.PitchOpts(p), None, x)
    assert kept_out.size == plain_out.size and np.isfinite(kept_out).all()
    kept, moved = F.envelope_errors(kept_out, f0 * ratio, formants, ratio)
    plain_kept, plain_moved = F.envelope_errors(plain_out, f0 * ratio, formants, ratio)
    hz, plain_hz = F.fundamental(kept_out), F.fundamental(plain_out)
    print("f0 %g p %d: kept %.3f moved %.3f dB; plain: kept %.3f moved %.4f dB; ratio %.3f (prototype %.2f); fundamental %.2f / plain %.2f Hz"
          % (f0, p, kept, moved, plain_kept, plain_moved, kept / plain_kept, prototype, hz, plain_hz))
    assert plain_moved <= 0.1                                              # the measurement itself: the plain pitch moves the envelope exactly
    assert abs(hz / (f0 * ratio) - 1.0) < 0.005 and abs(plain_hz / (f0 * ratio) - 1.0) < 0.005   # the fundamental moves by p / 1000
    assert kept < moved                                                    # with the option the envelope is nearer to its place than to where it would move
    assert kept <= 0.7 * plain_kept


def test_exactness(pkg):
    rt = pkg.runtime
    x = F.noise(4801)
    for to in (None, rt.TempoOpts(800), rt.TempoOpts(1250)):
        for f, po in ((rt.FormantOpts(1), rt.PitchOpts(1000)), (rt.FormantOpts(0), rt.PitchOpts(1250)), (rt.FormantOpts(0), rt.PitchOpts(1000))):
            assert np.array_equal(_u32(rt.formant_apply(f, po, to, x)), _u32(rt.pitch_apply(po, to, x)))           # today's bits
    assert not np.array_equal(rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(1250), None, x), rt.pitch_apply(rt.PitchOpts(1250), None, x))
    # the stage is its steps: analyse, whiten, the pitch's resample, shape, the tempo at E
    for p, s in ((800, None), (1250, 800), (1500, 1250)):
        po, to = rt.PitchOpts(p), None if s is None else rt.TempoOpts(s)
        c = rt.formant_analyse(x)
        z = rt.formant_shape(c, x.size, p, rt.pitch_resample(po, rt.formant_whiten(c, x)))
        E = rt.pitch_speed(po, to)
        want = z if E == 1000 else rt.tempo_apply(rt.TempoOpts(E), z)
        assert np.array_equal(_u32(rt.formant_apply(rt.FormantOpts(1), po, to, x)), _u32(want)), (p, s)
    # silence in, silence out; finite in, finite out
    for n in F.LENGTHS:
        for p in (800, 1250, 1500):
            y = rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(p), None, np.zeros(n, np.float32))
            assert y.size == R.length(n, 1000, p) and (y == 0.0).all(), (n, p)
            for name, x2 in F.parity_rows(n).items():
                if name != "special":
                    assert np.isfinite(rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(p), None, x2)).all(), (name, n, p)


def test_what_a_nan_reaches(pkg):
    rt = pkg.runtime
    n, at = 9600, 5000
    clean = F.noise(n, 21)
    x = clean.copy()
    x[at] = np.nan
    c, c0 = rt.formant_analyse(x), rt.formant_analyse(clean)
    identity = np.flatnonzero(np.abs(c).sum(1) == 0)
    assert identity.tolist() == [19, 20, 21] and (np.abs(c0).sum(1) > 0).all()       # the three frames whose windows hold it
    others = np.setdiff1d(np.arange(c.shape[0]), identity)
    assert np.array_equal(_u32(c[others]), _u32(c0[others]))
    e, e0 = rt.formant_whiten(c, x), rt.formant_whiten(c0, clean)
    assert np.flatnonzero(np.isnan(e)).tolist() == list(range(at, at + 25))           # residual samples 5000 .. 5024 only
    far = np.ones(n, bool)
    far[240 * 18 + 120:240 * 23 + 120] = False                                        # samples whose frame pair holds none of the three
    assert np.array_equal(_u32(e[far]), _u32(e0[far]))
    for p in (800, 1250, 1500):
        po = rt.PitchOpts(p)
        z = rt.formant_shape(c, n, p, rt.pitch_resample(po, e))
        z0 = rt.formant_shape(c0, n, p, rt.pitch_resample(po, e0))
        bad = np.flatnonzero(np.isnan(z))
        image = (at * 1000) // p                                                      # where sample 5000 lies in the resampled row
        support = (80 * max(1000, p)) // (3 * p) + 2                                  # the resampler's support, in outputs
        assert bad.size > 0 and bad.min() >= image - support, (p, bad.min(), image)
        assert bad.max() <= (at + 24) * 1000 // p + support + F.WARM + F.HOP, (p, bad.max(), image)
        # nothing else of the row is touched: beyond the NaN's reach and the three frames' reach the bits are the clean row's
        lo = min(image - support, (240 * 18 + 120) * 1000 // p) - F.HOP
        hi = max((at + 24) * 1000 // p + support, (240 * 23 + 120) * 1000 // p) + F.WARM + 2 * F.HOP
        assert np.array_equal(_u32(z[:lo]), _u32(z0[:lo])) and np.array_equal(_u32(z[hi:]), _u32(z0[hi:])) and z[hi:].size > 100, p


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 16), ("tail", C.c_uint8 * 16)]


def test_refusals_name_the_field(pkg):
    rt = pkg.runtime
    L = rt.lib()
    x = np.zeros(8, np.float32)
    y = np.zeros(16, np.float32)
    ext = rt.DspExt()
    p12 = rt.PitchOpts(1250)
    for keep in (2, -1, 7):
        o = rt.FormantOpts(keep)
        for call in (lambda: rt.formant_apply(o, p12, None, x), lambda: ext.set_formant(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and "keep %d" % keep in str(ei.value), str(ei.value)
    for reserved in ((1, 0), (0, -1)):
        o = rt.FormantOpts(1, reserved=reserved)
        for call in (lambda: rt.formant_apply(o, p12, None, x), lambda: ext.set_formant(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and "reserved" in str(ei.value)
    for o in (rt.FormantOpts(1, size=8), rt.FormantOpts(1, size=0)):
        for call in (lambda: rt.formant_apply(o, p12, None, x), lambda: ext.set_formant(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and "formant: size" in str(ei.value)
    wide = _Wide()                                                        # a larger struct: zeros beyond what the library knows are "off"
    C.memmove(C.byref(wide), C.byref(rt.FormantOpts(1, size=32)), 16)
    as_opts = C.cast(C.byref(wide), C.POINTER(rt.FormantOpts))
    assert L.ptts_formant_apply(as_opts, C.byref(p12), None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_OK
    for at in (0, 15):
        wide.tail[at] = 1
        assert L.ptts_formant_apply(as_opts, C.byref(p12), None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_EINVAL and "size" in L.ptts_last_error().decode()
        wide.tail[at] = 0
    # the range of the pitch with the option: both fields and both values; without the option, and at 1000, every pitch is served as before
    for p in (799, 1501, 500, 2000, 667):
        with pytest.raises(pkg.PttsError) as ei:
            rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(p), None, x)
        msg = str(ei.value)
        assert ei.value.code == rt.PTTS_EINVAL and all(w in msg for w in ("keep 1", "pitch_permille %d" % p, "800", "1500")), msg
        assert np.array_equal(_u32(rt.formant_apply(rt.FormantOpts(0), rt.PitchOpts(p), None, x)), _u32(rt.pitch_apply(rt.PitchOpts(p), None, x)))
    for p in (800, 1500):                                                # the ends of the range are served
        assert rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(p), None, x).size == R.length(8, 1000, p)
    with pytest.raises(pkg.PttsError) as ei:                             # the pitch's and the tempo's own fields are theirs to refuse
        rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(2001), None, x)
    assert "pitch_permille 2001" in str(ei.value) and "500 to 2000" in str(ei.value)
    with pytest.raises(pkg.PttsError) as ei:
        rt.formant_apply(rt.FormantOpts(1), p12, rt.TempoOpts(2001), x)
    assert "speed_permille" in str(ei.value)
    with pytest.raises(pkg.PttsError) as ei:                             # the effective speed names both fields and both values
        rt.formant_apply(rt.FormantOpts(1), rt.PitchOpts(1500), rt.TempoOpts(500), x)
    assert all(w in str(ei.value) for w in ("speed_permille 500", "pitch_permille 1500", "333"))
    # pointers
    f = rt.FormantOpts(1)
    fp, pp = C.byref(f), C.byref(p12)
    assert L.ptts_formant_apply(None, pp, None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_EINVAL and "formant: null options" in L.ptts_last_error().decode()
    assert L.ptts_formant_apply(fp, None, None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_EINVAL and "pitch: null options" in L.ptts_last_error().decode()
    assert L.ptts_formant_apply(fp, pp, None, None, 8, rt._fp(y)) == rt.PTTS_EINVAL and "null argument" in L.ptts_last_error().decode()
    assert L.ptts_formant_apply(fp, pp, None, rt._fp(x), 8, None) == rt.PTTS_EINVAL and "null argument" in L.ptts_last_error().decode()
    assert L.ptts_formant_apply(fp, pp, None, rt._fp(x), 8, rt._fp(x)) == rt.PTTS_EINVAL and "out is in" in L.ptts_last_error().decode()
    assert L.ptts_formant_apply(fp, pp, None, rt._fp(x), -1, rt._fp(y)) == rt.PTTS_EINVAL
    assert L.ptts_formant_apply(fp, pp, None, None, 0, None) == rt.PTTS_OK
    c = np.zeros(24, np.float32)
    assert L.ptts_formant_analyse(None, 8, rt._fp(c)) == rt.PTTS_EINVAL and L.ptts_formant_analyse(rt._fp(x), 8, None) == rt.PTTS_EINVAL
    assert L.ptts_formant_analyse(rt._fp(x), -1, rt._fp(c)) == rt.PTTS_EINVAL and L.ptts_formant_analyse(None, 0, None) == rt.PTTS_OK
    assert L.ptts_formant_whiten(rt._fp(c), rt._fp(x), 8, rt._fp(x)) == rt.PTTS_EINVAL and "e is x" in L.ptts_last_error().decode()
    assert L.ptts_formant_whiten(None, rt._fp(x), 8, rt._fp(y)) == rt.PTTS_EINVAL and "null argument" in L.ptts_last_error().decode()
    e_r = np.zeros(7, np.float32)
    assert L.ptts_formant_shape(rt._fp(c), 8, 1250, rt._fp(e_r), 7, rt._fp(y)) == rt.PTTS_OK
    assert L.ptts_formant_shape(rt._fp(c), 8, 1250, rt._fp(e_r), 6, rt._fp(y)) == rt.PTTS_EINVAL and "n_r 6" in L.ptts_last_error().decode()
    assert L.ptts_formant_shape(rt._fp(c), 8, 1501, rt._fp(e_r), 6, rt._fp(y)) == rt.PTTS_EINVAL and "pitch_permille 1501" in L.ptts_last_error().decode()
    assert L.ptts_formant_shape(rt._fp(c), 8, 1250, rt._fp(e_r), 7, rt._fp(e_r)) == rt.PTTS_EINVAL and "out is e_r" in L.ptts_last_error().decode()
    assert L.ptts_formant_shape(rt._fp(c), 8, 1250, None, 7, rt._fp(y)) == rt.PTTS_EINVAL and "null argument" in L.ptts_last_error().decode()
    ext.free()


def test_the_setter_wants_a_live_handle(pkg):
    rt = pkg.runtime
    L = rt.lib()
    o = rt.FormantOpts(1)
    ext = rt.DspExt(pitch=rt.PitchOpts(1100), formant=o)
    d = rt.DspOpts()
    d.ext = ext.h
    assert rt.dsp_opts_error(d) == ""                            # the options themselves are well formed; who may serve them is the entry point's to say
    ext.set_formant(None)
    ext.set_formant(o)
    alone = rt.DspExt(formant=o)                                 # without a pitch the option says nothing, and nothing refuses it
    d2 = rt.DspOpts()
    d2.ext = alone.h
    assert rt.dsp_opts_error(d2) == ""
    alone.free()
    h = ext.h
    ext.free()
    for dead in (h, None, 7):
        for p in (C.byref(o), None):
            rc = L.ptts_dsp_ext_set_formant(C.c_void_p(dead), p)
            msg = L.ptts_last_error().decode(errors="replace")
            assert rc == rt.PTTS_EINVAL and msg.startswith("ptts-hip: formant: ext") and "not a live handle" in msg, (dead, msg)
    with pytest.raises(pkg.PttsError) as ei:                     # the options are checked where the handle is made, and nothing leaks a handle
        rt.DspExt(formant=rt.FormantOpts(3))
    assert "keep 3" in str(ei.value)


SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "formant.h"
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

static ptts_formant_opts keep(int k) {
    ptts_formant_opts f;
    std::memset(&f, 0, sizeof f);
    f.size = sizeof f; f.keep = k;
    return f;
}
static ptts_pitch_opts pitch(int p) {
    ptts_pitch_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = sizeof o; o.pitch_permille = p;
    return o;
}
static ptts_tempo_opts tempo(int speed) {
    ptts_tempo_opts t;
    std::memset(&t, 0, sizeof t);
    t.size = sizeof t; t.speed_permille = speed;
    return t;
}
static float* block(long n) { return static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1)); }

// rows, coefficients and outputs in blocks of exactly their size: a read or a write one element too far is reported
static int rows() {
    const long sizes[10] = {0, 1, 2, 119, 121, 240, 241, 719, 721, 4801};
    const int pitches[6] = {800, 999, 1000, 1001, 1250, 1500};
    const int speeds[3] = {0, 800, 1250};   // 0: no tempo
    const ptts_formant_opts f = keep(1);
    for (int pv : pitches) {
        const ptts_pitch_opts p = pitch(pv);
        for (int speed : speeds) {
            const ptts_tempo_opts t = tempo(speed ? speed : 1000);
            const ptts_tempo_opts* tp = speed ? &t : nullptr;
            const int E = ptts_pitch_speed(&p, tp);
            CHECK(E >= 500 && E <= 2000);
            for (long n : sizes) {
                for (int pattern = 0; pattern < 3; pattern++) {   // zeros; a tone above full scale; a sawtooth with a NaN and an infinity
                    const long K = ptts_formant_frames(n), n_r = (long)ptts_pitch_resample_length(&p, n), n_f = (long)ptts_pitch_length(&p, tp, n);
                    CHECK(K == (n + 239) / 240);
                    float *x = block(n), *c = block(K * 24), *e = block(n), *er = block(n_r), *z = block(n_r), *y = block(n_f), *w = block(n_f);
                    CHECK(x && c && e && er && z && y && w);
                    for (long i = 0; i < n; i++) x[i] = pattern == 0 ? 0.0f : pattern == 1 ? 1.5f * std::sin(0.05f * (float)i) : (float)(i % 97) / 97.0f - 0.5f;
                    if (pattern == 2 && n > 300) { x[7] = NAN; x[300] = INFINITY; }
                    CHECK(ptts_formant_apply(&f, &p, tp, n ? x : nullptr, n, n_f ? y : nullptr) == PTTS_OK);
                    if (pv != 1000) {   // the stage is its steps
                        CHECK(ptts_formant_analyse(n ? x : nullptr, n, n ? c : nullptr) == PTTS_OK);
                        CHECK(ptts_formant_whiten(c, x, n, e) == PTTS_OK);
                        CHECK(ptts_pitch_resample(&p, n ? e : nullptr, n, n_r ? er : nullptr) == PTTS_OK);
                        CHECK(ptts_formant_shape(c, n, pv, er, n_r, z) == PTTS_OK);
                        const ptts_tempo_opts te = tempo(E);
                        CHECK(ptts_tempo_apply(&te, n_r ? z : nullptr, n_r, n_f ? w : nullptr) == PTTS_OK);
                        if (pattern < 2) CHECK(n_f == 0 || std::memcmp(y, w, (size_t)n_f * sizeof(float)) == 0);
                        if (pattern == 0) for (long i = 0; i < n_r; i++) CHECK(z[i] == 0.0f);
                        if (pattern == 1) for (long i = 0; i < n_r; i++) CHECK(std::isfinite(z[i]));
                    } else {
                        CHECK(ptts_pitch_apply(&p, tp, n ? x : nullptr, n, n_f ? w : nullptr) == PTTS_OK);
                        CHECK(n_f == 0 || pattern == 2 || std::memcmp(y, w, (size_t)n_f * sizeof(float)) == 0);
                    }
                    std::free(x); std::free(c); std::free(e); std::free(er); std::free(z); std::free(y); std::free(w);
                }
            }
        }
    }
    return 0;
}

static int refusals() {
    float x[8] = {0}, y[16];
    ptts_formant_opts f = keep(1);
    ptts_pitch_opts p = pitch(1250);
    CHECK(ptts_formant_apply(&f, &p, nullptr, nullptr, 4, y) == PTTS_EINVAL && has(g_err, "null"));
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, x) == PTTS_EINVAL && has(g_err, "out is in"));
    CHECK(ptts_formant_apply(nullptr, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "formant: null options"));
    CHECK(ptts_formant_apply(&f, nullptr, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "pitch: null options"));
    f = keep(2);
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "keep 2"));
    f = keep(1);
    f.reserved[1] = 3;
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "reserved"));
    f = keep(1);
    f.size = 8;
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "size"));
    f = keep(1);
    p = pitch(799);
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "keep 1") && has(g_err, "pitch_permille 799"));
    p = pitch(1501);
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_EINVAL && has(g_err, "pitch_permille 1501"));
    f = keep(0);
    CHECK(ptts_formant_apply(&f, &p, nullptr, x, 8, y) == PTTS_OK);
    CHECK(ptts_formant_frames(-1) == -PTTS_EINVAL && ptts_formant_frames(0) == 0 && ptts_formant_frames(241) == 2);
    const double* t = formant_tables();
    CHECK(t[kFormantWin] == 1.0001 && t[kFormantWin + kFormantOrder + 1] == 1.0 && t[0] > 0.0 && t[0] == t[kFormantWin - 1]);
    CHECK(formant_pair(0, 5).fa == 0 && formant_pair(0, 5).fb == 0 && formant_pair(120, 5).fb == 1 && formant_pair(120, 5).u == 0.0f && formant_pair(5000, 5).fa == 4);
    return 0;
}

int main() {
    if (rows() || refusals()) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/formant.cpp, csrc/pitch.cpp and csrc/tempo.cpp alone, built with g++ -fsanitize=address,undefined and run as a
    subprocess.  Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "formant_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "formant_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), os.path.join(CSRC, "formant.cpp"), os.path.join(CSRC, "pitch.cpp"), os.path.join(CSRC, "tempo.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
