"""CPU-side checks of the de-esser (include/ptts.h ptts_deesser_opts, ptts_deess_*, ptts_dsp_ext_set_deesser; go-pocket-tts_amd/csrc/deesser.{h,cpp};
DESIGN.md section 8, N3): the struct's layout; refusals that name their field; the band against the equaliser of one high-pass section, bit for
bit; rows the stage must hand back bit for bit; engagement inside sibilant bursts only; the floor; ptts_deess_apply -- the blocked form the
kernels run -- against the sample-by-sample statement of _deesser_ref.py within the margin tests/test_compressor_cpu.py grants the compressor for
the same comparison (_eq_ref.bound: one f32 step at the row's peak); the non-finite cases as documented; and a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _deesser_ref as R
import _eq_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
N = max(R.LENGTHS)
FIELDS = ("freq_hz", "q", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "max_reduction_db")
SIZE = 72


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _opts(rt, design, **kw):
    return rt.DeesserOpts(*design, **kw)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in ("ptts_dsp_ext_set_deesser", "ptts_deess_apply", "ptts_deess_band", "ptts_deess_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    assert C.sizeof(rt.DeesserOpts) == SIZE and rt.DeesserOpts.freq_hz.offset == 8 and rt.DeesserOpts.max_reduction_db.offset == 64
    assert rt.DeesserOpts().size == SIZE
    assert [f for f, _ in rt.DeesserOpts._fields_[2:]] == list(FIELDS)
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ptts_deesser_opts), '
                   'offsetof(ptts_deesser_opts, freq_hz), offsetof(ptts_deesser_opts, threshold_db), offsetof(ptts_deesser_opts, max_reduction_db)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [SIZE, 8, 24, 64]


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * SIZE), ("tail", C.c_uint8 * 16)]


def _apply_raw(rt, buf):
    L = rt.lib()
    x = np.zeros(8, np.float32)
    rc = L.ptts_deess_apply(C.cast(C.byref(buf), C.POINTER(rt.DeesserOpts)), x.ctypes.data_as(C.POINTER(C.c_float)), x.size)
    return rc, L.ptts_last_error().decode(errors="replace")


def test_refusals_name_the_field(pkg):
    rt = pkg.runtime
    nan, inf = float("nan"), float("inf")
    good = dict(zip(FIELDS, R.DESIGNS["soft"]))
    box = dict(freq_hz=(2000.0, 10000.0), q=(0.3, 4.0), threshold_db=(-60.0, 0.0), ratio=(1.0, 100.0), knee_db=(0.0, 24.0), attack_ms=(0.05, 200.0),
               release_ms=(5.0, 5000.0), max_reduction_db=(0.0, 40.0))
    x = np.zeros(8, np.float32)
    ext = rt.DspExt()
    for field, (lo, hi) in box.items():
        for v in (np.nextafter(lo, -inf), np.nextafter(hi, inf), nan, inf, -inf):
            o = rt.DeesserOpts(**dict(good, **{field: v}))
            for call in (lambda: rt.deess_apply(o, x), lambda: rt.deess_band(o, x), lambda: ext.set_deesser(o)):
                with pytest.raises(pkg.PttsError) as ei:
                    call()
                assert ei.value.code == rt.PTTS_EINVAL and "deesser" in str(ei.value) and field in str(ei.value), (field, v, str(ei.value))
        for v in (lo, hi):   # every edge of the box is inside it
            assert rt.deess_apply(rt.DeesserOpts(**dict(good, **{field: v})), x).shape == (8,)
    # size below the struct (every field is required), reserved
    for o, field in [(rt.DeesserOpts(size=SIZE - 8), "size"), (rt.DeesserOpts(size=0), "size"), (rt.DeesserOpts(reserved=1), "reserved")]:
        for call in (lambda: rt.deess_apply(o, x), lambda: rt.deess_band(o, x), lambda: ext.set_deesser(o)):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value), (field, str(ei.value))
    # size above it: zeros beyond what the library knows are "off", anything else is refused
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.DeesserOpts(size=SIZE + 16)), SIZE)
    rc, msg = _apply_raw(rt, wide)
    assert rc == rt.PTTS_OK, msg
    for at in (0, 15):
        wide.tail[at] = 1
        rc, msg = _apply_raw(rt, wide)
        assert rc == rt.PTTS_EINVAL and "size" in msg, (at, msg)
        wide.tail[at] = 0
    # null options and null samples
    L = rt.lib()
    assert L.ptts_deess_apply(None, None, 0) == rt.PTTS_EINVAL and "null options" in L.ptts_last_error().decode()
    assert L.ptts_deess_apply(C.byref(rt.DeesserOpts()), None, 4) == rt.PTTS_EINVAL and "null samples" in L.ptts_last_error().decode()
    ext.free()


def test_the_setter_wants_a_live_handle(pkg):
    rt = pkg.runtime
    L = rt.lib()
    o = rt.DeesserOpts()
    ext = rt.DspExt(deesser=o)
    d = rt.DspOpts()
    d.ext = ext.h
    assert rt.dsp_opts_error(d) == ""
    ext.set_deesser(None)
    assert rt.dsp_opts_error(d) == ""
    ext.set_deesser(o)
    h = ext.h
    ext.free()
    eq = rt.Eq(E.CASCADES["s1"])                                 # an equaliser is no ptts_dsp_ext
    for dead in (h, eq.h, None, 7):
        for c in (C.byref(o), None):
            rc = L.ptts_dsp_ext_set_deesser(C.c_void_p(dead), c)
            msg = L.ptts_last_error().decode(errors="replace")
            assert rc == rt.PTTS_EINVAL and "deesser" in msg and "not a live handle" in msg, (dead, msg)
    eq.free()
    with pytest.raises(pkg.PttsError) as ei:                     # the options are checked where the handle is made
        rt.DspExt(deesser=rt.DeesserOpts(q=0.1))
    assert "q" in str(ei.value)
    assert rt._dsp_opts(pkg.RuntimeGenerateConfig()) is None and rt._dsp_opts(pkg.RuntimeGenerateConfig(deesser=o)).ext


@pytest.fixture(scope="module")
def sib():
    x = R.engagement(N)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_band_is_the_equaliser_of_one_highpass_section(pkg, sib, name):
    rt = pkg.runtime
    design = R.DESIGNS[name]
    o = _opts(rt, design)
    eq = rt.Eq([(E.HIGHPASS, design[0], 0.0, design[1])])
    for x in (sib, E.signal(N, seed=31)):
        for n in R.LENGTHS:
            got, want = rt.deess_band(o, x[:n]), eq.apply(x[:n])
            assert got.dtype == np.float32 and got.shape == (n,) and np.array_equal(_u32(got), _u32(want)), (name, n)
    assert float(np.abs(rt.deess_band(o, sib)).max()) > 0.1      # the band is there
    eq.free()


def test_a_low_tone_passes_bit_for_bit(pkg):
    rt = pkg.runtime
    t = np.arange(N) / E.RATE
    x = (0.5 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    o = rt.DeesserOpts(freq_hz=5000.0, threshold_db=-30.0)
    assert np.array_equal(_u32(rt.deess_apply(o, x)), _u32(x))


def test_ratio_one_passes_bit_for_bit(pkg, sib):
    rt = pkg.runtime
    for name, design in R.DESIGNS.items():
        for knee in (0.0, 6.0):
            o = rt.DeesserOpts(**dict(zip(FIELDS, design), ratio=1.0, knee_db=knee))
            assert np.array_equal(_u32(rt.deess_apply(o, sib)), _u32(sib)), (name, knee)
        o = rt.DeesserOpts(**dict(zip(FIELDS, design), max_reduction_db=0.0))        # a floor of 0 dB does nothing either
        assert np.array_equal(_u32(rt.deess_apply(o, sib)), _u32(sib)), name
    y = np.array(sib)                                                                  # ... whatever the row holds
    y[100], y[2000] = np.nan, np.inf
    o = rt.DeesserOpts(ratio=1.0)
    assert np.array_equal(_u32(rt.deess_apply(o, y)), _u32(y))


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_it_engages_inside_the_bursts_only(pkg, sib, name):
    rt = pkg.runtime
    y = rt.deess_apply(_opts(rt, R.DESIGNS[name]), sib)
    inside = R.in_burst(N)
    changed = _u32(y) != _u32(sib)
    before = np.arange(N) < R.BURST_AT
    assert before.sum() == R.BURST_AT and inside.sum() == 2 * R.BURST_LEN
    assert not changed[before].any()                             # the stretch before the first burst: bit-identical
    assert changed[inside].mean() > 0.9                          # inside the bursts the samples change
    # only the band is turned down: the tone under the bursts keeps its level (what y - x holds under 1 kHz is the high-pass's stop band,
    # more than 24 dB down at either design's corner, times a gain change under 1)
    rms = lambda a: float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))  # noqa: E731
    low = rt.Eq([(E.LOWPASS, 1000.0, 0.0, 0.7071)])
    assert abs(rms(low.apply(y)[inside]) / rms(low.apply(sib)[inside]) - 1.0) < 0.01
    low.free()


def test_the_floor_holds_the_reduction(pkg):
    """A steady 7 kHz tone at 0.5, threshold -40 dB, ratio 100, at most 6 dB: the curve asks for far more than 6 dB, so once the level has
    settled every sample is x + (g - 1) b with g the floor's gain through the library's exp2 (restated in float64), rounded once."""
    rt = pkg.runtime
    n = 9600
    t = np.arange(n) / E.RATE
    x = (0.5 * np.sin(2 * np.pi * 7000.0 * t)).astype(np.float32)
    o = rt.DeesserOpts(freq_hz=5000.0, q=0.7071, threshold_db=-40.0, ratio=100.0, knee_db=6.0, attack_ms=1.0, release_ms=60.0, max_reduction_db=6.0)
    y, b = rt.deess_apply(o, x), rt.deess_band(o, x)
    g = R.lib_exp2((0.0 - 6.0) * R.LOG2_PER_DB)
    assert abs(20.0 * np.log10(g) + 6.0) < 1e-9
    want = (x.astype(np.float64) + (g - 1.0) * b.astype(np.float64)).astype(np.float32)
    settled = slice(n // 2, n)
    assert np.array_equal(_u32(y[settled]), _u32(want[settled]))
    assert float(np.abs(y[settled].astype(np.float64) - x[settled]).max()) > 0.1      # and that is a change one hears
    assert not np.array_equal(_u32(y[:48]), _u32(want[:48]))                          # the attack is not at the floor yet


@pytest.fixture(scope="module")
def refs(sib):
    """design name -> the sample-by-sample statement over the longest length: computed once, never written to"""
    out = {name: R.apply(sib, d) for name, d in R.DESIGNS.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_apply_is_the_sample_by_sample_statement_within_one_step(pkg, sib, refs, name):
    """The margin is the one tests/test_compressor_cpu.py grants the compressor's blocked form against its statement: _eq_ref.bound, one f32
    step at the row's peak (test_apply_is_the_sample_by_sample_statement_within_one_step there)."""
    rt = pkg.runtime
    ref = refs[name]
    o = _opts(rt, R.DESIGNS[name])
    moved = float(np.abs(ref.astype(np.float64) - sib).max())
    deepest = float(R.gain_db(sib, R.DESIGNS[name]).min())
    print(f"{name}: moved {moved:.3e} = {moved / E.bound(ref):.0f} bounds, deepest gain {deepest:.2f} dB")
    assert moved > 1000.0 * E.bound(ref) and deepest < -6.0, (moved, deepest)
    for n in R.LENGTHS:
        got = rt.deess_apply(o, sib[:n])
        assert got.dtype == np.float32 and got.shape == (n,)
        if n == 0:
            continue
        err = float(np.abs(got.astype(np.float64) - ref[:n]).max())
        diff = int((_u32(got) != _u32(ref[:n])).sum())
        print(f"{name} n={n}: max err {err:.3e} (bound {E.bound(ref[:n]):.3e}), {diff} samples differ")
        assert err <= E.bound(ref[:n]), (name, n, err)


def test_state_crosses_tile_boundaries(pkg, sib):
    """A row cut at a tile boundary inside a burst and started afresh gives other bits: all three states are carried."""
    rt = pkg.runtime
    o = _opts(rt, R.DESIGNS["soft"])
    whole, tail = rt.deess_apply(o, sib), rt.deess_apply(o, sib[R.TILE:])
    assert R.in_burst(N)[R.TILE] and not np.array_equal(_u32(whole[R.TILE:R.TILE + 60]), _u32(tail[:60]))


def test_non_finite_samples_do_what_the_header_says(pkg, sib):
    rt = pkg.runtime
    o = _opts(rt, R.DESIGNS["soft"])
    clean = rt.deess_apply(o, sib)
    at = R.BURST_AT + 700                                        # inside the first burst, where the gain is not 0 dB
    y = np.array(sib)
    y[at] = np.nan
    got = rt.deess_apply(o, y)
    assert np.array_equal(_u32(got[:at]), _u32(clean[:at]))      # samples in front are untouched
    assert np.isnan(got[at:at + 200]).all()                      # the band is NaN from there on, and the gain is not 0 dB yet
    quiet = slice(R.BURST_AT + R.BURST_EVERY - 500, R.BURST_AT + R.BURST_EVERY - 100)
    assert np.array_equal(_u32(got[quiet]), _u32(y[quiet]))      # the level has decayed under the knee: x bit for bit
    assert np.array_equal(_u32(got[-2000:]), _u32(y[-2000:]))    # ... and a NaN level never wins again
    y = np.array(sib)
    y[at] = np.inf
    got = rt.deess_apply(o, y)
    assert np.array_equal(_u32(got[:at]), _u32(clean[:at])) and not np.isfinite(got[at:]).any()


SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "dsp_ext.h"
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

static ptts_deesser_opts opts() {
    ptts_deesser_opts d;
    std::memset(&d, 0, sizeof d);
    d.size = sizeof d; d.freq_hz = 5000.0; d.q = 0.7071; d.threshold_db = -40.0; d.ratio = 8.0; d.knee_db = 6.0; d.attack_ms = 0.5; d.release_ms = 40.0;
    d.max_reduction_db = 18.0;
    return d;
}

// rows in blocks of exactly their size: a read or a write one sample too far is reported
int main() {
    const ptts_deesser_opts d = opts();
    const long sizes[8] = {0, 1, 29, 30, 1919, 1920, 1921, 5 * 1920 + 77};
    for (long n : sizes) {
        float* x = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
        float* keep = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
        float* band = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
        CHECK(x && keep && band);
        for (long i = 0; i < n; i++) keep[i] = x[i] = 0.3f * (float)std::sin(0.05 * (double)i) + 0.4f * (float)std::sin(1.9 * (double)i);
        CHECK(ptts_deess_band(&d, n ? x : nullptr, n, n ? band : nullptr) == PTTS_OK);
        CHECK(ptts_deess_apply(&d, n ? x : nullptr, n) == PTTS_OK);
        bool moved = false;
        for (long i = 0; i < n; i++) { CHECK(std::isfinite(x[i]) && std::isfinite(band[i])); moved = moved || x[i] != keep[i]; }
        CHECK(moved == (n >= 29));                                 // the 7.3 kHz tone at 0.4 lies far above -40 dB in the band
        CHECK(ptts_deess_band(&d, keep, n, keep) == PTTS_OK);      // in place
        CHECK(n == 0 || std::memcmp(keep, band, (size_t)n * sizeof(float)) == 0);
        std::free(x);
        std::free(keep);
        std::free(band);
    }
    CHECK(ptts_deess_apply(&d, nullptr, 4) == PTTS_EINVAL && has(g_err, "null samples"));
    CHECK(ptts_deess_apply(&d, nullptr, -1) == PTTS_EINVAL);
    CHECK(ptts_deess_apply(nullptr, nullptr, 0) == PTTS_EINVAL && has(g_err, "null options"));
    ptts_deesser_opts bad = d;
    bad.freq_hz = 100.0;
    CHECK(ptts_deess_apply(&bad, nullptr, 0) == PTTS_EINVAL && has(g_err, "freq_hz"));
    // a handle that is not live is refused unread; a compressor's setter likewise (compressor.cpp is in the program)
    CHECK(ptts_dsp_ext_set_deesser(nullptr, &d) == PTTS_EINVAL && has(g_err, "not a live handle"));
    CHECK(ptts_dsp_ext_set_deesser(reinterpret_cast<ptts_dsp_ext*>(&bad), nullptr) == PTTS_EINVAL && has(g_err, "not a live handle"));
    CHECK(ptts_dsp_ext_set_compressor(nullptr, nullptr) == PTTS_EINVAL);
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/deesser.cpp, eq.cpp and compressor.cpp, built with g++ -fsanitize=address,undefined and run as a
    subprocess over the lengths above.  Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "deesser_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "deesser_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main)] + [os.path.join(CSRC, f) for f in ("deesser.cpp", "eq.cpp", "compressor.cpp")] + ["-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
