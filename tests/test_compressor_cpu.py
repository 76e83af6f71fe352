"""CPU-side checks of the dynamic range compressor (include/ptts.h ptts_compressor_opts, ptts_compress_*, ptts_dsp_ext_set_compressor;
go-pocket-tts_amd/csrc/compressor.{h,cpp}): the struct's layout; refusals that name their field; the static curve
through the library's own log2 and exp2 against numpy's to the 2^-30 relative gain condition; ptts_compress_apply -- the blocked form the
kernels run -- against the sample-by-sample statement of _compressor_ref.py within one f32 step at the row's peak; state carried over tile
boundaries; a NaN that stays where it is; and a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _compressor_ref as R
import _eq_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
N = max(R.LENGTHS)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _opts(rt, design, **kw):
    return rt.CompressorOpts(*design, **kw)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in ("ptts_dsp_ext_set_compressor", "ptts_compress_gain", "ptts_compress_apply", "ptts_compress_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    assert C.sizeof(rt.CompressorOpts) == 56 and rt.CompressorOpts.threshold_db.offset == 8 and rt.CompressorOpts.makeup_db.offset == 48
    assert C.sizeof(rt.DspExtOpts) == 16
    assert rt.CompressorOpts().size == 56
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ptts_compressor_opts), '
                   'offsetof(ptts_compressor_opts, threshold_db), offsetof(ptts_compressor_opts, makeup_db), sizeof(ptts_dsp_ext_opts)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [56, 8, 48, 16]
    if shutil.which("g++"):
        cpp = tmp_path / "t.cpp"
        cpp.write_text(src.read_text())
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)])
        assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [56, 8, 48, 16]


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 56), ("tail", C.c_uint8 * 16)]


def _gain_raw(rt, buf):
    L = rt.lib()
    out = C.c_double(7.0)
    rc = L.ptts_compress_gain(C.cast(C.byref(buf), C.POINTER(rt.CompressorOpts)), -10.0, C.byref(out))
    return rc, L.ptts_last_error().decode(errors="replace")


def test_refusals_name_the_field(pkg):
    rt = pkg.runtime
    nan, inf = float("nan"), float("inf")
    good = dict(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0, makeup_db=0.0)
    bad = [("threshold_db", (-60.5, 0.5, nan, -inf)), ("ratio", (0.99, 100.5, nan, inf)), ("knee_db", (-0.1, 24.5, nan)),
           ("attack_ms", (0.04, 200.5, nan, 0.0)), ("release_ms", (4.9, 5000.5, nan)), ("makeup_db", (-24.5, 24.5, nan, inf))]
    x = np.zeros(8, np.float32)
    ext = rt.DspExt()
    for field, values in bad:
        for v in values:
            o = rt.CompressorOpts(**dict(good, **{field: v}))
            for call in (lambda: rt.compress_gain(o, -10.0), lambda: rt.compress_apply(o, x), lambda: ext.set_compressor(o)):
                with pytest.raises(pkg.PttsError) as ei:
                    call()
                assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value), (field, v, str(ei.value))
    for o, field in [(rt.CompressorOpts(size=48), "size"), (rt.CompressorOpts(size=0), "size"), (rt.CompressorOpts(reserved=1), "reserved")]:
        with pytest.raises(pkg.PttsError) as ei:
            rt.compress_gain(o, -10.0)
        assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value), (field, str(ei.value))
    with pytest.raises(pkg.PttsError) as ei:
        rt.compress_gain(rt.CompressorOpts(), nan)
    assert "level_db" in str(ei.value)
    # every edge of the box is inside it
    for field, lo, hi in [("threshold_db", -60.0, 0.0), ("ratio", 1.0, 100.0), ("knee_db", 0.0, 24.0), ("attack_ms", 0.05, 200.0),
                          ("release_ms", 5.0, 5000.0), ("makeup_db", -24.0, 24.0)]:
        for v in (lo, hi):
            assert math.isfinite(rt.compress_gain(rt.CompressorOpts(**dict(good, **{field: v})), -10.0))
    # a larger struct: zeros beyond what the library knows are "off", anything else is refused
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.CompressorOpts(size=72)), 56)
    rc, msg = _gain_raw(rt, wide)
    assert rc == rt.PTTS_OK, msg
    for at in (0, 15):
        wide.tail[at] = 1
        rc, msg = _gain_raw(rt, wide)
        assert rc == rt.PTTS_EINVAL and "size" in msg, (at, msg)
        wide.tail[at] = 0
    ext.free()


def test_the_setter_wants_a_live_handle(pkg):
    rt = pkg.runtime
    L = rt.lib()
    o = rt.CompressorOpts()
    ext = rt.DspExt(true_peak_dbtp=-1.0, compressor=o)
    d = rt.DspOpts()
    d.ext = ext.h
    assert rt.dsp_opts_error(d) == ""
    ext.set_compressor(None)                                     # accepted; that nothing is on again is the sanitizer program's to assert (dsp_resolve, dsp_active)
    assert rt.dsp_opts_error(d) == ""
    ext.set_compressor(o)
    h = ext.h
    ext.free()
    eq = rt.Eq(E.CASCADES["s1"])                                 # an equaliser is no ptts_dsp_ext
    for dead in (h, eq.h, None, 7):
        for c in (C.byref(o), None):
            rc = L.ptts_dsp_ext_set_compressor(C.c_void_p(dead), c)
            msg = L.ptts_last_error().decode(errors="replace")
            assert rc == rt.PTTS_EINVAL and "ext" in msg and "not a live handle" in msg, (dead, msg)
    eq.free()
    with pytest.raises(pkg.PttsError) as ei:                     # the options are checked where the handle is made, and nothing leaks a handle
        rt.DspExt(compressor=rt.CompressorOpts(ratio=0.5))
    assert "ratio" in str(ei.value)


@pytest.mark.parametrize("name", ["hard", "knee6", "ratio100"])
def test_curve_is_the_libm_curve_to_the_gain_condition(pkg, name):
    """The linear gain agrees with 10^(curve / 20) to 2^-30 relative, which in dB is 20 log10(1 + 2^-30)."""
    rt = pkg.runtime
    design = R.DESIGNS[name]
    o = _opts(rt, design)
    levels = np.round(np.arange(-9000, 1) * 0.01, 2)
    got = np.array([rt.compress_gain(o, float(v)) for v in levels])
    ref = R.curve_db(levels, design[0], design[1], design[2], design[5])
    bound = 20.0 * math.log10(1.0 + 2.0 ** -30)
    err = float(np.abs(got - ref).max())
    print(f"curve {name}: max |gain_db - ref| = {err:.3e} dB (bound {bound:.3e}); deepest gain {ref.min():.2f} dB")
    assert ref.min() < -10.0 and err <= bound, (name, err, bound)


@pytest.fixture(scope="module")
def cases():
    """input name -> (x, the reference over the longest length): computed once, never written to"""
    out = {}
    for name, x in (("signal", E.signal(N, seed=31)), ("burst", R.burst(N))):
        ref = R.apply(x, R.DESIGNS["knee6"])
        for a in (x, ref):
            a.setflags(write=False)
        out[name] = (x, ref)
    return out


@pytest.mark.parametrize("name", ["signal", "burst"])
def test_apply_is_the_sample_by_sample_statement_within_one_step(pkg, cases, name):
    rt = pkg.runtime
    x, ref = cases[name]
    design = R.DESIGNS["knee6"]
    o = _opts(rt, design)
    bound = E.bound(ref)
    # the stage bites: it moves the audio far above the bound, and its deepest gain is under -6 dB
    moved = float(np.abs(ref.astype(np.float64) - x).max())
    deepest = float(R.gain_db(x, design).min())
    print(f"{name}: moved {moved:.3e} = {moved / bound:.0f} bounds, deepest gain {deepest:.2f} dB")
    assert moved > 1000.0 * bound and deepest < -6.0, (moved, bound, deepest)
    for n in R.LENGTHS:
        got = rt.compress_apply(o, x[:n])
        assert got.dtype == np.float32 and got.shape == (n,)
        if n == 0:
            continue
        err = float(np.abs(got.astype(np.float64) - ref[:n]).max())
        diff = int((_u32(got) != _u32(ref[:n])).sum())
        print(f"{name} n={n}: max err {err:.3e} (bound {E.bound(ref[:n]):.3e}), {diff} samples differ")
        assert err <= E.bound(ref[:n]), (name, n, err)
    # the other designs at the longest length
    for other in ("hard", "ratio100"):
        r2 = R.apply(x, R.DESIGNS[other])
        got = rt.compress_apply(_opts(rt, R.DESIGNS[other]), x)
        assert float(np.abs(got.astype(np.float64) - r2).max()) <= E.bound(r2), other


def test_state_crosses_two_tile_boundaries(pkg):
    rt = pkg.runtime
    o = _opts(rt, R.DESIGNS["knee6"])   # release 120 ms: 3840 samples are 160 ms
    n = 3 * 1920 + 7
    t = np.arange(n) / 24000.0
    x = (0.02 * np.sin(2 * np.pi * 300.0 * t)).astype(np.float32)
    x[:1920] = (0.9 * np.sin(2 * np.pi * 300.0 * t[:1920])).astype(np.float32)   # the burst lies in tile 0
    whole, tail = rt.compress_apply(o, x), rt.compress_apply(o, x[3840:])
    ref = R.apply(x, R.DESIGNS["knee6"])
    assert float(np.abs(whole.astype(np.float64) - ref).max()) <= E.bound(ref)
    assert float(np.abs(tail).max()) > 2.0 * float(np.abs(whole[3840:]).max())    # the burst is still heard in tile 2: its level came through two carries
    assert (_u32(whole[3840:]) != _u32(tail)).any()


def test_a_nan_stays_where_it_is(pkg):
    rt = pkg.runtime
    o = _opts(rt, R.DESIGNS["knee6"])
    x = E.signal(3841, seed=3)
    clean = rt.compress_apply(o, x)
    y = x.copy()
    y[1930] = np.nan
    got = rt.compress_apply(o, y)
    assert np.isnan(got[1930]) and int(np.isnan(got).sum()) == 1
    keep = np.arange(3841) != 1930
    # the detector skipped one sample: at most the release's decay over that sample is missing from the level, and mostly nothing is
    assert (_u32(got[keep][:1930]) == _u32(clean[:1930])).all()
    assert float(np.abs(got[keep].astype(np.float64) - clean[keep]).max()) <= 0.01 * float(np.abs(clean).max())


SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "dsp_spec.h"
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

static ptts_compressor_opts opts() {
    ptts_compressor_opts c;
    std::memset(&c, 0, sizeof c);
    c.size = sizeof c; c.threshold_db = -24.0; c.ratio = 4.0; c.knee_db = 6.0; c.attack_ms = 5.0; c.release_ms = 120.0; c.makeup_db = 3.0;
    return c;
}

// rows in blocks of exactly their size: a read or a write one sample too far is reported
static int rows() {
    const ptts_compressor_opts c = opts();
    const long sizes[4] = {0, 1, 31, 1921};
    for (long n : sizes) {
        float* x = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
        float* keep = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
        CHECK(x && keep);
        for (long i = 0; i < n; i++) keep[i] = x[i] = 0.7f * (float)std::cos(0.05 * (double)i);
        CHECK(ptts_compress_apply(&c, n ? x : nullptr, n) == PTTS_OK);
        bool moved = false;
        for (long i = 0; i < n; i++) { CHECK(std::isfinite(x[i])); moved = moved || x[i] != keep[i]; }
        CHECK(moved == (n > 0));                                   // 3 dB of makeup gain alone moves every non-zero sample
        std::free(x);
        std::free(keep);
    }
    CHECK(ptts_compress_apply(&c, nullptr, 4) == PTTS_EINVAL && has(g_err, "null samples"));
    CHECK(ptts_compress_apply(&c, nullptr, -1) == PTTS_EINVAL);
    CHECK(ptts_compress_apply(nullptr, nullptr, 0) == PTTS_EINVAL && has(g_err, "null options"));
    double g = 0.0;
    CHECK(ptts_compress_gain(&c, -90.0, &g) == PTTS_OK && std::fabs(g - 3.0) < 1e-9);
    CHECK(ptts_compress_gain(&c, 0.0, &g) == PTTS_OK && std::fabs(g - (3.0 - 0.75 * 24.0)) < 1e-8);
    CHECK(ptts_compress_gain(&c, 0.0, nullptr) == PTTS_EINVAL);
    return 0;
}

// set, clear and free on the registry: a handle's memory is read only while the registry holds it
static int handles() {
    const ptts_compressor_opts c = opts();
    ptts_dsp_ext_opts xo = {sizeof(ptts_dsp_ext_opts), 0, 0.0};
    ptts_dsp_ext* e = nullptr;
    CHECK(ptts_dsp_ext_create(&xo, &e) == PTTS_OK && e);
    ptts_dsp_opts o = ptts_dsp_opts();
    o.ext = e;
    DspSpec s;
    CHECK(dsp_resolve(&o, &s).empty() && !s.any() && !dsp_active(&o));               // a handle that switches nothing on
    CHECK(ptts_dsp_ext_set_compressor(e, &c) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && s.compress && s.any() && !s.rest() && dsp_active(&o));
    const CmpScan want = cmp_design(c);
    CHECK(std::memcmp(&s.cmp, &want, sizeof want) == 0);                              // the design, by value
    ptts_compressor_opts bad = c;
    bad.ratio = 0.5;
    CHECK(ptts_dsp_ext_set_compressor(e, &bad) == PTTS_EINVAL && has(g_err, "ratio"));
    CHECK(dsp_resolve(&o, &s).empty() && s.compress);                                 // a refused call changes nothing
    CHECK(ptts_dsp_ext_set_compressor(e, nullptr) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && !s.any() && !s.compress && !dsp_active(&o)); // cleared: nothing on again
    CHECK(ptts_dsp_ext_set_compressor(e, &c) == PTTS_OK);
    // beside the ceiling: the existing truth table is as it was
    xo.true_peak = 1; xo.ceiling_dbtp = -3.0;
    ptts_dsp_ext* t = nullptr;
    CHECK(ptts_dsp_ext_create(&xo, &t) == PTTS_OK && t);
    o.ext = t;
    CHECK(dsp_resolve(&o, &s).empty() && s.true_peak && !s.compress && s.rest() && dsp_active(&o));
    CHECK(ptts_dsp_ext_set_compressor(t, &c) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && s.true_peak && s.compress && dsp_active(&o));
    ptts_dsp_ext_free(t);
    ptts_dsp_ext_free(e);
    // freed: refused unread (the sanitizer reports any read of the freed block)
    CHECK(ptts_dsp_ext_set_compressor(e, &c) == PTTS_EINVAL && has(g_err, "not a live handle"));
    CHECK(ptts_dsp_ext_set_compressor(e, nullptr) == PTTS_EINVAL);
    CHECK(ptts_dsp_ext_set_compressor(nullptr, &c) == PTTS_EINVAL && has(g_err, "not a live handle"));
    o.ext = e;
    CHECK(has(dsp_resolve(&o, &s), "dsp: ext") && !dsp_active(&o));
    return 0;
}

int main() {
    if (rows() || handles()) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/compressor.cpp and the handle registry (eq.cpp, true_peak.cpp, dsp_spec.cpp), built with g++
    -fsanitize=address,undefined and run as a subprocess.  Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "compressor_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "compressor_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main)] + [os.path.join(CSRC, f) for f in ("compressor.cpp", "dsp_spec.cpp", "eq.cpp", "true_peak.cpp")] + ["-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
