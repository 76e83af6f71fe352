"""CPU-side checks of the look-ahead peak limiter (include/ptts.h ptts_limiter_opts, ptts_limit_apply, ptts_dsp_ext_set_limiter;
go-pocket-tts_amd/csrc/limiter.{h,cpp}): the struct's layout; refusals that name their field; ptts_limit_apply -- the
blocked form the kernels run -- against the sample-by-sample statement of _limiter_ref.py within one f32 step at the row's peak; the ceiling
c (1 + 2^-22); that it engages only where it must; that the look-ahead is L samples; placed crests; a NaN that stays where it is; and a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _compressor_ref as CR
import _eq_ref as E
import _limiter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
OVER = 1.0 + 2.0 ** -22   # limiter.h: |y| <= c (1 + 2^-22)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _opts(rt, design, **kw):
    return rt.LimiterOpts(*design, **kw)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in ("ptts_dsp_ext_set_limiter", "ptts_limit_apply", "ptts_limit_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    assert C.sizeof(rt.LimiterOpts) == 40 and rt.LimiterOpts.ceiling_db.offset == 8 and rt.LimiterOpts.drive_db.offset == 32
    assert rt.LimiterOpts().size == 40
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(ptts_limiter_opts), '
                   'offsetof(ptts_limiter_opts, ceiling_db), offsetof(ptts_limiter_opts, drive_db)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 8, 32]


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 40), ("tail", C.c_uint8 * 16)]


def _apply_raw(rt, buf):
    L = rt.lib()
    x = np.zeros(8, np.float32)
    rc = L.ptts_limit_apply(C.cast(C.byref(buf), C.POINTER(rt.LimiterOpts)), x.ctypes.data_as(C.POINTER(C.c_float)), 8)
    return rc, L.ptts_last_error().decode(errors="replace")


def test_refusals_name_the_field(pkg):
    rt = pkg.runtime
    nan, inf = float("nan"), float("inf")
    good = dict(ceiling_db=-1.0, lookahead_ms=1.5, release_ms=80.0, drive_db=0.0)
    bad = [("ceiling_db", (-60.5, 0.5, nan, -inf)), ("lookahead_ms", (0.24, 5.01, nan, 0.0, inf)), ("release_ms", (4.9, 5000.5, nan)),
           ("drive_db", (-0.1, 24.5, nan, inf))]
    x = np.zeros(8, np.float32)
    ext = rt.DspExt()
    for field, values in bad:
        for v in values:
            o = rt.LimiterOpts(**dict(good, **{field: v}))
            for call in (lambda: rt.limit_apply(o, x), lambda: ext.set_limiter(o)):
                with pytest.raises(pkg.PttsError) as ei:
                    call()
                assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value), (field, v, str(ei.value))
    for o, field in [(rt.LimiterOpts(size=32), "size"), (rt.LimiterOpts(size=0), "size"), (rt.LimiterOpts(reserved=1), "reserved")]:
        with pytest.raises(pkg.PttsError) as ei:
            rt.limit_apply(o, x)
        assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value), (field, str(ei.value))
    # every edge of the box is inside it
    for field, lo, hi in [("ceiling_db", -60.0, 0.0), ("lookahead_ms", 0.25, 5.0), ("release_ms", 5.0, 5000.0), ("drive_db", 0.0, 24.0)]:
        for v in (lo, hi):
            assert np.isfinite(rt.limit_apply(rt.LimiterOpts(**dict(good, **{field: v})), E.signal(300, seed=1))).all()
    # a larger struct: zeros beyond what the library knows are "off", anything else is refused
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.LimiterOpts(size=56)), 40)
    rc, msg = _apply_raw(rt, wide)
    assert rc == rt.PTTS_OK, msg
    for at in (0, 15):
        wide.tail[at] = 1
        rc, msg = _apply_raw(rt, wide)
        assert rc == rt.PTTS_EINVAL and "size" in msg, (at, msg)
        wide.tail[at] = 0
    ext.free()


def test_the_setter_wants_a_live_handle(pkg):
    rt = pkg.runtime
    L = rt.lib()
    o = rt.LimiterOpts()
    ext = rt.DspExt(true_peak_dbtp=-1.0, limiter=o)
    d = rt.DspOpts()
    d.ext = ext.h
    assert rt.dsp_opts_error(d) == ""
    ext.set_limiter(None)                                        # accepted; that nothing is on again is the sanitizer program's to assert (dsp_resolve, dsp_active)
    assert rt.dsp_opts_error(d) == ""
    ext.set_limiter(o)
    h = ext.h
    ext.free()
    eq = rt.Eq(E.CASCADES["s1"])                                 # an equaliser is no ptts_dsp_ext
    for dead in (h, eq.h, None, 7):
        for l in (C.byref(o), None):
            rc = L.ptts_dsp_ext_set_limiter(C.c_void_p(dead), l)
            msg = L.ptts_last_error().decode(errors="replace")
            assert rc == rt.PTTS_EINVAL and "ext" in msg and "not a live handle" in msg, (dead, msg)
    eq.free()
    with pytest.raises(pkg.PttsError) as ei:                     # the options are checked where the handle is made, and nothing leaks a handle
        rt.DspExt(limiter=rt.LimiterOpts(drive_db=-1.0))
    assert "drive_db" in str(ei.value)


@pytest.fixture(scope="module")
def cases():
    """design name -> [(x, the reference)] for every length: computed once, never written to.  The limiter looks ahead, so the reference of a
    prefix is not a prefix of the reference: every length has its own."""
    out = {}
    for name, design in R.DESIGNS.items():
        lens = R.lengths(R.ahead(design))
        whole = E.signal(max(lens), seed=31)
        rows = []
        for n in lens:
            x = whole[:n].copy()
            ref = R.apply(x, design)
            for a in (x, ref):
                a.setflags(write=False)
            rows.append((x, ref))
        out[name] = rows
    return out


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_apply_is_the_sample_by_sample_statement_within_one_step(pkg, cases, name):
    rt = pkg.runtime
    design = R.DESIGNS[name]
    o = _opts(rt, design)
    c = R.ceiling(design)
    for x, ref in cases[name]:
        n = x.size
        got = rt.limit_apply(o, x)
        assert got.dtype == np.float32 and got.shape == (n,)
        if n == 0:
            continue
        err = float(np.abs(got.astype(np.float64) - ref).max())
        diff = int((_u32(got) != _u32(ref)).sum())
        peak = float(np.abs(got).max())
        print(f"{name} n={n}: max err {err:.3e} (bound {E.bound(ref):.3e}), {diff} samples differ; peak / c - 1 = {peak / c - 1.0:.3e}")
        assert err <= E.bound(ref), (name, n, err)
        assert peak <= c * OVER, (name, n, peak, c)
    # the stage bites on the longest row: it moves the audio far above the bound
    x, ref = cases[name][-1]
    moved = float(np.abs(ref.astype(np.float64) - x.astype(np.float64) * math.pow(10.0, design[3] / 20.0)).max())
    print(f"{name}: moved {moved:.3e} = {moved / E.bound(ref):.0f} bounds")
    assert moved > 1000.0 * E.bound(ref)


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_the_ceiling_holds_with_20_db_of_drive(pkg, cases, name):
    rt = pkg.runtime
    design = R.DESIGNS[name][:3] + (20.0,)
    o = _opts(rt, design)
    c = R.ceiling(design)
    for x, _ in cases[name]:
        if x.size == 0:
            continue
        peak = float(np.abs(rt.limit_apply(o, x)).max())
        assert peak <= c * OVER, (name, x.size, peak, c)
    assert peak >= 0.99 * c                                       # (the longest row: the drive brought it up to the ceiling)


def test_it_engages_only_where_it_must(pkg):
    rt = pkg.runtime
    x = E.signal(124801, seed=7)
    got = rt.limit_apply(_opts(rt, R.DESIGNS["gentle"]), x)
    changed = float((_u32(got) != _u32(x)).mean())
    print(f"signal: {100.0 * changed:.2f} % of the samples changed")
    assert 0.0 < changed < 0.10
    # a burst, then a quiet tail: behind the last reduced sample the input comes back bit for bit
    design = (-6.0, 1.5, 80.0, 0.0)
    b = CR.burst(9601)
    got = rt.limit_apply(_opts(rt, design), b)
    last = int(np.flatnonzero(_u32(got) != _u32(b)).max())
    print(f"burst: the last changed sample is {last}, the untouched tail has {b.size - 1 - last} samples")
    assert 6000 < last < 8000                                     # the burst ends at 6000; the release (80 ms) needs about 1150 samples from 0.9 down to c = 0.5
    assert (_u32(got[last + 1:]) == _u32(b[last + 1:])).all() and b.size - 1 - last > 1000
    assert float(np.abs(got[:6000]).max()) <= R.ceiling(design) * OVER < float(np.abs(b[:6000]).max())


@pytest.mark.parametrize("name", list(R.DESIGNS))
def test_the_look_ahead_is_what_it_says(pkg, name):
    """y[i] depends on x[0, i + L] only: y[:k] of a row is y[:k] of the row cut at k + L, bit for bit."""
    rt = pkg.runtime
    design = R.DESIGNS[name]
    o, L = _opts(rt, design), R.ahead(design)
    x = E.signal(6000, seed=11)
    whole = rt.limit_apply(o, x)
    for k in (1, 30, 1919, 1920, 1921, 3000, 3840):
        cut = rt.limit_apply(o, x[:k + L])
        assert (_u32(cut[:k]) == _u32(whole[:k])).all(), (name, k)
    # ... and no less: a crest L samples ahead is seen, one further is not
    y = np.full(400, 0.25, np.float32)
    y[200] = 4.0
    got, flat = rt.limit_apply(o, y), rt.limit_apply(o, np.full(400, 0.25, np.float32))
    assert got[200 - L] < flat[200 - L] and (_u32(got[:200 - L]) == _u32(flat[:200 - L])).all()


def crest_rows(design, n=3841):
    """a quiet constant with one sample of 2.0: (name, row, index of the crest)"""
    L = R.ahead(design)
    rows = []
    for at in (0, n - 1, 1919, 1920, 1920 + L // 2):
        x = np.full(n, 0.25, np.float32)
        x[at] = 2.0
        rows.append((f"crest{at}", x, at))
    return rows


def test_placed_crests(pkg):
    rt = pkg.runtime
    design = R.DESIGNS["gentle"]
    o, L, c = _opts(rt, design), R.ahead(design), R.ceiling(design)
    for name, x, at in crest_rows(design):
        got = rt.limit_apply(o, x)
        ref = R.apply(x, design)
        assert float(np.abs(got.astype(np.float64) - ref).max()) <= E.bound(ref), name
        assert c * (1.0 - 2.0 ** -20) <= float(got[at]) <= c * OVER, (name, got[at])          # the crest lands on the ceiling
        lo = max(at - L, 0)
        g = got[lo:at].astype(np.float64) / 0.25                                              # the gain in front of the crest
        assert (np.diff(g) <= 0.0).all() and (g <= 1.0).all(), name                           # monotone down to it
        if at > L:
            assert (_u32(got[:at - L]) == _u32(x[:at - L])).all() and got[at - L] < x[at - L], name   # it starts L samples ahead, not earlier
        if at == 1920 + L // 2:
            assert got[1919] < x[1919]                                                        # in the tile before the crest's
        assert float(np.abs(got).max()) <= c * OVER


def test_a_nan_stays_where_it_is(pkg):
    rt = pkg.runtime
    o = _opts(rt, R.DESIGNS["gentle"])
    x = E.signal(3841, seed=3)
    clean = rt.limit_apply(o, x)
    y = x.copy()
    y[1930] = np.nan
    got = rt.limit_apply(o, y)
    assert np.isnan(got[1930]) and int(np.isnan(got).sum()) == 1
    keep = np.arange(3841) != 1930
    L = R.ahead(R.DESIGNS["gentle"])
    assert (_u32(got[:1930 - 2 * L]) == _u32(clean[:1930 - 2 * L])).all()          # nothing in front of the hold windows that held it has moved
    assert float(np.abs(got[keep]).max()) <= R.ceiling(R.DESIGNS["gentle"]) * OVER  # the hold skipped one sample; every other one is still held
    ref = R.apply(y, R.DESIGNS["gentle"])
    assert float(np.abs(got[keep].astype(np.float64) - ref[keep]).max()) <= E.bound(ref[keep])


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

static ptts_limiter_opts opts(double lookahead_ms) {
    ptts_limiter_opts l;
    std::memset(&l, 0, sizeof l);
    l.size = sizeof l; l.ceiling_db = -6.0; l.lookahead_ms = lookahead_ms; l.release_ms = 20.0; l.drive_db = 6.0;
    return l;
}

// rows in blocks of exactly their size: a read or a write one sample too far is reported
static int rows() {
    const double ahead[3] = {0.25, 1.5, 5.0};
    const long sizes[7] = {0, 1, 31, 120, 121, 1921, 3841};
    for (double ms : ahead) {
        const ptts_limiter_opts l = opts(ms);
        for (long n : sizes) {
            float* x = static_cast<float*>(std::malloc(n ? (size_t)n * sizeof(float) : 1));
            CHECK(x);
            for (long i = 0; i < n; i++) x[i] = 0.7f * (float)std::cos(0.05 * (double)i);
            CHECK(ptts_limit_apply(&l, n ? x : nullptr, n) == PTTS_OK);
            for (long i = 0; i < n; i++) CHECK(std::fabs(x[i]) <= 0.5012f);              // 0.7 * 2 is over the ceiling: every crest is held under it
            std::free(x);
        }
    }
    const ptts_limiter_opts l = opts(1.5);
    CHECK(ptts_limit_apply(&l, nullptr, 4) == PTTS_EINVAL && has(g_err, "null samples"));
    CHECK(ptts_limit_apply(&l, nullptr, -1) == PTTS_EINVAL);
    CHECK(ptts_limit_apply(nullptr, nullptr, 0) == PTTS_EINVAL && has(g_err, "null options"));
    return 0;
}

// set, clear and free on the registry: a handle's memory is read only while the registry holds it
static int handles() {
    const ptts_limiter_opts l = opts(1.5);
    ptts_dsp_ext_opts xo = {sizeof(ptts_dsp_ext_opts), 0, 0.0};
    ptts_dsp_ext* e = nullptr;
    CHECK(ptts_dsp_ext_create(&xo, &e) == PTTS_OK && e);
    ptts_dsp_opts o = ptts_dsp_opts();
    o.ext = e;
    DspSpec s;
    CHECK(dsp_resolve(&o, &s).empty() && !s.any() && !dsp_active(&o));               // a handle that switches nothing on
    CHECK(ptts_dsp_ext_set_limiter(e, &l) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && s.limit && s.any() && s.rest() && !s.compress && dsp_active(&o));
    const LimScan want = lim_design(l);
    CHECK(std::memcmp(&s.lim, &want, sizeof want) == 0 && want.L == 36);              // the design, by value
    ptts_limiter_opts bad = l;
    bad.lookahead_ms = 6.0;
    CHECK(ptts_dsp_ext_set_limiter(e, &bad) == PTTS_EINVAL && has(g_err, "lookahead_ms"));
    CHECK(dsp_resolve(&o, &s).empty() && s.limit);                                    // a refused call changes nothing
    CHECK(ptts_dsp_ext_set_limiter(e, nullptr) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && !s.any() && !s.limit && !dsp_active(&o));    // cleared: nothing on again
    // beside the ceiling and the compressor: each switch is its own
    xo.true_peak = 1; xo.ceiling_dbtp = -3.0;
    ptts_dsp_ext* t = nullptr;
    CHECK(ptts_dsp_ext_create(&xo, &t) == PTTS_OK && t);
    o.ext = t;
    ptts_compressor_opts c;
    std::memset(&c, 0, sizeof c);
    c.size = sizeof c; c.threshold_db = -24.0; c.ratio = 4.0; c.knee_db = 6.0; c.attack_ms = 5.0; c.release_ms = 120.0;
    CHECK(ptts_dsp_ext_set_compressor(t, &c) == PTTS_OK && ptts_dsp_ext_set_limiter(t, &l) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && s.true_peak && s.compress && s.limit && dsp_active(&o));
    CHECK(ptts_dsp_ext_set_limiter(t, nullptr) == PTTS_OK);
    CHECK(dsp_resolve(&o, &s).empty() && s.true_peak && s.compress && !s.limit);
    ptts_dsp_ext_free(t);
    ptts_dsp_ext_free(e);
    // freed: refused unread (the sanitizer reports any read of the freed block)
    CHECK(ptts_dsp_ext_set_limiter(e, &l) == PTTS_EINVAL && has(g_err, "not a live handle"));
    CHECK(ptts_dsp_ext_set_limiter(e, nullptr) == PTTS_EINVAL);
    CHECK(ptts_dsp_ext_set_limiter(nullptr, &l) == PTTS_EINVAL && has(g_err, "not a live handle"));
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
    """A stand-alone program over csrc/limiter.cpp, csrc/compressor.cpp and the handle registry (eq.cpp, true_peak.cpp, dsp_spec.cpp), built
    with g++ -fsanitize=address,undefined and run as a subprocess.  Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "limiter_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "limiter_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main)] + [os.path.join(CSRC, f) for f in ("limiter.cpp", "compressor.cpp", "dsp_spec.cpp", "eq.cpp", "true_peak.cpp")] + ["-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
