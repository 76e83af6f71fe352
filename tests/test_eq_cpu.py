"""CPU-side checks of the per-request equaliser (include/ptts.h ptts_eq_*; go-pocket-tts_amd/csrc/eq.cpp, scan_block.h):
ptts_dsp_opts kept its layout with `eq` over reserved[0..1]; the designed sections are the cookbook's; ptts_eq_apply -- the blocked form the device
kernels run -- agrees with the sequential float64 recurrence to one f32 step at the row's peak; bad arguments are refused by name; and the host
code is clean under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import ctypes as C
import itertools
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _eq_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_dsp_opts_keeps_its_layout_and_eq_lies_over_reserved(pkg, tmp_path):
    rt = pkg.runtime
    assert C.sizeof(rt.DspOpts) == 40 and rt.DspOpts.reserved.offset == 24 and rt.DspOpts.eq.offset == 24
    assert C.sizeof(rt.EqSection) == 32
    o = rt.DspOpts(normalize=1, fade_in_ms=2.5)
    o.reserved[2] = 7
    o.eq = 0x1122334455667788
    assert (o.normalize, o.fade_in_ms, o.reserved[2]) == (1, 2.5, 7) and o.reserved[0] == 0x55667788 and o.reserved[1] == 0x11223344
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(ptts_dsp_opts), '
                   'offsetof(ptts_dsp_opts, reserved), offsetof(ptts_dsp_opts, eq), sizeof(ptts_eq_section)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 24, 24, 32]
    if shutil.which("g++"):
        cpp = tmp_path / "t.cpp"
        cpp.write_text(src.read_text())
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)])
        assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 24, 24, 32]


def test_symbols(pkg):
    rt = pkg.runtime
    for s in ("ptts_eq_design", "ptts_eq_response", "ptts_eq_create", "ptts_eq_free", "ptts_eq_apply", "ptts_eq_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s


@pytest.mark.parametrize("kind", E.TYPES)
def test_design_is_the_cookbook_section(pkg, kind):
    """Same float64 formulas on both sides: libm differences only."""
    rt = pkg.runtime
    for f, g, q in E.box(kind):
        got = rt.eq_design((kind, f, g, q))
        want = np.array(E.design(kind, f, g, q))
        rel = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"type {kind} f0={f} gain={g} q={q}: max relative difference {rel:.3e}")
        assert rel <= 1e-12, (kind, f, g, q, got, want)
        b0, b1, b2, a1, a2 = got
        assert abs(a2) < 1.0 and abs(a1) < 1.0 + a2, (kind, f, g, q, a1, a2)      # both poles inside the unit circle


def test_dc_block_section_is_one_of_these(pkg):
    import _dsp_ref as D
    got = pkg.runtime.eq_design((E.HIGHPASS, 20.0, 0.0, 0.707))
    assert np.max(np.abs(got - np.array(D.dc_coeffs())) / np.abs(np.array(D.dc_coeffs()))) <= 1e-12


def test_response(pkg):
    rt = pkg.runtime
    for f0 in (100.0, 1000.0, 5000.0):
        assert abs(rt.eq_response([(E.PEAKING, f0, 6.0, 1.0)], f0) - 6.0) <= 1e-9
        assert abs(rt.eq_response([(E.HIGHPASS, f0, 0.0, 0.7071)], f0) - -3.01) <= 0.01
        assert abs(rt.eq_response([(E.LOWPASS, f0, 0.0, 0.7071)], f0) - -3.01) <= 0.01
    assert abs(rt.eq_response([(E.HIGHSHELF, 1000.0, 9.0, 0.7071)], 11500.0) - 9.0) <= 0.01
    assert abs(rt.eq_response([(E.HIGHSHELF, 1000.0, 9.0, 0.7071)], 20.0)) <= 0.01
    assert abs(rt.eq_response([(E.LOWSHELF, 1000.0, -12.0, 0.7071)], 20.0) - -12.0) <= 0.01
    assert abs(rt.eq_response([(E.LOWSHELF, 1000.0, -12.0, 0.7071)], 11500.0)) <= 0.01
    for name, secs in E.CASCADES.items():      # the cascade multiplies its sections; the restated formulas agree
        for f in (50.0, 300.0, 1000.0, 3400.0, 9000.0):
            assert abs(rt.eq_response(secs, f) - E.response_db(secs, f)) <= 1e-9, (name, f)
    eq = rt.Eq(E.CASCADES["s2"])               # telephony band: flat inside, falling outside
    assert abs(eq.response(1000.0)) < 0.5 and eq.response(60.0) < -24.0 and eq.response(10000.0) < -18.0
    for bad in (0.0, 12000.0, float("nan")):
        with pytest.raises(pkg.PttsError) as ei:
            rt.eq_response(E.CASCADES["s1"], bad)
        assert ei.value.code == rt.PTTS_EINVAL and "freq_hz" in str(ei.value)


@pytest.fixture(scope="module")
def references():
    """The sequential float64 recurrence over the longest signal, once per cascade: a shorter length's reference is its prefix."""
    x = E.signal(max(E.LENGTHS), seed=11)
    return x, {name: E.apply(x, secs) for name, secs in E.CASCADES.items()}


@pytest.mark.parametrize("name", list(E.CASCADES))
def test_apply_is_the_sequential_recurrence_to_one_f32_step(pkg, references, name):
    rt = pkg.runtime
    x, refs = references
    eq = rt.Eq(E.CASCADES[name])
    out = os.environ.get("PTTS_EQ_PARITY_OUT")
    moved = float(np.abs(refs[name].astype(np.float64) - x.astype(np.float64)).max())
    assert moved > 0.05                                         # the cascade does something: a skipped filter shows
    for n in E.LENGTHS:
        got, ref = eq.apply(x[:n]), refs[name][:n]
        assert got.size == n
        if n == 0:
            continue
        diff = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        bound = E.bound(ref)
        print(f"{name} n={n}: max |blocked - sequential| {diff:.3e}, bound {bound:.3e}, {np.count_nonzero(got != ref)} of {n} samples differ")
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"case": f"{name} n={n}", "observed": diff, "bound": bound, "observed_over_bound": diff / bound}) + "\n")
        assert diff <= bound, (name, n, diff, bound)
        assert np.array_equal(_u32(got[:30]), _u32(ref[:30]))   # the first run starts from the same zero state with the same operations
    eq.free()


def test_identity(pkg):
    """A 0 dB peaking section returns the input by value, in every place of a cascade."""
    rt = pkg.runtime
    x = E.signal(5000, seed=3)
    for secs in ([(E.PEAKING, 1000.0, 0.0, 1.0)], [(E.PEAKING, 10.0, 0.0, 10.0)] * 4):
        assert np.array_equal(rt.Eq(secs).apply(x), x)
    both = rt.Eq([(E.PEAKING, 700.0, 0.0, 2.0)] + E.CASCADES["s2"]).apply(x)
    assert np.array_equal(_u32(both), _u32(rt.Eq(E.CASCADES["s2"]).apply(x)))


def test_refusals_name_the_field_and_the_section(pkg):
    rt = pkg.runtime
    good = (E.PEAKING, 1000.0, 3.0, 1.0)
    nan, inf = float("nan"), float("inf")
    bad = [((0, 1000.0, 0.0, 1.0), "type"), ((6, 1000.0, 0.0, 1.0), "type"),
           ((E.PEAKING, 9.99, 0.0, 1.0), "freq_hz"), ((E.PEAKING, 11000.5, 0.0, 1.0), "freq_hz"), ((E.PEAKING, nan, 0.0, 1.0), "freq_hz"),
           ((E.PEAKING, inf, 0.0, 1.0), "freq_hz"), ((E.LOWSHELF, 1000.0, 24.5, 1.0), "gain_db"), ((E.HIGHSHELF, 1000.0, -24.5, 1.0), "gain_db"),
           ((E.PEAKING, 1000.0, nan, 1.0), "gain_db"), ((E.PEAKING, 1000.0, -inf, 1.0), "gain_db"), ((E.PEAKING, 1000.0, 0.0, 0.05), "q"),
           ((E.PEAKING, 1000.0, 0.0, 10.5), "q"), ((E.PEAKING, 1000.0, 0.0, nan), "q"), ((E.PEAKING, 1000.0, 0.0, inf), "q"),
           ((E.LOWPASS, 1000.0, 3.0, 1.0), "gain_db"), ((E.HIGHPASS, 1000.0, -1.0, 1.0), "gain_db"), ((E.HIGHPASS, 1000.0, nan, 1.0), "gain_db")]
    for sec, field in bad:
        for at in (0, 2):
            secs = [good] * at + [sec]
            for call in (lambda: rt.Eq(secs), lambda: rt.eq_response(secs, 1000.0)):
                with pytest.raises(pkg.PttsError) as ei:
                    call()
                assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value) and f"section {at}" in str(ei.value), (sec, at, str(ei.value))
        with pytest.raises(pkg.PttsError) as ei:
            rt.eq_design(sec)
        assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value) and "section 0" in str(ei.value)
    res = rt.EqSection(E.PEAKING, 5, 1000.0, 0.0, 1.0)
    with pytest.raises(pkg.PttsError) as ei:
        rt.Eq([good, res])
    assert ei.value.code == rt.PTTS_EINVAL and "reserved" in str(ei.value) and "section 1" in str(ei.value)
    for n in (0, 5):
        with pytest.raises(pkg.PttsError) as ei:
            rt.Eq([good] * n)
        assert ei.value.code == rt.PTTS_EINVAL and f"n is {n}" in str(ei.value)
    # the edges of the box are inside it
    for sec in itertools.chain.from_iterable([(k, f, g, q) for f, g, q in E.box(k)] for k in E.TYPES):
        rt.Eq([sec]).free()
    # a freed handle is not an equaliser any more; freeing NULL or freeing twice does nothing
    eq = rt.Eq([good])
    h = eq.h
    eq.free()
    L = rt.lib()
    x = np.ones(8, np.float32)
    assert L.ptts_eq_apply(C.c_void_p(h), x.ctypes.data_as(C.POINTER(C.c_float)), 8) == rt.PTTS_EINVAL and b"eq" in L.ptts_last_error()
    L.ptts_eq_free(None)
    L.ptts_eq_free(C.c_void_p(h))
    assert np.array_equal(x, np.ones(8, np.float32))


SANITIZER_MAIN = r'''
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include "eq.h"
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
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (%s)\n", __LINE__, #c, ptts::g_err.c_str()); return 1; } } while (0)
int main() {
    const ptts_eq_section s[4] = {{PTTS_EQ_HIGHPASS, 0, 80.0, 0.0, 0.7071}, {PTTS_EQ_PEAKING, 0, 10.0, 24.0, 10.0}, {PTTS_EQ_LOWSHELF, 0, 300.0, -6.0, 0.9},
                                  {PTTS_EQ_HIGHSHELF, 0, 11000.0, 24.0, 0.1}};
    const long lengths[4] = {0, 1, 1921, 122881};
    for (int n = 1; n <= 4; n++) {
        ptts_eq* e = nullptr;
        CHECK(ptts_eq_create(s, n, &e) == PTTS_OK && e);
        double db = 0.0, c[5];
        CHECK(ptts_eq_response(s, n, 1000.0, &db) == PTTS_OK && ptts_eq_design(s + n - 1, c) == PTTS_OK);
        for (long len : lengths) {
            std::vector<float> x((size_t)len);                  // exactly len samples: a read or a write past the end is caught
            for (long i = 0; i < len; i++) x[(size_t)i] = 0.25f + 0.5f * (float)((i * 7919) % 200 - 100) / 100.0f;
            CHECK(ptts_eq_apply(e, x.data(), len) == PTTS_OK);
            for (long i = 0; i < len; i++) CHECK(x[(size_t)i] == x[(size_t)i]);
        }
        CHECK(ptts::eq_lookup(e) == &e->sc);
        ptts_eq_free(e);
        CHECK(ptts::eq_lookup(e) == nullptr);                   // a freed handle: looked up by address, never read
        float one = 1.0f;
        CHECK(ptts_eq_apply(e, &one, 1) == PTTS_EINVAL && one == 1.0f);
        ptts_eq_free(e);                                        // ... and freeing it again does nothing
    }
    ptts_eq* e = nullptr;
    CHECK(ptts_eq_create(s, 0, &e) == PTTS_EINVAL && !e && ptts_eq_create(s, 5, &e) == PTTS_EINVAL && !e);
    ptts_eq_free(nullptr);
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/eq.cpp, built with g++ -fsanitize=address,undefined and run as a subprocess."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    main = tmp_path / "eq_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "eq_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), os.path.join(CSRC, "eq.cpp"), "-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
