"""CPU-side checks of the true-peak ceiling (include/ptts.h ptts_true_peak*, ptts_dsp_ext_*; go-pocket-tts_amd/csrc/true_peak.cpp, true_peak.h;
DESIGN.md section 8, N3): ptts_dsp_opts kept its layout with `ext` over reserved[2..3]; ptts_dsp_ext_create refuses bad options by name; the host
meter agrees with its float64 restatement within the bound of its fmaf chains and reads known signals right; ptts_true_peak_limit is one f32
gain, or nothing."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _eq_ref as E
import _true_peak_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 26, 27, 54, 55, 1919, 1920, 1921, 5000]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _db(v):
    return 20.0 * math.log10(v)


def test_dsp_opts_keeps_its_layout_and_ext_lies_over_reserved(pkg, tmp_path):
    rt = pkg.runtime
    assert C.sizeof(rt.DspOpts) == 40 and rt.DspOpts.reserved.offset == 24 and rt.DspOpts.eq.offset == 24 and rt.DspOpts.ext.offset == 32
    assert C.sizeof(rt.DspExtOpts) == 16 and rt.DspExtOpts.ceiling_dbtp.offset == 8
    o = rt.DspOpts(normalize=1, fade_in_ms=2.5)
    o.eq = 0x1122334455667788
    o.ext = 0x0102030405060708
    assert (o.normalize, o.fade_in_ms) == (1, 2.5) and list(o.reserved) == [0x55667788, 0x11223344, 0x05060708, 0x01020304]
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_dsp_opts), '
                   'offsetof(ptts_dsp_opts, reserved), offsetof(ptts_dsp_opts, eq), offsetof(ptts_dsp_opts, ext), sizeof(ptts_dsp_ext_opts)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 24, 24, 32, 16]
    if shutil.which("g++"):
        cpp = tmp_path / "t.cpp"
        cpp.write_text(src.read_text())
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)])
        assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 24, 24, 32, 16]


def test_symbols(pkg):
    rt = pkg.runtime
    for s in ("ptts_dsp_ext_create", "ptts_dsp_ext_free", "ptts_true_peak", "ptts_true_peak_limit", "ptts_true_peak_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    for s in ("ptts_debug_true_peak_taps", "ptts_debug_true_peak_oversample"):
        assert s in rt.HOOK_SYMBOLS and hasattr(rt.hooks(), s) and not hasattr(rt.lib(), s), s


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint32 * 4), ("tail", C.c_uint8 * 16)]


def _create_raw(rt, buf):
    L = rt.lib()
    L.ptts_dsp_ext_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    rc = L.ptts_dsp_ext_create(C.byref(buf), C.byref(h))
    return rc, L.ptts_last_error().decode(errors="replace"), h.value


def test_ext_create_refusals_name_the_field(pkg):
    rt = pkg.runtime
    nan = float("nan")
    for opts, field in [(rt.DspExtOpts(8, 1, -1.0), "size"), (rt.DspExtOpts(0, 1, -1.0), "size"), (rt.DspExtOpts(16, 2, -1.0), "true_peak"),
                        (rt.DspExtOpts(16, -1, -1.0), "true_peak"), (rt.DspExtOpts(16, 1, 0.5), "ceiling_dbtp"), (rt.DspExtOpts(16, 1, -61.0), "ceiling_dbtp"),
                        (rt.DspExtOpts(16, 1, nan), "ceiling_dbtp"), (rt.DspExtOpts(16, 1, float("-inf")), "ceiling_dbtp")]:
        rc, msg, h = _create_raw(rt, opts)
        assert rc == rt.PTTS_EINVAL and field in msg and h is None, (field, rc, msg)
        with pytest.raises(pkg.PttsError) as ei:
            rt.DspExt(opts=opts)
        assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value)
    # a larger struct: zeros beyond what the library knows are "off", anything else is refused
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.DspExtOpts(32, 1, -1.0)), 16)
    rc, msg, h = _create_raw(rt, wide)
    assert rc == rt.PTTS_OK and h
    rt.lib().ptts_dsp_ext_free(C.c_void_p(h))
    for at in (0, 15):
        wide.tail[at] = 1
        rc, msg, h = _create_raw(rt, wide)
        assert rc == rt.PTTS_EINVAL and "size" in msg and h is None, (at, msg)
        wide.tail[at] = 0
    # the edges of the range are inside it; a handle that switches nothing on is a handle
    for c in (-60.0, 0.0):
        rt.DspExt(true_peak_dbtp=c).free()
    rt.DspExt().free()
    rt.lib().ptts_dsp_ext_free(None)


def test_a_freed_handle_is_not_live(pkg):
    """The check every entry point runs on a ptts_dsp_opts (the hook ptts_debug_dsp_opts_error): an address the registry does not know is refused
    unread, with the words the refusal tests of the earlier stages look for."""
    rt = pkg.runtime
    e = rt.DspExt(true_peak_dbtp=-1.0)
    h = e.h
    o = rt.DspOpts()
    o.ext = h
    assert rt.dsp_opts_error(o) == ""
    e.free()
    rt.lib().ptts_dsp_ext_free(C.c_void_p(h))                    # freeing it again does nothing
    eq = rt.Eq(E.CASCADES["s1"])                                 # an equaliser is no ptts_dsp_ext
    for bad in (h, eq.h, 7, 1 << 32):
        o = rt.DspOpts()
        o.ext = bad
        msg = rt.dsp_opts_error(o)
        assert "dsp: ext" in msg and "reserved[2..3]" in msg and "live handle" in msg, (hex(bad), msg)
    o = rt.DspOpts()
    o.eq = eq.h
    assert rt.dsp_opts_error(o) == ""
    live = rt.DspExt(true_peak_dbtp=-3.0)
    o.ext = live.h
    assert rt.dsp_opts_error(o) == ""
    live.free()
    eq.free()


@pytest.fixture(scope="module")
def signal():
    return E.signal(max(LENGTHS), seed=21)


def test_host_is_the_float64_meter_within_the_chain_bound(pkg, signal):
    rt = pkg.runtime
    h = T.taps(pkg)
    S = T.gain_sum(h)
    print(f"S = max over phases of sum |h| = {S:.4f}")
    assert 2.0 < S < 2.4
    out = os.environ.get("PTTS_TP_PARITY_OUT")
    for n in LENGTHS:
        x = signal[:n]
        y = rt.true_peak_oversample(x)
        ref = T.oversample(x, h)
        assert y.size == 8 * n and ref.size == 8 * n
        tp = rt.true_peak(x)
        if n == 0:
            assert tp == 0.0
            continue
        bound = T.y_bound(x, h)
        err = float(np.abs(y.astype(np.float64) - ref).max())
        print(f"n={n}: max |host y - ref y| {err:.3e}, bound {bound:.3e}")
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"case": f"host y n={n}", "observed": err, "bound": bound, "observed_over_bound": err / bound}) + "\n")
        assert err <= bound, (n, err, bound)
        assert _u32(np.float32(tp)) == _u32(np.float32(max(np.abs(x).max(), np.abs(y).max())))   # TP is the maximum over exactly these
        assert abs(float(tp) - T.true_peak(x, h)) <= bound and tp >= np.abs(x).max()


def test_known_answers(pkg):
    rt = pkg.runtime
    h = T.taps(pkg)
    amp = 0.5
    for freq, phase, sample_db in [(6000.0, math.pi / 4, -3.0103), (3000.0, math.pi / 8, -0.6877), (997.0, 0.0, 0.0)]:
        x = T.tone(freq, phase, amp)
        sp, tp, ref = float(np.abs(x).max()), float(rt.true_peak(x)), T.true_peak(x, h)
        print(f"{freq:.0f} Hz: sample peak {_db(sp / amp):+.4f} dB, true peak {_db(tp / amp):+.5f} dB (float64 restatement {_db(ref / amp):+.5f} dB)")
        assert abs(_db(tp / amp)) <= 0.01, (freq, tp)
        assert abs(_db(sp / amp) - sample_db) <= (0.001 if freq == 6000.0 else 0.01), (freq, sp)
    for n in (1, 27, 5000):
        for at in (0, n - 1):
            x = np.zeros(n, np.float32)
            x[at] = 1.0
            assert rt.true_peak(x) == 1.0, (n, at)
            x[at] = -1.0
            assert rt.true_peak(x) == 1.0, (n, at)
    x = T.burst(4000, 1900)
    assert rt.true_peak(x) > 1.01 * np.abs(x).max()              # the crest between the samples is what the meter is for
    x[100] = np.nan                                              # a NaN never wins: the peak is that of the windows it does not touch
    assert np.isfinite(rt.true_peak(x)) and rt.true_peak(x) > 1.01 * np.nanmax(np.abs(x))


def test_limit_is_one_f32_gain_or_nothing(pkg, signal):
    rt = pkg.runtime
    h = T.taps(pkg)
    S = T.gain_sum(h)
    out = os.environ.get("PTTS_TP_PARITY_OUT")
    for x in (signal[:5000], T.burst(4000, 1900), T.tone(6000.0, math.pi / 4)):
        tp = rt.true_peak(x)
        ceiling = _db(float(tp)) - 6.0
        y, before = rt.true_peak_limit(x, ceiling)
        assert _u32(before) == _u32(tp)
        c = np.float32(10.0 ** (ceiling / 20.0))
        g = np.float32(c) / np.float32(tp)
        assert g.dtype == np.float32 and np.array_equal(_u32(y), _u32(x * g))
        again = float(rt.true_peak(y))
        bound = (2 * T.K + 3) * T.EPS * S
        print(f"ceiling {ceiling:.2f} dBTP: true peak after {again:.7f}, c {float(c):.7f}, excess {again / float(c) - 1.0:+.2e}, bound {bound:.2e}")
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"case": f"ceiling excess n={x.size}", "observed": max(again / float(c) - 1.0, 0.0), "bound": bound,
                                    "observed_over_bound": max(again / float(c) - 1.0, 0.0) / bound}) + "\n")
        assert again <= float(c) * (1.0 + bound)
        above = min(_db(float(tp)) + 1.0, 0.0)
        if above > _db(float(tp)):
            same, before = rt.true_peak_limit(x, above)
            assert np.array_equal(_u32(same), _u32(x)) and _u32(before) == _u32(tp)
    for bad in (0.5, -61.0, float("nan")):
        with pytest.raises(pkg.PttsError) as ei:
            rt.true_peak_limit(signal[:100], bad)
        assert ei.value.code == rt.PTTS_EINVAL and "ceiling_dbtp" in str(ei.value)
    y, before = rt.true_peak_limit(np.zeros(0, np.float32), -1.0)
    assert y.size == 0 and before == 0.0
