"""CPU-side checks of the device post-processing (go-pocket-tts_amd/csrc/dsp.hip, scan_block.h): the numpy restatement the GPU
tests use is tied to ptts_dsp_apply; the blocked form of the DC block -- the host instantiation of the functions the kernels call -- agrees with the
sequential recurrence to one f32 step; ptts_request kept its size and `dsp` sits where reserved2 sat."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _dsp_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = [dict(normalize=True), dict(fade_in_ms=50.0), dict(fade_out_ms=80.0), dict(fade_in_ms=1e6, fade_out_ms=1e6),
            dict(normalize=True, fade_in_ms=12.5, fade_out_ms=33.0)]


@pytest.mark.parametrize("n", D.LENGTHS)
def test_reference_chain_is_the_host_function(pkg, n):
    rt = pkg.runtime
    x = D.signal(n)
    for sw in SWITCHES:
        want = rt.dsp_apply(x, **sw)
        got = D.apply(x, normalize=sw.get("normalize", False), fade_in_ms=sw.get("fade_in_ms", 0.0), fade_out_ms=sw.get("fade_out_ms", 0.0))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, sw)
    for sw in (dict(dc_block=True), dict(normalize=True, dc_block=True, fade_in_ms=50.0, fade_out_ms=80.0)):
        want = rt.dsp_apply(x, **sw)
        got = D.apply(x, normalize=sw.get("normalize", False), dc=True, fade_in_ms=sw.get("fade_in_ms", 0.0), fade_out_ms=sw.get("fade_out_ms", 0.0))
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"ref vs host n={n} {sw}: max diff {err:.3e}, bound {D.dc_bound(want):.3e}")
        assert err <= D.dc_bound(want), (n, sw, err)
    assert np.array_equal(rt.dsp_apply(np.zeros(n, np.float32), normalize=True), np.zeros(n, np.float32))


@pytest.mark.parametrize("n", D.LENGTHS)
def test_blocked_recurrence_is_the_sequential_one_to_one_f32_step(pkg, n):
    rt = pkg.runtime
    x = D.signal(n, seed=7)
    seq = rt.dsp_apply(x, dc_block=True)
    blk = rt.dsp_blocked_host(x)
    diff = np.abs(blk.astype(np.float64) - seq.astype(np.float64))
    bound = D.dc_bound(seq)
    print(f"blocked vs sequential n={n}: max diff {diff.max():.3e} = {diff.max() / bound:.3f} steps at the peak, {np.count_nonzero(diff)} of {n} samples differ")
    assert diff.max() <= bound, (n, float(diff.max()), bound)
    if n > 4000:                                       # the filter did run: the offset is gone from the tail
        assert abs(float(seq[n // 2:].mean())) < 0.02 and abs(float(blk[n // 2:].mean())) < 0.02
    assert np.array_equal(blk[:min(n, 30)].view(np.uint32), seq[:min(n, 30)].view(np.uint32))   # the first run starts from the same zero state


def test_request_keeps_its_size_and_dsp_sits_where_reserved2_sat(pkg, tmp_path):
    rt = pkg.runtime
    assert C.sizeof(rt._Request) == 176 and rt._Request.dsp.offset == rt._Request.sample_rate.offset + 4 == 168
    assert C.sizeof(rt.DspOpts) == 40 and rt.DspOpts.fade_in_ms.offset == 8 and rt.DspOpts.reserved.offset == 24
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_request), '
                   'offsetof(ptts_request, dsp), offsetof(ptts_request, sample_rate), sizeof(ptts_dsp_opts), offsetof(ptts_dsp_opts, reserved)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == [C.sizeof(rt._Request), rt._Request.dsp.offset, rt._Request.sample_rate.offset, C.sizeof(rt.DspOpts), rt.DspOpts.reserved.offset], out


def test_symbols(pkg):
    rt = pkg.runtime
    assert "ptts_dsp_rows" in rt.ABI_SYMBOLS and hasattr(rt.lib(), "ptts_dsp_rows")
    assert "ptts_debug_dsp_blocked_host" in rt.HOOK_SYMBOLS and not hasattr(rt.lib(), "ptts_debug_dsp_blocked_host")
