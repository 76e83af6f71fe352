"""CPU-side checks of the loudness normalisation (go-pocket-tts_amd/csrc/loudness.cpp, scan_block.h): ptts_loudness --
the blocked float64 evaluation the device kernels run, instantiated for the host -- against the sequential BS.1770-4 restatement of _loudness_ref.py;
the K-weighting coefficients against the standard's 48 kHz table; the rows that stay as they are; ptts_request kept its size and `loudness` sits
where reserved[1] sat."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _loudness_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [9600, 9601, 11999, 12000, 240000, 487680]
# library against yardstick: both are float64 evaluations of one linear system and one sum; rounding at n <= 5e5 terms bounds the relative
# error of the mean square near 1e-10 = 1e-9 dB, so 1e-6 LU leaves three orders of margin
PARITY_BOUND = 1e-6
GATE_MARGIN = 1e-3   # no block of a test input lies this close (LU) to a gate: a gate decision cannot flip between the two evaluations


def _signals():
    out = [("sine 997 Hz 0 dBFS", L.sine(997.0, 1.0, 10.0)), ("sine 1 kHz -20 dBFS", L.sine(1000.0, 0.1, 10.0)), ("sine 440 Hz 0.5, 3 s", L.sine(440.0, 0.5, 3.0)),
           ("gated noise", L.gated_noise())]
    return out + [(f"ragged {n}", L.ragged(n)) for n in RAGGED]


def test_kweighting_reproduces_the_bs1770_table_at_48_khz(pkg):
    got = pkg.runtime.kweighting(48000)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, 1.0, -2.0, 1.0, -1.99004745483398]
    for g, w in zip(got[:9], table):
        assert abs(g - w) <= 1e-12, (g, w)
    # the table's high-pass a2 is 0.99004745483398; the bilinear form gives 0.990072250366 -- a known difference, and the form is the definition
    assert abs(got[9] - 0.990072250366) <= 1e-12 and abs(got[9] - 0.99004745483398) > 1e-5
    (sb, sa), (hb, ha) = L.kweighting(48000)
    ref = np.concatenate([sb, sa[1:], hb, ha[1:]])
    assert np.abs(ref - got).max() <= 1e-15
    (sb, sa), (hb, ha) = L.kweighting(24000)
    assert np.abs(np.concatenate([sb, sa[1:], hb, ha[1:]]) - pkg.runtime.kweighting(24000)).max() <= 1e-15


def test_meter_reference_tones(pkg):
    """EBU Tech 3341's meter tolerance, +-0.1 LU, around the values of a full-scale and a -20 dBFS sine."""
    rt = pkg.runtime
    a = rt.loudness(L.sine(997.0, 1.0, 10.0))
    b = rt.loudness(L.sine(1000.0, 0.1, 10.0))
    print(f"997 Hz 0 dBFS: {a:.4f} LUFS (yardstick {L.loudness(L.sine(997.0, 1.0, 10.0)):.4f}); 1 kHz -20 dBFS: {b:.4f} LUFS")
    assert abs(a - -3.01) <= 0.1 and abs(b - -23.0) <= 0.1


def test_library_is_the_yardstick_to_1e_6_lu(pkg):
    rt = pkg.runtime
    worst = 0.0
    rows = []
    for name, x in _signals():
        margin = L.gate_margin(x)
        assert margin > GATE_MARGIN, (name, margin)        # asserted on the yardstick alone
        want, got = L.loudness(x), rt.loudness(x)
        d = abs(got - want)
        print(f"{name}: library {got:.9f} LUFS, yardstick {want:.9f}, |diff| {d:.3e} LU, nearest block to a gate {margin:.3f} LU")
        assert math.isfinite(want) and d <= PARITY_BOUND, (name, got, want)
        worst = max(worst, d)
        rows.append({"case": name, "abs_diff_lu": d})
    # the noise case exercises the relative gate: blocks pass the absolute gate and fail the relative one
    z, l, m_abs, rel = L.gates(L.gated_noise())
    assert int((m_abs & ~(l > rel)).sum()) >= 1 and int((~m_abs).sum()) >= 1
    out = os.environ.get("PTTS_LOUDNESS_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps({"case": "max", "abs_diff_lu": worst}) + "\n")


def test_rows_with_nothing_above_the_gates_stay_as_they_are(pkg):
    rt = pkg.runtime
    quiet = (L.ragged(48000) * 1e-4).astype(np.float32)
    assert L.loudness(quiet) == -math.inf and float(np.abs(quiet).max()) > 0
    for x in (L.ragged(9599), np.zeros(30000, np.float32), quiet, np.zeros(0, np.float32), L.ragged(1)):
        assert rt.loudness(x) == -math.inf
        y, m = rt.loudness_normalize(x, -16.0)
        assert m == -math.inf and np.array_equal(y.view(np.uint32), x.view(np.uint32))
    nan = L.ragged(24000).copy()
    nan[100] = np.nan                                        # every block's energy is NaN: no block passes a gate
    y, m = rt.loudness_normalize(nan, -16.0)
    assert m == -math.inf and np.array_equal(y.view(np.uint32), nan.view(np.uint32))
    for bad in (-70.5, -0.5, 3.0, float("nan")):
        with pytest.raises(pkg.PttsError) as ei:
            rt.loudness_normalize(L.ragged(12000), bad)
        assert ei.value.code == rt.PTTS_EINVAL and "loudness" in str(ei.value)


def test_normalised_audio_measures_at_the_target(pkg):
    """Targets the signal reaches without the ceiling: the yardstick measures the output at the target within 1e-4 LU (the f32 gain rounds at
    2^-24 = 5e-7 dB, the samples' own f32 rounding averages out over a block)."""
    rt = pkg.runtime
    for name, x in _signals():
        for target in (-23.0, -16.0, -30.5):
            before = L.loudness(x)
            peak = float(np.abs(x).max())
            if peak * 10.0 ** ((target - before) / 20.0) > 0.99:   # the ceiling would bind
                continue
            y, m = rt.loudness_normalize(x, target)
            after = L.loudness(y)
            print(f"{name} -> {target}: measured {m:.6f}, output {after:.7f} LUFS")
            assert abs(m - before) <= PARITY_BOUND and abs(after - target) <= 1e-4, (name, target, after)
    x = L.sine(997.0, 0.5, 10.0)                             # the ceiling: -1 LUFS is out of reach, the gain stops at 1 / peak
    y, _ = rt.loudness_normalize(x, -1.0)
    assert np.array_equal(y.view(np.uint32), rt.dsp_apply(x, normalize=True).view(np.uint32)) and float(np.abs(y).max()) == 1.0


def test_energies_hook_is_the_k_weighted_energy(pkg):
    rt = pkg.runtime
    x = L.ragged(12345)
    e = rt.loudness_energies(x)
    y = L.kweighted(x)
    want = (y[: e.size * 480] ** 2).reshape(-1, 480).sum(axis=1)
    assert e.size == 12345 // 480 and np.abs(e / want - 1.0).max() <= 1e-9
    assert rt.loudness_energies(L.ragged(479)).size == 0


def test_request_keeps_its_size_and_loudness_sits_where_reserved_sat(pkg, tmp_path):
    rt = pkg.runtime
    assert C.sizeof(rt._Request) == 176 and rt._Request.loudness.offset == rt._Request.noise_rows.offset + 4 == 140
    assert rt._Request.pcm_callback.offset == 144 and rt._Request.dsp.offset == 168
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_request), '
                   'offsetof(ptts_request, loudness), offsetof(ptts_request, noise_rows), offsetof(ptts_request, pcm_callback), offsetof(ptts_request, dsp)); '
                   'return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == [176, 140, 136, 144, 168], out


def test_symbols(pkg):
    rt = pkg.runtime
    for s in ("ptts_loudness", "ptts_loudness_normalize", "ptts_loudness_rows", "ptts_loudness_normalize_rows"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    for s in ("ptts_debug_loudness_energies", "ptts_debug_kweighting"):
        assert s in rt.HOOK_SYMBOLS and not hasattr(rt.lib(), s), s
