"""CPU-side checks of streamed joined synthesis (include/ptts.h ptts_join_stream_opts, ptts_generate_joined_streamed, ptts_join_stream_ready;
go-pocket-tts_amd/csrc/join.{h,cpp}): the struct's layout; where the new symbols live; ptts_join_stream_ready against a
numpy statement of its formula; the size rules of the stream options, refused before a model is asked for."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1920


def test_layout(pkg, tmp_path):
    S = pkg.runtime.JoinStreamOpts
    assert C.sizeof(S) == 24 and [getattr(S, f).offset for f in ("size", "first_group", "pcm_callback", "pcm_user")] == [0, 4, 8, 16]
    assert S().size == 24 and S(first_group=3).first_group == 3
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#define S(f) offsetof(ptts_join_stream_opts, f)\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ptts_join_stream_opts), S(size), S(first_group), S(pcm_callback), S(pcm_user));\n'
                   ' printf("%zu\\n", sizeof(ptts_join_opts)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [24, 0, 4, 8, 16, 40]


def test_symbols(pkg):
    rt = pkg.runtime
    product = C.CDLL(rt.LIB_PATH)
    for s in ("ptts_generate_joined_streamed", "ptts_join_stream_ready"):
        assert s in rt.ABI_SYMBOLS and hasattr(product, s), s
    assert "ptts_debug_dsp_windows" in rt.HOOK_SYMBOLS and "ptts_debug_dsp_windows" not in rt.ABI_SYMBOLS
    assert not hasattr(product, "ptts_debug_dsp_windows")
    assert hasattr(C.CDLL(rt.HOOKS_PATH), "ptts_debug_dsp_windows")


def _samples(ms):
    return int(np.float64(ms) / np.float64(1000.0) * np.float64(24000.0))   # (int64)(ms / 1000 * 24000)


def _ready(joined, crossfade_ms, fade_out_ms):
    hold = max(_samples(crossfade_ms), _samples(fade_out_ms) if fade_out_ms > 0 else 0)
    return max(0, joined - hold) // TILE * TILE, hold


JOINED = [0, 1, 1919, 1920, 1921, 1920 * 7 + 5, 2 ** 31 - 1]


@pytest.mark.parametrize("mode", [dict(gap_ms=37.5), dict(crossfade_ms=10.0), dict(crossfade_ms=2000.0)], ids=lambda m: "%s=%g" % next(iter(m.items())))
@pytest.mark.parametrize("fade_out_ms", [0.0, 80.0, 2000.0])
def test_ready_is_the_numpy_statement(pkg, mode, fade_out_ms):
    rt = pkg.runtime
    dsp = rt.DspOpts(0, 0, 0.0, fade_out_ms) if fade_out_ms > 0 else None
    o = rt.JoinOpts(dsp=dsp, **mode)
    got = []
    for joined in JOINED:
        want, hold = _ready(joined, mode.get("crossfade_ms", 0.0), fade_out_ms)
        r = rt.join_stream_ready(o, joined)
        assert r == want, (mode, fade_out_ms, joined, r, want)
        assert r % TILE == 0 and (r == 0 or r <= joined - hold), (joined, r, hold)
        got.append(r)
    assert got == sorted(got)                                               # monotone in `joined`
    # ... and between the listed values: every boundary of a tile around the hold-back
    _, hold = _ready(0, mode.get("crossfade_ms", 0.0), fade_out_ms)
    prev = 0
    for joined in range(max(0, hold - 2), hold + 3 * TILE + 2, 7):
        r = rt.join_stream_ready(o, joined)
        assert r == _ready(joined, mode.get("crossfade_ms", 0.0), fade_out_ms)[0] and r >= prev
        prev = r
    assert rt.join_stream_ready(o, hold + TILE - 1) == 0 and rt.join_stream_ready(o, hold + TILE) == TILE
    # a gap holds nothing back by itself; a dsp without a fade out neither
    if "gap_ms" in mode and fade_out_ms == 0.0:
        assert rt.join_stream_ready(o, 1920) == 1920 and rt.join_stream_ready(rt.JoinOpts(dsp=rt.DspOpts(0, 1, 50.0, 0.0), **mode), 3840) == 3840


def test_ready_refuses_bad_arguments(pkg):
    rt = pkg.runtime
    L = rt.lib()
    for o, word in ((rt.JoinOpts(gap_ms=1.0, crossfade_ms=1.0), "both"), (rt.JoinOpts(size=8), "size"), (rt.JoinOpts(crossfade_ms=2000.5), "crossfade_ms")):
        with pytest.raises(pkg.PttsError) as ei:
            rt.join_stream_ready(o, 1920)
        assert ei.value.code == rt.PTTS_EINVAL and word in str(ei.value)
    assert int(L.ptts_join_stream_ready(None, 5)) == -rt.PTTS_EINVAL and "null options" in L.ptts_last_error().decode()
    assert int(L.ptts_join_stream_ready(C.byref(rt.JoinOpts()), -1)) == -rt.PTTS_EINVAL and "negative" in L.ptts_last_error().decode()


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 24), ("tail", C.c_uint8 * 16)]


def test_size_rules_need_no_gpu(pkg):
    """The stream options are checked before the model is asked for: a NULL model is reached only by options that are well formed."""
    rt = pkg.runtime
    L = rt.lib()
    reqs, res = (rt._Request * 1)(), rt._Result()

    def call(so):
        rc = L.ptts_generate_joined_streamed(None, reqs, 1, C.byref(rt.JoinOpts()), so, C.byref(res), None)
        return int(rc), L.ptts_last_error().decode(errors="replace")

    for size in (0, 8, 23):
        rc, msg = call(C.byref(rt.JoinStreamOpts(size=size)))
        assert rc == rt.PTTS_EINVAL and "size" in msg and "stream" in msg, (size, msg)
    rc, msg = call(None)
    assert rc == rt.PTTS_EINVAL and "stream" in msg and "null options" in msg, msg
    rc, msg = call(C.byref(rt.JoinStreamOpts(first_group=-1)))
    assert rc == rt.PTTS_EINVAL and "first_group" in msg, msg
    wide = _Wide()
    C.memmove(C.byref(wide), C.byref(rt.JoinStreamOpts(first_group=2, size=40)), 24)
    as_opts = C.cast(C.byref(wide), C.POINTER(rt.JoinStreamOpts))
    rc, msg = call(as_opts)                                                 # zeros beyond what the library knows are "off": the model is asked for next
    assert rc == rt.PTTS_EINVAL and "size" not in msg and ("model" in msg or "runtime unavailable" in msg), msg
    for at in (0, 15):
        wide.tail[at] = 1
        rc, msg = call(as_opts)
        assert rc == rt.PTTS_EINVAL and "size" in msg, (at, msg)
        wide.tail[at] = 0
    rc, msg = call(C.byref(rt.JoinStreamOpts()))                            # well formed: refused for the model alone
    assert rc == rt.PTTS_EINVAL and ("model" in msg or "runtime unavailable" in msg), msg


def test_service_with_a_dispatcher_refuses_streamed_joined_calls(pkg):
    svc = pkg.Service(None, lambda s: [1], dispatcher=object())
    with pytest.raises(pkg.PttsError) as ei:
        svc.synthesize_joined("Hello.", pcm_callback=lambda off, x: None, first_group=1)
    assert "dispatcher" in str(ei.value)
