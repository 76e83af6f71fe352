"""CPU-side checks of the join of a text's parts (include/ptts.h ptts_join_opts, ptts_join_part, ptts_join_length, ptts_join;
go-pocket-tts_amd/csrc/join.{h,cpp}): the structs' layouts; ptts_join against the numpy restatement of _join_ref.py, bit
for bit, plain, with gaps and with crossfades; NaN and infinity through a plain copy; lengths and offsets; refusals that name what was wrong;
and a stand-alone program over join.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _join_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in ("ptts_join_length", "ptts_join", "ptts_join_rows", "ptts_generate_joined"):
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    O, P = rt.JoinOpts, rt.JoinPart
    assert C.sizeof(O) == 40 and [getattr(O, f).offset for f in ("size", "pcm_format", "sample_rate", "loudness", "dsp", "gap_ms", "crossfade_ms")] == [0, 4, 8, 12, 16, 24, 32]
    assert C.sizeof(P) == 32 and [getattr(P, f).offset for f in ("offset", "n_samples", "n_frames", "eos_step", "status", "reserved")] == [0, 8, 16, 20, 24, 28]
    assert O().size == 40
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#define O(f) offsetof(ptts_join_opts, f)\n#define P(f) offsetof(ptts_join_part, f)\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptts_join_opts), O(size), O(pcm_format), O(sample_rate), O(loudness), O(dsp), '
                   'O(gap_ms), O(crossfade_ms));\n printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptts_join_part), P(offset), P(n_samples), P(n_frames), P(eos_step), '
                   'P(status), P(reserved)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [40, 0, 4, 8, 12, 16, 24, 32, 32, 0, 8, 16, 20, 24, 28]


@pytest.fixture(scope="module")
def cases():
    """(lengths, mode) -> (parts, the reference): computed once, never written to."""
    out = {}
    for oi, lengths in enumerate(J.ORDERS):
        parts = J.parts_for(lengths, seed=oi)
        for p in parts:
            p.setflags(write=False)
        for mi, mode in enumerate(J.MODES):
            ref = J.join(parts, **mode)
            ref.setflags(write=False)
            out[(oi, mi)] = (parts, ref)
    return out


@pytest.mark.parametrize("mi", range(len(J.MODES)), ids=[("plain" if not m else "%s=%g" % next(iter(m.items()))) for m in J.MODES])
def test_join_is_the_numpy_statement_bit_for_bit(pkg, cases, mi):
    rt = pkg.runtime
    mode = J.MODES[mi]
    for oi, lengths in enumerate(J.ORDERS):
        parts, ref = cases[(oi, mi)]
        o = rt.JoinOpts(**mode)
        got = rt.join(parts, o)
        offs, total = J.offsets(lengths, **mode)
        assert got.dtype == np.float32 and got.size == ref.size == total, (lengths, mode)
        assert np.array_equal(_u32(got), _u32(ref)), (lengths, mode, int((_u32(got) != _u32(ref)).sum()))
        n, o_got = rt.join_length(lengths, o, offsets=True)
        assert n == total and o_got.tolist() == offs, (lengths, mode)
    # the seam lengths that the orders reach: the whole K, K clamped by either neighbour, and none
    if "crossfade_ms" in mode:
        K = J.samples(mode["crossfade_ms"])
        seams = {J.seam(K, a, b) for lengths in J.ORDERS for a, b in zip(lengths, lengths[1:])}
        assert 0 in seams and (K >= 2400 or K in seams) and (K < 240 or any(0 < s < K for s in seams)), (K, sorted(seams))


def test_a_crossfade_is_the_two_fades_of_dsp_apply(pkg):
    """The seam is ptts_dsp_apply's fade out of the tail plus its fade in of the head: the host functions agree with each other, not only with numpy."""
    rt = pkg.runtime
    a, b = J.parts_for([4801, 1921], seed=7)
    K = 240
    got = rt.join([a, b], rt.JoinOpts(crossfade_ms=10.0))
    tail = rt.dsp_apply(a[-K:], fade_out_ms=10.0)
    head = rt.dsp_apply(b[:K], fade_in_ms=10.0)
    assert np.array_equal(_u32(got[4801 - K:4801]), _u32(tail + head))
    assert np.array_equal(_u32(got[:4801 - K]), _u32(a[:-K])) and np.array_equal(_u32(got[4801:]), _u32(b[K:]))


def test_nan_and_inf_pass_a_plain_copy(pkg):
    rt = pkg.runtime
    a, b, c = J.parts_for([1921, 5, 1920], seed=3)
    a[7], a[1920], b[0], c[1919] = np.nan, np.inf, -np.inf, np.nan
    _u32(a)[100] = 0x7FC12345                                  # a NaN with a payload
    _u32(c)[0] = 0xFFFFFFFF
    for mode in (dict(), dict(gap_ms=37.5)):
        got = rt.join([a, b, c], rt.JoinOpts(**mode))
        assert np.array_equal(_u32(got), _u32(J.join([a, b, c], **mode))), mode
        offs, _ = J.offsets([1921, 5, 1920], **mode)
        for p, off in zip((a, b, c), offs):
            assert np.array_equal(_u32(got[off:off + p.size]), _u32(p))
        assert int(np.isnan(got).sum()) == 4 and int(np.isinf(got).sum()) == 2


def _length_raw(rt, n, rows, o):
    ns = np.ascontiguousarray(n, np.int64)
    rc = rt.lib().ptts_join_length(ns.ctypes.data_as(C.POINTER(C.c_int64)), rows, C.byref(o) if o is not None else None, None)
    return int(rc), rt.lib().ptts_last_error().decode(errors="replace")


class _Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
    _fields_ = [("o", C.c_uint8 * 40), ("tail", C.c_uint8 * 16)]


def test_refusals_name_what_is_wrong(pkg):
    rt = pkg.runtime
    L = rt.lib()
    nan, inf = float("nan"), float("inf")
    x = np.ones(8, np.float32)
    for field, values in (("gap_ms", (-0.1, 2000.5, nan, inf)), ("crossfade_ms", (-1.0, 2001.0, nan, -inf))):
        for v in values:
            for call in (lambda o: rt.join([x, x], o), lambda o: rt.join_length([8, 8], o)):
                with pytest.raises(pkg.PttsError) as ei:
                    call(rt.JoinOpts(**{field: v}))
                assert ei.value.code == rt.PTTS_EINVAL and field in str(ei.value) and "join" in str(ei.value), (field, v, str(ei.value))
    with pytest.raises(pkg.PttsError) as ei:
        rt.join([x, x], rt.JoinOpts(gap_ms=1.0, crossfade_ms=1.0))
    assert "gap_ms" in str(ei.value) and "crossfade_ms" in str(ei.value) and "both" in str(ei.value)
    for v in (0.0, 2000.0):                                    # every edge of the box is inside it
        assert rt.join_length([8, 8], rt.JoinOpts(gap_ms=v)) == 16 + J.samples(v)
        assert rt.join_length([8, 8], rt.JoinOpts(crossfade_ms=v)) == 16 - min(J.samples(v), 4)
    for size in (0, 32, 39):
        with pytest.raises(pkg.PttsError) as ei:
            rt.join([x], rt.JoinOpts(size=size))
        assert ei.value.code == rt.PTTS_EINVAL and "size" in str(ei.value)
    wide = _Wide()                                             # zeros beyond what the library knows are "off", anything else is refused
    C.memmove(C.byref(wide), C.byref(rt.JoinOpts(gap_ms=1.0, size=56)), 40)
    ns = np.array([8, 8], np.int64)
    call = lambda: int(L.ptts_join_length(ns.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.cast(C.byref(wide), C.POINTER(rt.JoinOpts)), None))  # noqa: E731
    assert call() == 16 + 24
    for at in (0, 15):
        wide.tail[at] = 1
        assert call() == -rt.PTTS_EINVAL and "size" in L.ptts_last_error().decode()
        wide.tail[at] = 0
    # rows from 1 to 4096, a joined length below 2^31, lengths that are not negative, options that are there
    for rows in (0, 4097, -1):
        rc, msg = _length_raw(rt, np.zeros(max(rows, 1), np.int64), rows, rt.JoinOpts())
        assert rc == -rt.PTTS_EINVAL and "rows" in msg and "4096" in msg, (rows, msg)
    assert _length_raw(rt, np.ones(4096, np.int64), 4096, rt.JoinOpts())[0] == 4096
    rc, msg = _length_raw(rt, [2 ** 30, 2 ** 30], 2, rt.JoinOpts())
    assert rc == -rt.PTTS_EINVAL and "2^31" in msg, msg
    assert _length_raw(rt, [2 ** 30, 2 ** 30 - 1], 2, rt.JoinOpts())[0] == 2 ** 31 - 1
    rc, msg = _length_raw(rt, [2 ** 31 - 1000, 0], 2, rt.JoinOpts(gap_ms=2000.0))
    assert rc == -rt.PTTS_EINVAL and "2^31" in msg, msg
    rc, msg = _length_raw(rt, [4, -1], 2, rt.JoinOpts())
    assert rc == -rt.PTTS_EINVAL and "negative" in msg, msg
    rc, msg = _length_raw(rt, [4, 4], 2, None)
    assert rc == -rt.PTTS_EINVAL and "null options" in msg, msg
    # the device entry points refuse a model that is not there before anything else
    reqs, res = (rt._Request * 1)(), rt._Result()
    for rc in (L.ptts_generate_joined(None, reqs, 1, C.byref(rt.JoinOpts()), C.byref(res), None),
               L.ptts_join_rows(None, None, ns.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.byref(rt.JoinOpts()), None)):
        assert rc == rt.PTTS_EINVAL and ("model" in L.ptts_last_error().decode() or "runtime unavailable" in L.ptts_last_error().decode())


def test_service_with_a_dispatcher_refuses_joined_calls(pkg):
    svc = pkg.Service(None, lambda s: [1], dispatcher=object())
    with pytest.raises(pkg.PttsError) as ei:
        svc.synthesize_joined("Hello.")
    assert "dispatcher" in str(ei.value)


SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "join.h"
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

static ptts_join_opts opts(double gap_ms, double crossfade_ms) {
    ptts_join_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = sizeof o; o.gap_ms = gap_ms; o.crossfade_ms = crossfade_ms;
    return o;
}

// parts and the joined row in blocks of exactly their size: a read or a write one sample too far is reported
static int one(const std::vector<long>& len, double gap_ms, double crossfade_ms) {
    const ptts_join_opts o = opts(gap_ms, crossfade_ms);
    const int rows = (int)len.size();
    std::vector<float*> in((size_t)rows);
    std::vector<int64_t> n((size_t)rows), off((size_t)rows);
    for (int i = 0; i < rows; i++) {
        n[(size_t)i] = len[(size_t)i];
        in[(size_t)i] = len[(size_t)i] ? static_cast<float*>(std::malloc((size_t)len[(size_t)i] * sizeof(float))) : nullptr;
        for (long j = 0; j < len[(size_t)i]; j++) in[(size_t)i][j] = (float)(i + 1);
    }
    const int64_t total = ptts_join_length(n.data(), rows, &o, off.data());
    CHECK(total >= 0);
    float* out = static_cast<float*>(std::malloc(total ? (size_t)total * sizeof(float) : 1));
    CHECK(out);
    for (int64_t q = 0; q < total; q++) out[q] = -7.0f;
    CHECK(ptts_join(in.data(), n.data(), rows, &o, total ? out : nullptr) == PTTS_OK);
    // parts are constants 1, 2, 3 ...: a gap is 0, a seam lies between its neighbours' values (the two weights sum to (K - 1) / K), nothing keeps the fill
    for (int64_t q = 0; q < total; q++) CHECK(out[q] >= 0.0f && out[q] <= (float)rows);
    for (int i = 0; i < rows; i++)
        if (n[(size_t)i] > 0 && crossfade_ms == 0.0) CHECK(out[off[(size_t)i]] == (float)(i + 1) && out[off[(size_t)i] + n[(size_t)i] - 1] == (float)(i + 1));
    CHECK(off[0] == 0);
    for (int i = 0; i < rows; i++) std::free(in[(size_t)i]);
    std::free(out);
    return 0;
}

int main() {
    const std::vector<std::vector<long>> orders = {{0, 1, 3, 5, 1920, 1921, 4801}, {4801, 1921, 1920, 5, 3, 1, 0}, {4801, 0, 1, 1921, 0, 3, 1920, 5},
                                                   {0, 0, 1920, 1, 4801, 3, 1921, 5, 0}, {5, 4801, 3, 1920, 1, 1921}, {0}, {1}, {0, 0}};
    const double gaps[4] = {0.0, 0.05, 37.5, 2000.0}, fades[3] = {0.1, 10.0, 2000.0};
    for (const auto& len : orders) {
        for (double g : gaps) if (one(len, g, 0.0)) return 1;
        for (double c : fades) if (one(len, 0.0, c)) return 1;
    }
    const int64_t n2[2] = {4, 4};
    ptts_join_opts o = opts(1.0, 1.0);
    CHECK(ptts_join_length(n2, 2, &o, nullptr) == -PTTS_EINVAL && has(g_err, "both"));
    o = opts(0.0, 0.0);
    CHECK(ptts_join_length(n2, 0, &o, nullptr) == -PTTS_EINVAL && has(g_err, "rows"));
    CHECK(ptts_join_length(n2, 4097, &o, nullptr) == -PTTS_EINVAL && has(g_err, "rows"));
    CHECK(ptts_join_length(nullptr, 2, &o, nullptr) == -PTTS_EINVAL && has(g_err, "null"));
    CHECK(ptts_join(nullptr, n2, 2, &o, nullptr) == PTTS_EINVAL && has(g_err, "null"));
    o.size = 8;
    CHECK(ptts_join_length(n2, 2, &o, nullptr) == -PTTS_EINVAL && has(g_err, "size"));
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/join.cpp alone, built with g++ -fsanitize=address,undefined and run as a subprocess.  Nothing loaded into
    Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "join_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "join_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), os.path.join(CSRC, "join.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
