"""CPU-side checks of per-part prosody for the join (include/ptts.h ptts_part_opts, ptts_join_parts_length, ptts_join_parts,
ptts_join_parts_stream_ready; go-pocket-tts_amd/csrc/join.{h,cpp}): the struct's layout; the symbols; refusals that name
the field and the part; ptts_join_parts against the numpy restatement of _join_parts_ref.py, bit for bit, with mixed per-seam modes and gains; a
list of defaults against ptts_join; NaN payloads through a part without a gain; the level rows; and a stand-alone program over join.cpp under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _join_parts_ref as R
import _join_ref as J
import _loudness_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")
FIELDS = ("size", "level", "trim", "pitch", "formant", "tempo", "gain_db", "gap_ms", "crossfade_ms")
OFFSETS = [0, 4, 8, 16, 24, 32, 40, 48, 56]
SYMBOLS = ("ptts_join_parts_length", "ptts_join_parts", "ptts_join_parts_rows", "ptts_join_parts_stream_ready", "ptts_generate_joined_parts")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _opts(rt, pairs, gains_db, levels=None):
    return [rt.PartOpts(gain_db=db, gap_ms=g, crossfade_ms=c, level=(levels[i] if levels else 0)) for i, ((g, c), db) in enumerate(zip(pairs, gains_db))]


def test_symbols_and_layout(pkg, tmp_path):
    rt = pkg.runtime
    for s in SYMBOLS:
        assert s in rt.ABI_SYMBOLS and hasattr(rt.lib(), s), s
    P = rt.PartOpts
    assert C.sizeof(P) == 64 and [getattr(P, f).offset for f in FIELDS] == OFFSETS
    assert P().size == 64 and P().gap_ms < 0 and P().crossfade_ms < 0 and P().gain_db == 0.0 and P().level == 0
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptts.h"\n#define P(f) offsetof(ptts_part_opts, f)\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptts_part_opts), ' + ", ".join("P(%s)" % f for f in FIELDS) +
                   '); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [64] + OFFSETS


@pytest.fixture(scope="module")
def cases():
    """(order, shift) -> (parts, seam pairs, gains in dB, the restatement's audio and gains): computed once, never written to."""
    out = {}
    for oi, lengths in enumerate(J.ORDERS):
        parts = J.parts_for(lengths, seed=20 + oi)
        for p in parts:
            p.setflags(write=False)
        for shift in range(3):
            pairs, gains_db = R.cycle(len(lengths), shift)
            default = (37.5, 0.0) if shift == 1 else (0.0, 10.0) if shift == 2 else (0.0, 0.0)
            ref, g = R.statement(parts, pairs, gains_db, default)
            ref.setflags(write=False)
            out[(oi, shift)] = (parts, pairs, gains_db, default, ref, g)
    return out


@pytest.mark.parametrize("shift", range(3))
def test_join_parts_is_the_numpy_statement_bit_for_bit(pkg, cases, shift):
    rt = pkg.runtime
    seen_gap = seen_fade = seen_gain_at_fade = False
    for oi, lengths in enumerate(J.ORDERS):
        parts, pairs, gains_db, default, ref, g_ref = cases[(oi, shift)]
        o = rt.JoinOpts(gap_ms=default[0], crossfade_ms=default[1])
        po = _opts(rt, pairs, gains_db)
        got, g = rt.join_parts(parts, po, o, gains=True)
        seams = [R.seam_pair(a, b, default) for a, b in pairs]
        offs, total = R.offsets(lengths, seams)
        assert got.dtype == np.float32 and got.size == ref.size == total, (lengths, shift)
        assert np.array_equal(_u32(got), _u32(ref)), (lengths, shift, int((_u32(got) != _u32(ref)).sum()))
        assert np.array_equal(_u32(g), _u32(g_ref)), (lengths, shift)
        n, o_got = rt.join_parts_length(lengths, po, o, offsets=True)
        assert n == total and o_got.tolist() == offs, (lengths, shift)
        assert not np.array_equal(_u32(got[:min(got.size, ref.size)]), _u32(J.join(parts)[:min(got.size, ref.size)])) or total == 0
        for i in range(len(lengths) - 1):
            k = J.seam(seams[i][1], lengths[i], lengths[i + 1])
            seen_gap |= seams[i][0] > 0
            seen_fade |= k > 0
            seen_gain_at_fade |= k > 0 and (gains_db[i] != 0.0 or gains_db[i + 1] != 0.0)
    assert seen_gap and seen_fade and seen_gain_at_fade   # the cycles reach every kind of seam, a crossfade with a gain beside it among them


def test_a_list_of_defaults_is_ptts_join(pkg):
    rt = pkg.runtime
    for oi, lengths in enumerate(J.ORDERS):
        parts = J.parts_for(lengths, seed=40 + oi)
        for mode in J.MODES:
            o = rt.JoinOpts(**mode)
            got, g = rt.join_parts(parts, [rt.PartOpts() for _ in parts], o, gains=True)
            assert np.array_equal(_u32(got), _u32(rt.join(parts, o))), (lengths, mode)
            assert np.array_equal(_u32(g), _u32(np.ones(len(parts), np.float32)))
            assert rt.join_parts_length(lengths, [rt.PartOpts() for _ in parts], o) == rt.join_length(lengths, o)


def test_a_part_without_a_gain_moves_nan_payloads_untouched(pkg):
    rt = pkg.runtime
    a, b, c = J.parts_for([1921, 5, 1920], seed=3)
    a[7], a[1920], b[0], c[1919] = np.nan, np.inf, -np.inf, np.nan
    _u32(a)[100] = 0x7FC12345                                  # a quiet NaN with a payload
    _u32(a)[101] = 0x7F812345                                  # a signalling one: a product would quiet it
    _u32(c)[0] = 0xFFFFFFFF
    po = [rt.PartOpts(gain_db=0.0, gap_ms=37.5), rt.PartOpts(gain_db=0.0, gap_ms=0.0), rt.PartOpts()]
    got = rt.join_parts([a, b, c], po)
    offs, _ = R.offsets([1921, 5, 1920], [(900, 0), (0, 0), (0, 0)])
    for p, off in zip((a, b, c), offs):
        assert np.array_equal(_u32(got[off:off + p.size]), _u32(p))
    assert _u32(got)[100] == 0x7FC12345 and _u32(got)[101] == 0x7F812345


def test_the_level_rows(pkg):
    """Each part at its own level: the part is what ptts_loudness_normalize makes of it.  The preconditions first, on the CPU (_join_parts_ref.py has
    the reasoning): every row's loudness is finite; the 10 Hz row at 0.9 needs more than 1 / peak to reach the target, the 440 Hz rows need less."""
    rt = pkg.runtime
    parts = R.level_parts()
    target = R.LEVEL_TARGET / 100.0
    lufs = [rt.loudness(p) for p in parts]
    assert all(np.isfinite(v) for v in lufs), lufs
    for p, v in zip(parts, lufs):                              # the independent float64 measurement agrees
        assert abs(LR.loudness(p) - v) < 0.05, (LR.loudness(p), v)
    want = [10.0 ** ((target - v) / 20.0) for v in lufs]
    ceil = [np.float32(1.0) / np.abs(p).max() for p in parts]
    assert want[2] > 1.05 * ceil[2] and want[0] < 0.95 * ceil[0] and want[1] < 0.95 * ceil[1], (want, ceil)
    po = [rt.PartOpts(level=R.LEVEL_TARGET, gap_ms=0.0), rt.PartOpts(level=R.LEVEL_TARGET, crossfade_ms=10.0), rt.PartOpts(level=R.LEVEL_TARGET)]
    got, g = rt.join_parts(parts, po, gains=True)
    assert _u32(g)[2] == _u32(ceil[2])                         # the 0.9 row's gain is the peak ceiling
    assert g[0] != 1.0 and g[1] != 1.0 and g[0] != ceil[0] and g[1] != ceil[1]
    assert abs(g[0] / want[0] - 1.0) < 1e-2 and abs(g[1] / want[1] - 1.0) < 1e-2
    levelled = [rt.loudness_normalize(p, target)[0] for p in parts]
    ref = R.join_parts(levelled, [(0, 0), (0, 240), (0, 0)], [None, None, None])
    assert np.array_equal(_u32(got), _u32(ref))
    assert not np.array_equal(_u32(got), _u32(rt.join_parts(parts, [rt.PartOpts(gap_ms=0.0), rt.PartOpts(crossfade_ms=10.0), rt.PartOpts()])))
    # a part in which no block passes the gates (shorter than 400 ms; silence) keeps its bits, its gain is 1
    short = [parts[0][:9599].copy(), np.zeros(14400, np.float32)]
    got, g = rt.join_parts(short, [rt.PartOpts(level=R.LEVEL_TARGET), rt.PartOpts(level=R.LEVEL_TARGET)], gains=True)
    assert g.tolist() == [1.0, 1.0] and np.array_equal(_u32(got), _u32(np.concatenate(short)))


def test_stream_ready_takes_the_seam_behind_the_last_part(pkg):
    rt = pkg.runtime
    o = rt.JoinOpts(crossfade_ms=10.0)
    assert rt.join_parts_stream_ready(o, rt.PartOpts(), 50000) == rt.join_stream_ready(o, 50000) == (50000 - 240) // 1920 * 1920
    assert rt.join_parts_stream_ready(o, rt.PartOpts(crossfade_ms=100.0), 50000) == (50000 - 2400) // 1920 * 1920
    assert rt.join_parts_stream_ready(o, rt.PartOpts(gap_ms=5.0), 50000) == 50000 // 1920 * 1920
    with pytest.raises(pkg.PttsError) as ei:
        rt.join_parts_stream_ready(o, rt.PartOpts(), -1)
    assert "negative" in str(ei.value)


def test_refusals_name_the_field_and_the_part(pkg):
    rt = pkg.runtime
    L = rt.lib()
    nan, inf = float("nan"), float("inf")
    x = np.ones(8, np.float32)

    def refused(po, *words, call=None):
        for f in ([lambda: rt.join_parts([x] * len(po), po), lambda: rt.join_parts_length([8] * len(po), po)] if call is None else [call]):
            with pytest.raises(pkg.PttsError) as ei:
                f()
            assert ei.value.code == rt.PTTS_EINVAL and all(w in str(ei.value) for w in words + ("join: parts",)), (words, str(ei.value))

    ok = rt.PartOpts
    for field, values in (("gap_ms", (2000.5, nan, inf)), ("crossfade_ms", (2001.0, nan, inf))):
        for v in values:
            refused([ok(), ok(), ok(**{field: v})], field, "part 2")    # the last part's fields are range-checked too
            refused([ok(), ok(**{field: v}), ok()], field, "part 1")
    refused([ok(gap_ms=1.0, crossfade_ms=1.0), ok()], "gap_ms", "crossfade_ms", "both", "part 0")
    for v in (-60.5, 24.01, nan, inf, -inf):                            # the volume fields: only where they are read
        refused([ok(), ok(gain_db=v)], "gain_db", "part 1", call=lambda v=v: rt.join_parts([x, x], [ok(), ok(gain_db=v)]))
        assert rt.join_parts_length([8, 8], [ok(), ok(gain_db=v)]) == 16
    for v in (-7001, -99, 5):
        refused([ok(level=v), ok()], "level", "part 0", call=lambda v=v: rt.join_parts([x, x], [ok(level=v), ok()]))
    refused([ok(), ok(), ok(level=-1600, gain_db=3.0)], "level", "gain_db", "part 2", call=lambda: rt.join_parts([x] * 3, [ok(), ok(), ok(level=-1600, gain_db=3.0)]))
    for v in (-60.0, 24.0):                                             # the edges of the box are inside it
        assert rt.join_parts([x], [ok(gain_db=v)]).size == 8
    for v in (0.0, 2000.0):
        assert rt.join_parts_length([8, 8], [ok(gap_ms=v), ok()]) == 16 + J.samples(v)
        assert rt.join_parts_length([8, 8], [ok(crossfade_ms=v), ok()]) == 16 - min(J.samples(v), 4)
    assert rt.join_parts_length([8, 8], [ok(gap_ms=-inf, crossfade_ms=-1.0), ok()], rt.JoinOpts(gap_ms=1.0)) == 16 + 24   # both negative: the options' pair
    assert rt.join_parts_length([8, 8], [ok(gap_ms=-inf, crossfade_ms=0.0), ok()], rt.JoinOpts(gap_ms=1.0)) == 16        # one negative: 0
    # sizes: smaller than the known fields; elements that disagree; bytes beyond the known ones
    refused([ok(size=56), ok(size=56)], "size", "part 0")
    refused([ok(), ok(size=72)], "size", "part 1")

    class Wide(C.Structure):   # a caller compiled against a later header: sixteen more bytes behind the fields this library knows
        _fields_ = [("o", C.c_uint8 * 64), ("tail", C.c_uint8 * 16)]

    wide = (Wide * 2)()
    for i, gap in enumerate((1.0, -1.0)):
        C.memmove(C.byref(wide[i]), C.byref(ok(gap_ms=gap, size=80)), 64)
    ns = np.array([8, 8], np.int64)
    o = rt.JoinOpts()
    call = lambda: int(L.ptts_join_parts_length(ns.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.byref(o), C.cast(wide, C.POINTER(rt.PartOpts)), None))  # noqa: E731
    assert call() == 16 + 24                                            # the elements lie `size` bytes apart
    wide[1].tail[3] = 1
    assert call() == -rt.PTTS_EINVAL and "size" in L.ptts_last_error().decode() and "part 1" in L.ptts_last_error().decode()
    # the list is required; what ptts_join refuses is refused in its words
    assert int(L.ptts_join_parts_length(ns.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.byref(o), None, None)) == -rt.PTTS_EINVAL
    assert "null list" in L.ptts_last_error().decode()
    with pytest.raises(pkg.PttsError) as ei:
        rt.join_parts([x, x], [ok(), ok()], rt.JoinOpts(gap_ms=1.0, crossfade_ms=1.0))
    assert "both" in str(ei.value) and "parts" not in str(ei.value)
    # the device entry points refuse a model that is not there before anything else
    reqs, res = (rt._Request * 1)(), rt._Result()
    po = (rt.PartOpts * 2)(ok(), ok())
    for rc in (L.ptts_generate_joined_parts(None, reqs, 1, C.byref(o), po, None, C.byref(res), None, None),
               L.ptts_join_parts_rows(None, None, ns.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.byref(o), po, None, None)):
        assert rc == rt.PTTS_EINVAL and ("model" in L.ptts_last_error().decode() or "runtime unavailable" in L.ptts_last_error().decode())
    assert L.ptts_generate_joined_parts(None, reqs, 1, C.byref(o), None, None, C.byref(res), None, None) == rt.PTTS_EINVAL
    assert "null list" in L.ptts_last_error().decode()


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
// loudness.cpp stays out of this program: ptts_join_parts is join_parts_run with its measurement, here a stand-in that reads every sample of the part
static float level_gain(const float* x, int64_t n, double) {
    float peak = 0.0f;
    for (int64_t i = 0; i < n; i++) peak = std::fmax(peak, std::fabs(x[i]));
    return peak > 0.0f ? 0.5f / peak : 1.0f;
}
static int join_parts(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, float* out, float* gains) {
    return join_parts_run(in, n, rows, o, po, out, gains, level_gain);
}
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (%s)\n", __LINE__, #c, ptts::g_err.c_str()); return 1; } } while (0)
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static ptts_join_opts opts(double gap_ms, double crossfade_ms) {
    ptts_join_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = sizeof o; o.gap_ms = gap_ms; o.crossfade_ms = crossfade_ms;
    return o;
}
static ptts_part_opts part(double gain_db, int level, double gap_ms, double crossfade_ms) {
    ptts_part_opts p;
    std::memset(&p, 0, sizeof p);
    p.size = sizeof p; p.gain_db = gain_db; p.level = level; p.gap_ms = gap_ms; p.crossfade_ms = crossfade_ms;
    return p;
}

// parts, the list and the joined row in blocks of exactly their size: a read or a write one element too far is reported
static int one(const std::vector<long>& len, int shift, double gap_ms, double crossfade_ms) {
    static const double seams[8][2] = {{-1, -1}, {0, -1}, {37.5, -1}, {-1, 10}, {0.05, 0}, {-5, 2000}, {0, 0.1}, {2000, -3}};
    static const double gains[8] = {0, -6, 3, 0, 0, -60, 24, 0.5};
    const ptts_join_opts o = opts(gap_ms, crossfade_ms);
    const int rows = (int)len.size();
    std::vector<float*> in((size_t)rows);
    std::vector<int64_t> n((size_t)rows), off((size_t)rows);
    ptts_part_opts* po = static_cast<ptts_part_opts*>(std::malloc((size_t)rows * sizeof(ptts_part_opts)));
    float* g = static_cast<float*>(std::malloc((size_t)rows * sizeof(float)));
    for (int i = 0; i < rows; i++) {
        n[(size_t)i] = len[(size_t)i];
        in[(size_t)i] = len[(size_t)i] ? static_cast<float*>(std::malloc((size_t)len[(size_t)i] * sizeof(float))) : nullptr;
        for (long j = 0; j < len[(size_t)i]; j++) in[(size_t)i][j] = (float)(i + 1);
        const int s = (i + shift) % 8, v = (i + 2 * shift) % 8;
        po[i] = part(v == 3 ? 0.0 : gains[v], v == 3 ? -1600 : 0, seams[s][0], seams[s][1]);
    }
    const int64_t total = ptts_join_parts_length(n.data(), rows, &o, po, off.data());
    CHECK(total >= 0);
    float* out = static_cast<float*>(std::malloc(total ? (size_t)total * sizeof(float) : 1));
    CHECK(out);
    for (int64_t q = 0; q < total; q++) out[q] = -7.0f;
    CHECK(join_parts(in.data(), n.data(), rows, &o, po, total ? out : nullptr, g) == PTTS_OK);
    // parts are constants 1, 2, 3 ... times a gain of at most 24 dB: nothing keeps the fill, nothing is negative or beyond the loudest part
    for (int64_t q = 0; q < total; q++) CHECK(out[q] >= 0.0f && out[q] <= 16.0f * (float)rows);
    for (int i = 0; i < rows; i++) CHECK(g[i] > 0.0f && g[i] < 16.0f);
    CHECK(off[0] == 0);
    CHECK(ptts_join_parts_stream_ready(&o, po + rows - 1, total) >= 0);
    for (int i = 0; i < rows; i++) std::free(in[(size_t)i]);
    std::free(out); std::free(po); std::free(g);
    return 0;
}

int main() {
    const std::vector<std::vector<long>> orders = {{0, 1, 3, 5, 1920, 1921, 4801}, {4801, 1921, 1920, 5, 3, 1, 0}, {4801, 0, 1, 1921, 0, 3, 1920, 5},
                                                   {0, 0, 1920, 1, 4801, 3, 1921, 5, 0}, {5, 4801, 3, 1920, 1, 1921}, {0}, {1}, {0, 0}};
    for (const auto& len : orders)
        for (int shift = 0; shift < 8; shift++) {
            if (one(len, shift, 0.0, 0.0)) return 1;
            if (one(len, shift, 37.5, 0.0)) return 1;
            if (one(len, shift, 0.0, 10.0)) return 1;
        }
    const int64_t n2[2] = {4, 4};
    const ptts_join_opts o = opts(0.0, 0.0);
    ptts_part_opts po[2] = {part(0, 0, 1.0, 1.0), part(0, 0, -1, -1)};
    CHECK(ptts_join_parts_length(n2, 2, &o, po, nullptr) == -PTTS_EINVAL && has(g_err, "both") && has(g_err, "part 0"));
    po[0] = part(0, 0, -1, -1); po[1] = part(30.0, 0, -1, -1);
    CHECK(ptts_join_parts_length(n2, 2, &o, po, nullptr) == 8);
    float out[8];
    const float a[4] = {1, 1, 1, 1};
    const float* in[2] = {a, a};
    CHECK(join_parts(in, n2, 2, &o, po, out, nullptr) == PTTS_EINVAL && has(g_err, "gain_db") && has(g_err, "part 1"));
    CHECK(ptts_join_parts_length(n2, 2, &o, nullptr, nullptr) == -PTTS_EINVAL && has(g_err, "null"));
    CHECK(ptts_join_parts_length(n2, 0, &o, po, nullptr) == -PTTS_EINVAL && has(g_err, "rows"));
    po[1].size = 8;
    CHECK(ptts_join_parts_length(n2, 2, &o, po, nullptr) == -PTTS_EINVAL && has(g_err, "size"));
    std::printf("ok\n");
    return 0;
}
'''


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/join.cpp alone (ptts_join_parts is its join_parts_run with loudness.cpp's measurement handed in), built with g++ -fsanitize=address,undefined and run as a subprocess, over the shapes of the
    tests above.  Nothing loaded into Python is sanitised."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for lib in ("libasan.a", "libubsan.a"):   # asked before anything is built: a build that fails is a failure
        if not os.path.isabs(subprocess.run(["g++", "-print-file-name=" + lib], capture_output=True, text=True).stdout.strip()):
            pytest.skip(f"the sanitizer runtime {lib} is not installed")
    main = tmp_path / "join_parts_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "join_parts_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), os.path.join(CSRC, "join.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
