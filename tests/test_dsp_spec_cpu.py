"""CPU-side checks of what the host-rows entry points and a request's post-processing share (go-pocket-tts_amd/csrc/dsp_spec.{h,cpp}, host_rows.h):
a ptts_dsp_opts is resolved into a DspSpec without a handle's memory being read before the registry knows it, dsp_active agrees with the spec, and
rows are packed without overlap.  A stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")

SANITIZER_MAIN = r'''
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include "dsp_spec.h"
#include "host_rows.h"
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
// every field of a resolved spec against what is expected, and any() against dsp_active
static bool is(const ptts_dsp_opts* o, bool nz, bool dc, double fi, double fo, const EqScan* eq, bool tp, float ceiling) {
    DspSpec s;
    s.loud = true;                                              // (the resolver starts from an all-off spec, whatever it is handed)
    if (!dsp_resolve(o, &s).empty()) return false;
    const bool on = nz || dc || fi > 0 || fo > 0 || eq || tp;
    return s.normalize == nz && s.dc_block == dc && s.fade_in_ms == fi && s.fade_out_ms == fo && s.eq == eq && s.true_peak == tp && s.ceiling == ceiling &&
           !s.loud && s.target_power == 0.0 && s.any() == on && dsp_active(o) == on && (!o || dsp_opts_error(*o).empty());
}
static ptts_dsp_opts off() { ptts_dsp_opts o = ptts_dsp_opts(); return o; }

static int resolver() {
    const ptts_eq_section sec = {PTTS_EQ_HIGHPASS, 0, 80.0, 0.0, 0.7071};
    ptts_eq* eq = nullptr;
    CHECK(ptts_eq_create(&sec, 1, &eq) == PTTS_OK && eq);
    ptts_dsp_ext_opts xo = {sizeof(ptts_dsp_ext_opts), 1, -6.0};
    ptts_dsp_ext *tp = nullptr, *quiet = nullptr;
    CHECK(ptts_dsp_ext_create(&xo, &tp) == PTTS_OK && tp);
    xo.true_peak = 0;
    CHECK(ptts_dsp_ext_create(&xo, &quiet) == PTTS_OK && quiet);
    const float c = tp_ceiling(-6.0);
    // nothing, and every switch alone
    CHECK(is(nullptr, false, false, 0, 0, nullptr, false, 1.0f));
    ptts_dsp_opts o = off();
    CHECK(is(&o, false, false, 0, 0, nullptr, false, 1.0f));
    o = off(); o.normalize = 1;        CHECK(is(&o, true, false, 0, 0, nullptr, false, 1.0f));
    o = off(); o.dc_block = 1;         CHECK(is(&o, false, true, 0, 0, nullptr, false, 1.0f));
    o = off(); o.fade_in_ms = 12.5;    CHECK(is(&o, false, false, 12.5, 0, nullptr, false, 1.0f));
    o = off(); o.fade_out_ms = 33.0;   CHECK(is(&o, false, false, 0, 33.0, nullptr, false, 1.0f));
    o = off(); o.eq = eq;              CHECK(is(&o, false, false, 0, 0, &eq->sc, false, 1.0f));       // the equaliser by pointer
    o = off(); o.ext = tp;             CHECK(is(&o, false, false, 0, 0, nullptr, true, c));           // the ceiling by value
    o = off(); o.ext = quiet;          CHECK(is(&o, false, false, 0, 0, nullptr, false, c));          // a live handle that switches nothing on
    o = off(); o.normalize = 1; o.dc_block = 1; o.fade_in_ms = 50; o.fade_out_ms = 80; o.eq = eq; o.ext = tp;
    CHECK(is(&o, true, true, 50, 80, &eq->sc, true, c));
    // the loudness of a row is the caller's to add
    DspSpec s;
    CHECK(!s.any());
    s.loud = true;
    CHECK(s.any());
    // fades
    const double bad[3] = {-1.0, -1e-300, std::nan("")};
    for (double v : bad) {
        o = off(); o.fade_in_ms = v;
        CHECK(has(dsp_resolve(&o, &s), "dsp: fade_in_ms") && has(dsp_opts_error(o), "is negative or not a number") && !dsp_active(&o));
        o = off(); o.fade_out_ms = v;
        CHECK(has(dsp_resolve(&o, &s), "dsp: fade_out_ms") && has(dsp_opts_error(o), "is negative or not a number") && !dsp_active(&o));
    }
    // a handle of the other kind: looked up with its kind, refused
    o = off(); o.eq = reinterpret_cast<const ptts_eq*>(tp);
    CHECK(has(dsp_resolve(&o, &s), "dsp: eq") && has(dsp_opts_error(o), "is not a live handle of ptts_eq_create") && dsp_active(&o));
    o = off(); o.ext = reinterpret_cast<const ptts_dsp_ext*>(eq);
    CHECK(has(dsp_resolve(&o, &s), "dsp: ext") && has(dsp_opts_error(o), "(reserved[2..3]) is not a live handle of ptts_dsp_ext_create") && !dsp_active(&o));
    // freed handles: the memory is gone, and the sanitizer reports any read of it
    ptts_eq_free(eq);
    ptts_dsp_ext_free(tp);
    o = off(); o.eq = eq;
    CHECK(has(dsp_resolve(&o, &s), "dsp: eq") && has(dsp_opts_error(o), "is not a live handle of ptts_eq_create"));
    CHECK(dsp_active(&o));                                      // an eq counts unseen: the row is refused where it is resolved
    o = off(); o.ext = tp;
    CHECK(has(dsp_resolve(&o, &s), "dsp: ext") && has(dsp_opts_error(o), "(reserved[2..3]) is not a live handle of ptts_dsp_ext_create"));
    CHECK(!dsp_active(&o));                                     // an ext that is not live counts for nothing
    o = off(); o.normalize = 1; o.ext = tp;
    CHECK(has(dsp_resolve(&o, &s), "dsp: ext") && dsp_active(&o));
    ptts_dsp_ext_free(quiet);
    return 0;
}

static int planner() {
    const size_t sizes[6] = {0, 1, 255, 256, 257, 4 * 1921};
    for (int masked = 0; masked < 2; masked++) {
        for (unsigned mask = 0; mask < (masked ? 64u : 1u); mask++) {
            bool skip[6];
            size_t off[6], want = 0;
            for (int i = 0; i < 6; i++) {
                skip[i] = (mask >> i) & 1;
                if (!skip[i]) want += (sizes[i] + 255) / 256 * 256;
            }
            const size_t total = pack_rows(sizes, masked ? skip : nullptr, 6, off);
            CHECK(total == want);                               // the sum of the rounded sizes; a skipped row takes no bytes
            size_t end = 0;
            for (int i = 0; i < 6; i++) {
                CHECK(off[i] % 256 == 0 && off[i] >= end && off[i] <= total);   // aligned, behind every row in front of it
                if (!skip[i]) { end = off[i] + sizes[i]; CHECK(end <= total); }
            }
        }
    }
    size_t none = 7;
    CHECK(pack_rows(nullptr, nullptr, 0, &none) == 0 && none == 7);
    return 0;
}

int main() {
    if (resolver() || planner()) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_resolver_and_row_packing_are_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/dsp_spec.cpp, eq.cpp and true_peak.cpp, built with g++ -fsanitize=address,undefined and run as a subprocess."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    main = tmp_path / "dsp_spec_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "dsp_spec_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main)] + [os.path.join(CSRC, f) for f in ("dsp_spec.cpp", "eq.cpp", "true_peak.cpp")] + ["-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
