"""CPU-side checks of the two things every stage of the post-processing chain shares on the host (go-pocket-tts_amd/csrc/row_tables.h, dsp_spec.h):
the rule that cuts a list of rows into tables of at most 256 rows and 16 distinct designs, and the plan that gives each stage of a row its part
of the scratch buffer.  A stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go-pocket-tts_amd", "csrc")

SANITIZER_MAIN = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp_spec.h"
#include "row_tables.h"
using namespace ptts;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Design { double a; int32_t b, pad; };
static bool by_value(const Design& x, const Design& y) { return std::memcmp(&x, &y, sizeof x) == 0; }
static bool by_identity(const Design& x, const Design& y) { return &x == &y; }

struct Table { size_t first; int count; std::vector<int32_t> index; std::vector<const Design*> designs; };
template <class Same>
static std::vector<Table> cut(const std::vector<const Design*>& key, int max_rows, int max_designs, Same same) {
    std::vector<Table> out;
    cut_tables(key, max_rows, max_designs, same, [&](size_t first, int count, const int32_t* index, const std::vector<const Design*>& designs) {
        out.push_back(Table{first, count, std::vector<int32_t>(index, index + count), designs});
    });
    return out;
}
// the tables cover the rows in order, within both limits, and every row's index names a design that is the row's own
template <class Same>
static bool sound(const std::vector<Table>& t, const std::vector<const Design*>& key, int max_rows, int max_designs, Same same) {
    size_t at = 0;
    for (const Table& x : t) {
        if (x.first != at || x.count < 1 || x.count > max_rows || (int)x.designs.size() > max_designs || (int)x.index.size() != x.count) return false;
        for (int k = 0; k < x.count; k++) {
            const Design* d = key[at + (size_t)k];
            if (!d) { if (x.index[(size_t)k] != 0) return false; continue; }
            if (x.index[(size_t)k] < 0 || (size_t)x.index[(size_t)k] >= x.designs.size() || !same(*x.designs[(size_t)x.index[(size_t)k]], *d)) return false;
        }
        at += (size_t)x.count;
    }
    return at == key.size();
}

static int tables() {
    constexpr int kRows = 256, kDesigns = 16;
    std::vector<Design> d(17);
    for (int i = 0; i < 17; i++) d[(size_t)i] = Design{1.0 + i, i, 0};
    std::vector<const Design*> key;
    // no rows: no table
    CHECK(cut(key, kRows, kDesigns, by_value).empty());
    // one row: one table
    key.assign(1, &d[3]);
    std::vector<Table> t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 1 && t[0].first == 0 && t[0].count == 1 && t[0].designs.size() == 1 && t[0].designs[0] == &d[3] && t[0].index[0] == 0);
    // 256 rows of one design: one table; 257: tables of 256 and 1
    key.assign(256, &d[0]);
    t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 1 && t[0].count == 256 && t[0].designs.size() == 1 && sound(t, key, kRows, kDesigns, by_value));
    key.assign(257, &d[0]);
    t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 2 && t[0].count == 256 && t[1].first == 256 && t[1].count == 1 && t[1].designs.size() == 1 && sound(t, key, kRows, kDesigns, by_value));
    // 257 rows cycling through 17 designs: the 17th design starts the next table every time, so sixteen tables of 16 rows and one of 1
    key.clear();
    for (int i = 0; i < 257; i++) key.push_back(&d[(size_t)(i % 17)]);
    for (int pass = 0; pass < 2; pass++) {
        t = pass ? cut(key, kRows, kDesigns, by_identity) : cut(key, kRows, kDesigns, by_value);
        CHECK(t.size() == 17 && sound(t, key, kRows, kDesigns, by_value));
        for (size_t k = 0; k < 17; k++) {
            CHECK(t[k].first == 16 * k && t[k].count == (k < 16 ? 16 : 1) && t[k].designs.size() == (size_t)t[k].count);
            for (int j = 0; j < t[k].count; j++) {   // first-use order: the table's j-th design is its j-th row's, and the row's index is j
                CHECK(t[k].designs[(size_t)j] == key[t[k].first + (size_t)j] && t[k].index[(size_t)j] == j);
            }
        }
    }
    // two designs equal by value at different addresses: one index under the value predicate, two under the identity predicate
    Design twin_a = Design{2.5, 7, 0}, twin_b = Design{2.5, 7, 0};
    key = {&twin_a, &twin_b, &twin_a};
    t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 1 && t[0].designs.size() == 1 && t[0].designs[0] == &twin_a && t[0].index == (std::vector<int32_t>{0, 0, 0}));
    t = cut(key, kRows, kDesigns, by_identity);
    CHECK(t.size() == 1 && t[0].designs.size() == 2 && t[0].designs[1] == &twin_b && t[0].index == (std::vector<int32_t>{0, 1, 0}));
    // the 17th design arriving at row 255 leaves a table of 255 rows, not 256
    key.clear();
    for (int i = 0; i < 255; i++) key.push_back(&d[(size_t)(i % 16)]);
    key.push_back(&d[16]);
    key.push_back(&d[0]);
    t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 2 && t[0].count == 255 && t[0].designs.size() == 16 && t[1].first == 255 && t[1].count == 2 && t[1].designs.size() == 2 &&
          t[1].designs[0] == &d[16] && t[1].designs[1] == &d[0] && sound(t, key, kRows, kDesigns, by_value));
    // rows without a design fit any table, take index 0 and bring no design
    key.assign(300, nullptr);
    for (int i = 0; i < 17; i++) key[(size_t)(10 * i)] = &d[(size_t)i];
    t = cut(key, kRows, kDesigns, by_value);
    CHECK(t.size() == 2 && t[0].count == 160 && t[0].designs.size() == 16 && t[1].count == 140 && t[1].designs.size() == 1 && sound(t, key, kRows, kDesigns, by_value));
    return 0;
}

// What each stage's region held before there was a plan, restated: the expressions that sized and carved the scratch buffer
static size_t tiles_of(int64_t n) { return (size_t)((n + 1919) / 1920); }
static size_t want_cmp(int64_t n) { return 2 * (tiles_of(n) * 2 * 1); }                        // cmp_state_doubles: two recurrences of scan_state_doubles<1>
static size_t want_dc(int64_t n) { return tiles_of(n) * 2 * 2; }                               // scan_state_doubles<2>
static size_t want_loud(int64_t n) { return 2 + tiles_of(n) * 2 * 4 + tiles_of(n) * 4; }       // loud_doubles: head, scan_state_doubles<4>, four sub-blocks a tile
static size_t want_eq(int64_t n, int S) { return tiles_of(n) * 4 * (size_t)S; }                // tiles * 4 * S
static size_t want_lim(int64_t n) { return tiles_of(n) * 2 * 1 + (size_t)((n + 1) / 2); }      // lim_scratch_doubles: scan_state_doubles<1>, then one f32 a sample

static int scratch() {
    const int64_t lengths[6] = {0, 1, 1919, 1920, 1921, 9601};
    EqScan eq{};
    for (int S = 1; S <= kEqMaxSections; S += kEqMaxSections - 1) {
        eq.S = S;
        for (int apply = 0; apply < 2; apply++) {
            for (unsigned mask = 0; mask < 32; mask++) {
                DspSpec sp;
                sp.compress = mask & 1; sp.dc_block = mask & 2; sp.loud = mask & 4; sp.eq = (mask & 8) ? &eq : nullptr; sp.limit = mask & 16;
                // the six rows of one call, each row's regions behind the row in front: every region inside the total, none overlapping another
                size_t total = 0, end = 0;
                for (int64_t n : lengths) total += dsp_scratch(sp, n, apply != 0).total();
                size_t row_at = 0;
                for (int64_t n : lengths) {
                    const DspScratch q = dsp_scratch(sp, n, apply != 0);
                    const size_t at[5] = {q.cmp_at(), q.dc_at(), q.loud_at(), q.eq_at(), q.lim_at()}, size[5] = {q.cmp, q.dc, q.loud, q.eq, q.lim};
                    for (int k = 0; k < 5; k++) {
                        CHECK(row_at + at[k] >= end && row_at + at[k] + size[k] <= total && at[k] + size[k] <= q.total());
                        end = row_at + at[k] + size[k];
                    }
                    row_at += q.total();
                    // no stage gets less than it got; a stage that is off, or that a measurement alone does not run, gets nothing
                    const bool on = n > 0;
                    CHECK(q.cmp == (on && sp.compress && apply ? want_cmp(n) : 0));
                    CHECK(q.dc == (on && sp.dc_block ? want_dc(n) : 0));
                    CHECK(q.loud == (on && sp.loud ? want_loud(n) : 0));
                    CHECK(q.eq == (on && sp.eq && apply ? want_eq(n, S) : 0));
                    CHECK(q.lim == (on && sp.limit && apply ? want_lim(n) : 0));
                }
                CHECK(row_at == total && end <= total);
            }
        }
    }
    return 0;
}

int main() {
    if (tables() || scratch()) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_table_cuts_and_scratch_plan_are_clean_under_sanitizers(tmp_path):
    """A stand-alone program over csrc/row_tables.h and dsp_spec.h alone, built with g++ -fsanitize=address,undefined and run as a subprocess."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    main = tmp_path / "row_tables_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "row_tables_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",   # the runtimes inside the program: it does not depend on what else the process loads first
           "-I", CSRC, str(main), "-o", str(exe), "-pthread"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and not run.stderr.strip(), (run.returncode, run.stdout, run.stderr)
