// dsp_device.cpp -- the host side of the device post-processing (dsp.hip, compressor.hip, deesser.hip, limiter.hip, true_peak.hip):
// the order of the chain's stages, their row tables (cut by row_tables.h's rule) and scratch (planned by dsp_spec.h's dsp_scratch), their
// launches, and the round trip of host rows through them.  The coefficients come from dsp.cpp (dsp_scan_coeffs), made as dsp_dc_block makes
// them; what a row gets is resolved in dsp_spec.cpp.  At the end: the tables of k_join (join.hip) and the round trip of ptts_join_rows, then the part
// stages of a joined call -- the trim (trim.hip), the pitch (pitch.hip, with its one table image per model; formant.hip around it for the rows
// that keep their formants) and the tempo (tempo.hip): their table builders, the one chain that runs them in that order (parts_launch) and the
// one round trip of host rows through it (part_rows_device).
#include <cmath>

#include "row_tables.h"
#include "runtime.h"
#include "scan_block.h"

namespace ptts {

namespace {
int64_t fade_samples(double ms, int64_t n) {   // dsp_fade_in / dsp_fade_out: min((int64)(ms / 1000 * 24000), n)
    if (!(ms > 0)) return 0;
    const double f = ms / 1000.0 * (double)kNativeRate;
    return f >= (double)n ? n : (int64_t)f;
}

// the tiles a row's launch covers: its window's where the record has one (kernels.h), else the row's
template <class Row> int64_t row_tiles(const Row& r) { return scan_tiles(r.n); }
int64_t row_tiles(const DspRow& r) { return win_tiles(r.t0, r.n); }
int64_t row_tiles(const CmpRow& r) { return win_tiles(r.t0, r.n); }

// The tables of one stage (row_tables.h has the rule): rows, in order, into up to kRows rows with up to max_designs distinct designs a table,
// which travel behind the rows in the same turn of the ring.  key[i]: row i's design (null: none); index: where a row names its own among its
// table's.  launch(first, count, rows_dev, max_tiles, designs_dev) runs between the turn's stage() and done().  stage: the name in the refusal
template <class Row, size_t kTail, class Design, class Same, class Launch>
void launch_tables(RowRing<Row, kTail>& ring, std::vector<Row>& rows, const std::vector<const Design*>& key, int max_designs, Same&& same,
                   int32_t Row::*index, const char* stage, hipStream_t s, Launch&& launch) {
    std::vector<Design> designs;
    cut_tables(key, RowRing<Row, kTail>::kRows, max_designs, same, [&](size_t first, int n, const int32_t* at, const std::vector<const Design*>& distinct) {
        int64_t max_tiles = 0;
        for (int k = 0; k < n; k++) {
            rows[first + (size_t)k].*index = at[k];
            max_tiles = std::max(max_tiles, row_tiles(rows[first + (size_t)k]));
        }
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, strfmt("ptts-hip: %s: too many samples for one launch", stage));
        designs.clear();
        for (const Design* d : distinct) designs.push_back(*d);
        const void* designs_dev = nullptr;
        const Row* rows_dev = ring.stage(rows.data() + first, n, s, designs.data(), designs.size() * sizeof(Design), &designs_dev);
        launch(first, n, rows_dev, (int)max_tiles, static_cast<const Design*>(designs_dev));
        ring.done(s);
    });
}

template <class Design>
bool same_bytes(const Design& a, const Design& b) { return std::memcmp(&a, &b, sizeof a) == 0; }   // a design by value: compressors, de-essers, limiters
}  // namespace

// The chain's order, all of it: the compressor's tables, then the de-esser's, in front of everything that measures or rewrites a row; then, DSP table by DSP table,
// launch_dsp's kernels, the limiter's tables for that table's limiter rows (behind the fades, in front of the ceiling) and the true-peak pair
// on what all of them stored.  A measurement alone (apply false) rewrites nothing: no compressor, no de-esser, no equaliser, no limiter, k_tp_peak alone.
// A job with a window (DspJob::t0, open, carry; kernels.h has what a window is) takes the same way: its scratch is planned for the window's
// samples, its fade in counts in the whole row and its fade out waits for the window that closes the row.
void dsp_launch(Model& m, std::vector<DspJob>& jobs, hipStream_t s, bool apply) {
    static const DspScan scan = dsp_scan_coeffs(kNativeRate);
    if (jobs.empty()) return;
    // scratch: a peak word and a true-peak word per row, then what dsp_scratch (dsp_spec.h) gives each row's stages
    size_t tile_doubles = 0;
    for (const DspJob& j : jobs) tile_doubles += dsp_scratch(j.spec, j.n - j.t0 * kDspTile, apply).total();
    const size_t peak_bytes = (2 * jobs.size() * sizeof(uint32_t) + 255) & ~(size_t)255;   // [jobs] sample peaks, then [jobs] true peaks
    char* scratch = m.work(WORK_DSP_SCRATCH, peak_bytes + std::max<size_t>(tile_doubles, 1) * sizeof(double)).as<char>();
    uint32_t* peaks = reinterpret_cast<uint32_t*>(scratch);
    double* tiles = reinterpret_cast<double*>(scratch + peak_bytes);
    PTTS_HIP(hipMemsetAsync(peaks, 0, peak_bytes, s));
    std::vector<CmpRow> cmp_rows;
    std::vector<const CmpScan*> cmp_key;
    std::vector<DeRow> de_rows;
    std::vector<const DeScan*> de_key;
    std::vector<DspRow> rows;
    std::vector<const EqScan*> eq_key;       // per DSP row: its equaliser, where it is applied
    std::vector<const LimScan*> lim_key;     // per DSP row: its limiter, where it is applied
    std::vector<double*> lim_scratch;        // ... and that limiter's region
    rows.reserve(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) {
        DspJob& j = jobs[k];
        const DspSpec& sp = j.spec;
        j.loud_out = nullptr;
        j.tp_out = nullptr;
        const int64_t wn = j.n - j.t0 * kDspTile;   // the window's samples (a one-shot job: the row's)
        if (wn <= 0) continue;
        const DspScratch q = dsp_scratch(sp, wn, apply);
        double* const mine = tiles;   // the row's regions: mine + q.<stage>_at()
        tiles += q.total();
        if (q.cmp) {
            CmpRow r{};
            r.x = j.x; r.n = j.n;
            r.p_tiles = mine + q.cmp_at();
            r.s_tiles = r.p_tiles + scan_state_doubles<1>(scan_tiles(wn));
            r.open = j.open ? 1 : 0; r.t0 = j.t0; r.carry = j.carry;
            cmp_rows.push_back(r);
            cmp_key.push_back(&sp.cmp);
        }
        if (q.de) {
            if (j.t0 || j.open || j.carry) throw Error(PTTS_EINVAL, "ptts-hip: internal: the de-esser is not served window after window (dsp_window_refusal)");
            const int64_t F = scan_tiles(wn);
            DeRow r{};
            r.x = j.x; r.n = j.n;
            r.b_tiles = mine + q.de_at();
            r.p_tiles = r.b_tiles + scan_state_doubles<2>(F);
            r.s_tiles = r.p_tiles + scan_state_doubles<1>(F);
            de_rows.push_back(r);
            de_key.push_back(&sp.des);
        }
        if (!sp.rest()) continue;   // (a compressor or a de-esser alone: no row of the DSP table)
        DspRow r{};
        r.x = j.x; r.n = j.n;
        r.fade_in = fade_samples(sp.fade_in_ms, j.open ? j.n_row : j.n);   // (an open row: the length it will have, or one beyond every fade)
        r.fade_out = j.open ? 0 : fade_samples(sp.fade_out_ms, j.n);
        r.peak = peaks + k;
        r.flags = (sp.normalize ? DSP_NORMALIZE : 0) | (sp.dc_block ? DSP_DC : 0) | (sp.loud ? DSP_LOUD : 0) | (j.open ? DSP_OPEN : 0);
        r.t0 = j.t0; r.carry = j.carry;
        if (q.dc) r.tiles = mine + q.dc_at();
        if (q.loud) {
            r.loud = j.loud_out = mine + q.loud_at();
            r.target = sp.target_power;
        }
        if (q.eq) {
            r.flags |= DSP_EQ;
            r.eq_tiles = mine + q.eq_at();
        }
        if (sp.true_peak) {
            r.flags |= DSP_TP;
            r.tp = j.tp_out = peaks + jobs.size() + k;
            r.ceiling = sp.ceiling;
        }
        rows.push_back(r);
        eq_key.push_back(q.eq ? sp.eq : nullptr);
        lim_key.push_back(q.lim ? &sp.lim : nullptr);
        lim_scratch.push_back(mine + q.lim_at());
    }
    launch_tables(m.cmp_ring, cmp_rows, cmp_key, kCmpMaxDesigns, same_bytes<CmpScan>, &CmpRow::design, "compressor", s,
                  [&](size_t first, int n, const CmpRow* rows_dev, int max_tiles, const CmpScan* designs_dev) {
        bool any_open = false;
        for (size_t i = first; i < first + (size_t)n; i++) any_open = any_open || cmp_rows[i].open;
        launch_compressor(rows_dev, n, max_tiles, designs_dev, s, any_open);
    });
    launch_tables(m.de_ring, de_rows, de_key, kDeMaxDesigns, same_bytes<DeScan>, &DeRow::design, "deesser", s,
                  [&](size_t, int n, const DeRow* rows_dev, int max_tiles, const DeScan* designs_dev) { launch_deesser(rows_dev, n, max_tiles, designs_dev, s); });
    std::vector<LimRow> lim_rows;
    std::vector<const LimScan*> lim_rows_key;
    launch_tables(m.dsp_ring, rows, eq_key, kDspMaxEq, [](const EqScan& a, const EqScan& b) { return &a == &b; } /* a handle's identity */, &DspRow::eq, "dsp", s,
                  [&](size_t first, int n, const DspRow* rows_dev, int max_tiles, const EqScan* eqs_dev) {
        DspLaunch p{false, false, false, apply, &scan, &loud_scan()};
        p.eqs = eqs_dev;
        bool any_tp = false;
        lim_rows.clear();
        lim_rows_key.clear();
        for (size_t i = first; i < first + (size_t)n; i++) {
            const DspRow& r = rows[i];
            p.any_norm = p.any_norm || (r.flags & DSP_NORMALIZE);
            p.any_dc = p.any_dc || (r.flags & DSP_DC);
            p.any_loud = p.any_loud || (r.flags & DSP_LOUD);
            p.any_eq = p.any_eq || (r.flags & DSP_EQ);
            p.any_open = p.any_open || (r.flags & DSP_OPEN);
            any_tp = any_tp || (r.flags & DSP_TP);
            if (!lim_key[i]) continue;
            LimRow q{};
            q.x = r.x; q.n = r.n;
            q.p_tiles = lim_scratch[i];
            q.r = reinterpret_cast<float*>(lim_scratch[i] + scan_state_doubles<1>(scan_tiles(r.n)));
            lim_rows.push_back(q);
            lim_rows_key.push_back(lim_key[i]);
        }
        launch_dsp(rows_dev, n, max_tiles, p, s);
        launch_tables(m.lim_ring, lim_rows, lim_rows_key, kLimMaxDesigns, same_bytes<LimScan>, &LimRow::design, "limiter", s,
                      [&](size_t, int k, const LimRow* lim_dev, int lim_tiles, const LimScan* designs_dev) { launch_limiter(lim_dev, k, lim_tiles, designs_dev, s); });
        if (any_tp) {   // the last stage (true_peak.hip): on what the chain stored; a measurement alone does not scale
            launch_tp_peak(rows_dev, n, max_tiles, tp_taps(), s);
            if (apply) launch_tp_scale(rows_dev, n, max_tiles, s);
        }
    });
}

void dsp_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const DspSpec* per_row, bool apply, const DspRowsOut& o) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> bytes((size_t)rows);
    std::unique_ptr<bool[]> skip(new bool[(size_t)rows + 1]);
    for (int i = 0; i < rows; i++) {
        skip[(size_t)i] = n[i] <= 0 || !per_row[i].any();
        bytes[(size_t)i] = skip[(size_t)i] ? 0 : (size_t)n[i] * sizeof(float);
    }
    PackedRows buf(m, WORK_HOST_ROWS, std::move(bytes), skip.get());
    std::vector<DspJob> jobs;
    std::vector<int> job_row;
    for (int i = 0; i < rows; i++) {
        if (o.M) o.M[i] = 0.0;
        if (o.sub) o.sub[i].clear();
        if (o.true_peaks) o.true_peaks[i] = 0.0f;
        if (skip[(size_t)i]) {   // nothing to do on the device: a copy
            if (n[i] > 0 && o.out && o.out[i] != in[i]) std::memmove(o.out[i], in[i], (size_t)n[i] * sizeof(float));
            continue;
        }
        buf.upload(i, in[i], s);
        jobs.push_back(DspJob{(float*)buf.row(i), n[i], per_row[i]});
        job_row.push_back(i);
    }
    dsp_launch(m, jobs, s, apply);
    for (size_t k = 0; k < jobs.size(); k++) {
        const int i = job_row[k];
        const DspJob& j = jobs[k];
        if (o.M && j.loud_out) PTTS_HIP(hipMemcpyAsync(o.M + i, j.loud_out, sizeof(double), hipMemcpyDeviceToHost, s));
        if (o.sub && j.loud_out) {
            const int64_t F = scan_tiles(n[i]);
            o.sub[i].resize((size_t)F * kLoudSubsPerTile);
            PTTS_HIP(hipMemcpyAsync(o.sub[i].data(), loud_subs(j.loud_out, F), o.sub[i].size() * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        if (o.true_peaks && j.tp_out) PTTS_HIP(hipMemcpyAsync(o.true_peaks + i, j.tp_out, sizeof(float), hipMemcpyDeviceToHost, s));
        if (o.out) buf.download(i, o.out[i], s);
    }
    PTTS_HIP(hipStreamSynchronize(s));
}

// ptts_debug_dsp_windows: the rows uploaded whole, then one dsp_launch per window -- [prev, cut) of every row that has samples there, the row
// open where it goes on behind the cut -- and a last one to every row's end; the rows' carried states lie behind the rows, zeroed once
void dsp_windows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const DspSpec& spec, const int64_t* cuts, int32_t n_cuts, float* const* out) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> bytes((size_t)rows + 1);
    std::unique_ptr<bool[]> skip(new bool[(size_t)rows + 2]);
    for (int i = 0; i < rows; i++) {
        skip[(size_t)i] = n[i] <= 0;
        bytes[(size_t)i] = skip[(size_t)i] ? 0 : (size_t)n[i] * sizeof(float);
    }
    skip[(size_t)rows] = false;
    bytes[(size_t)rows] = (size_t)std::max(rows, 1) * kCarryDoubles * sizeof(double);
    PackedRows buf(m, WORK_HOST_ROWS, std::move(bytes), skip.get());
    double* const carry = reinterpret_cast<double*>(buf.row(rows));
    PTTS_HIP(hipMemsetAsync(carry, 0, (size_t)std::max(rows, 1) * kCarryDoubles * sizeof(double), s));
    for (int i = 0; i < rows; i++) if (n[i] > 0) buf.upload(i, in[i], s);
    int64_t prev = 0;
    for (int w = 0; w <= n_cuts; w++) {
        const int64_t cut = w < n_cuts ? cuts[w] : INT64_MAX;
        std::vector<DspJob> jobs;
        for (int i = 0; i < rows; i++) {
            if (n[i] <= prev) continue;   // the row ended in an earlier window, which closed it
            DspJob j{(float*)buf.row(i), std::min(n[i], cut), spec};
            j.t0 = prev / kDspTile; j.open = n[i] > cut; j.n_row = n[i]; j.carry = carry + (size_t)i * kCarryDoubles;
            jobs.push_back(j);
        }
        dsp_launch(m, jobs, s);
        prev = cut;
    }
    for (int i = 0; i < rows; i++) if (n[i] > 0) buf.download(i, out[i], s);
    PTTS_HIP(hipStreamSynchronize(s));
}

// ---- the join (join.hip; join.h has the rule) ----

void join_launch(Model& m, const std::vector<JoinRow>& rows, hipStream_t s) {
    constexpr int kRows = RowRing<JoinRow>::kRows;
    for (size_t at = 0; at < rows.size(); at += kRows) {
        const int n = (int)std::min<size_t>(kRows, rows.size() - at);
        int64_t tiles = 0;
        for (int i = 0; i < n; i++) {
            const JoinRow& r = rows[at + (size_t)i];
            if (r.gap + r.n > 0) tiles = std::max(tiles, (r.gap + r.n + 3 + kJoinTile - 1) / kJoinTile);
        }
        if (tiles == 0) continue;
        if (tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: join: too many samples for one launch");
        launch_join(m.join_ring.stage(rows.data() + at, n, s), n, (int)tiles, s);
        m.join_ring.done(s);
    }
}

void join_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const JoinLens& l, float* out) {
    std::vector<int64_t> off((size_t)rows), seam((size_t)rows);
    int64_t total = 0;
    const std::string e = join_plan(n, rows, l, off.data(), seam.data(), &total);
    if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
    if (total == 0) return;
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> bytes((size_t)rows + 1);
    for (int i = 0; i < rows; i++) bytes[(size_t)i] = (size_t)n[i] * sizeof(float);
    bytes[(size_t)rows] = (size_t)total * sizeof(float);   // the joined row, behind the parts
    PackedRows buf(m, WORK_HOST_ROWS, std::move(bytes));
    std::vector<JoinRow> jr;
    for (int i = 0; i < rows; i++) {
        if (n[i] > 0) buf.upload(i, in[i], s);
        const int64_t k = seam[(size_t)i], k_next = i + 1 < rows ? seam[(size_t)i + 1] : 0;
        JoinRow r{};
        r.src = (const float*)buf.row(i);
        r.prev = k ? (const float*)buf.row(i - 1) + (n[i - 1] - k) : nullptr;
        r.dst = (float*)buf.row(rows);
        r.off = off[(size_t)i];
        r.n = n[i] - k_next;
        r.k = (int32_t)k;
        r.gap = i ? (int32_t)l.gap : 0;
        jr.push_back(r);
    }
    join_launch(m, jr, s);
    buf.download(rows, out, s);
    PTTS_HIP(hipStreamSynchronize(s));
}

// ---- per-part options (include/ptts.h ptts_part_opts): the level's measuring launches, the gain form of the join ----

void level_launch(Model& m, const std::vector<const float*>& x, const std::vector<int64_t>& n, const std::vector<double>& target, std::vector<const float*>& words,
                  hipStream_t s) {
    const size_t R = x.size();
    words.assign(R, nullptr);
    size_t doubles = 0, live = 0;
    for (size_t i = 0; i < R; i++)
        if (n[i] > 0) { doubles += loud_doubles(scan_tiles(n[i])); live++; }
    if (!live) return;
    const size_t peak_bytes = (live * sizeof(uint32_t) + 255) & ~(size_t)255;
    char* scratch = m.work(WORK_PART_LEVEL, peak_bytes + doubles * sizeof(double)).as<char>();
    uint32_t* peaks = reinterpret_cast<uint32_t*>(scratch);
    double* loud = reinterpret_cast<double*>(scratch + peak_bytes);
    PTTS_HIP(hipMemsetAsync(peaks, 0, peak_bytes, s));
    std::vector<DspRow> rows;
    for (size_t i = 0; i < R; i++) {
        if (n[i] <= 0) continue;   // (an empty part: nothing passes the gates, its gain is 1)
        DspRow r{};
        r.x = const_cast<float*>(x[i]); r.n = n[i];   // the measuring kernels write nothing to x
        r.peak = peaks + rows.size();
        r.flags = DSP_LOUD;
        r.loud = loud;
        r.target = target[i];
        words[i] = reinterpret_cast<const float*>(loud + 1);
        loud += loud_doubles(scan_tiles(n[i]));
        rows.push_back(r);
    }
    constexpr size_t kRows = RowRing<DspRow, kDspMaxEq * kDspEqBytes>::kRows;
    static const DspScan scan = dsp_scan_coeffs(kNativeRate);
    for (size_t at = 0; at < rows.size(); at += kRows) {
        const int k = (int)std::min(kRows, rows.size() - at);
        int64_t tiles = 0;
        for (int i = 0; i < k; i++) tiles = std::max(tiles, scan_tiles(rows[at + (size_t)i].n));
        if (tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: join: parts: level: too many samples for one launch");
        DspLaunch p{false, false, true, false, &scan, &loud_scan()};
        p.gain_only = true;
        launch_dsp(m.dsp_ring.stage(rows.data() + at, k, s), k, (int)tiles, p, s);
        m.dsp_ring.done(s);
    }
}

void join_gain_launch(Model& m, const std::vector<JoinGainRow>& rows, hipStream_t s) {
    constexpr int kRows = RowRing<JoinGainRow>::kRows;
    std::vector<JoinRow> plain;
    for (size_t at = 0; at < rows.size(); at += kRows) {
        const int n = (int)std::min<size_t>(kRows, rows.size() - at);
        int64_t tiles = 0;
        bool any = false;
        for (int i = 0; i < n; i++) {
            const JoinRow& r = rows[at + (size_t)i].r;
            any = any || rows[at + (size_t)i].flags != 0;
            if (r.gap + r.n > 0) tiles = std::max(tiles, (r.gap + r.n + 3 + kJoinTile - 1) / kJoinTile);
        }
        if (tiles == 0) continue;
        if (tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: join: too many samples for one launch");
        if (!any) {   // a table without a gain: k_join, as join_launch launches it
            plain.clear();
            for (int i = 0; i < n; i++) plain.push_back(rows[at + (size_t)i].r);
            launch_join(m.join_ring.stage(plain.data(), n, s), n, (int)tiles, s);
            m.join_ring.done(s);
            continue;
        }
        launch_join_gain(m.join_gain_ring.stage(rows.data() + at, n, s), n, (int)tiles, s);
        m.join_gain_ring.done(s);
    }
}

// the flags and the gains of row r from the part's volume and, for a seam whose tail lies in the predecessor's own buffer, the predecessor's
static void join_row_gains(JoinGainRow& r, const PartGain& mine, const PartGain* prev) {
    if (mine.fixed) { r.flags |= JOIN_GAIN_IMM; r.g = mine.g; }
    else if (mine.word) { r.flags |= JOIN_GAIN_WORD; r.gw = mine.word; }
    if (!prev || r.r.k <= 0) return;
    if (prev->fixed) { r.flags |= JOIN_PREV_IMM; r.g_prev = prev->g; }
    else if (prev->word) { r.flags |= JOIN_PREV_WORD; r.gw_prev = prev->word; }
}

JoinGainRow join_gain_row(const JoinRow& r, const PartGain& mine, const PartGain* prev) {
    JoinGainRow g{};
    g.r = r; g.g = 1.0f; g.g_prev = 1.0f;
    join_row_gains(g, mine, prev);
    return g;
}

// the parts' volumes on device rows: the fixed gains as they are, the levels' words from one level_launch over the rows that have one
std::vector<PartGain> part_gains_launch(Model& m, const std::vector<const float*>& x, const std::vector<int64_t>& n, const std::vector<PartVolume>& vol, hipStream_t s) {
    std::vector<PartGain> g(vol.size());
    std::vector<const float*> lx, words;
    std::vector<int64_t> ln;
    std::vector<double> lt;
    std::vector<size_t> at;
    for (size_t i = 0; i < vol.size(); i++) {
        if (vol[i].fixed) { g[i].fixed = true; g[i].g = vol[i].g; }
        else if (vol[i].level) { lx.push_back(x[i]); ln.push_back(n[i]); lt.push_back(loud_target_power(vol[i].target_lufs)); at.push_back(i); }
    }
    if (!lx.empty()) {
        level_launch(m, lx, ln, lt, words, s);
        for (size_t k = 0; k < at.size(); k++) g[at[k]].word = words[k];
    }
    return g;
}

void join_parts_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const JoinSeams& seams, const std::vector<PartVolume>& vol, float* out,
                            float* gains) {
    std::vector<int64_t> off((size_t)rows), seam((size_t)rows);
    int64_t total = 0;
    const std::string e = join_parts_plan(n, rows, seams, off.data(), seam.data(), &total);
    if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
    for (int i = 0; gains && i < rows; i++) gains[i] = vol[(size_t)i].fixed ? vol[(size_t)i].g : 1.0f;
    if (total == 0) return;
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> bytes((size_t)rows + 1);
    for (int i = 0; i < rows; i++) bytes[(size_t)i] = (size_t)n[i] * sizeof(float);
    bytes[(size_t)rows] = (size_t)total * sizeof(float);   // the joined row, behind the parts
    PackedRows buf(m, WORK_HOST_ROWS, std::move(bytes));
    std::vector<const float*> x((size_t)rows);
    std::vector<int64_t> len(n, n + rows);
    for (int i = 0; i < rows; i++) {
        if (n[i] > 0) buf.upload(i, in[i], s);
        x[(size_t)i] = (const float*)buf.row(i);
    }
    const std::vector<PartGain> pg = part_gains_launch(m, x, len, vol, s);
    std::vector<JoinGainRow> jr;
    for (int i = 0; i < rows; i++) {
        const int64_t k = seam[(size_t)i], k_next = i + 1 < rows ? seam[(size_t)i + 1] : 0;
        JoinRow r{};
        r.src = x[(size_t)i];
        r.prev = k ? x[(size_t)i - 1] + (n[i - 1] - k) : nullptr;
        r.dst = (float*)buf.row(rows);
        r.off = off[(size_t)i];
        r.n = n[i] - k_next;
        r.k = (int32_t)k;
        r.gap = i ? (int32_t)seams.lens[(size_t)i - 1].gap : 0;
        jr.push_back(join_gain_row(r, pg[(size_t)i], i ? &pg[(size_t)i - 1] : nullptr));
    }
    join_gain_launch(m, jr, s);
    buf.download(rows, out, s);
    for (int i = 0; gains && i < rows; i++)
        if (pg[(size_t)i].word) PTTS_HIP(hipMemcpyAsync(gains + i, pg[(size_t)i].word, sizeof(float), hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipStreamSynchronize(s));
}

// ---- the part stages of a joined call: the trim (trim.hip; trim.h), the pitch (pitch.hip; pitch.h), the tempo (tempo.hip; tempo.h) ----

UploadedTable::~UploadedTable() {
    if (ready) { (void)hipEventSynchronize(ready); (void)hipEventDestroy(ready); }
    if (staged) (void)hipHostFree(staged);
}

namespace {
// The trim's tables: rows[i] states src, dst and n, key[i] its design; their scratch (WORK_TRIM_SCRATCH) and their tables are made here, one launch
// sequence per table.  Returns the device copy of the rows' records, [rows.size()], complete behind the launches
const ptts_trim_info* trim_launch(Model& m, std::vector<TrimRow>& rows, const std::vector<const TrimScan*>& key, hipStream_t s) {
    size_t tiles = 0;
    for (const TrimRow& r : rows) tiles += (size_t)scan_tiles(std::max<int64_t>(r.n, 0));
    const size_t info_bytes = (rows.size() * sizeof(ptts_trim_info) + 255) & ~(size_t)255;
    char* scratch = m.work(WORK_TRIM_SCRATCH, info_bytes + std::max<size_t>(tiles, 1) * sizeof(TrimTile)).as<char>();
    ptts_trim_info* info = reinterpret_cast<ptts_trim_info*>(scratch);
    TrimTile* t = reinterpret_cast<TrimTile*>(scratch + info_bytes);
    for (size_t i = 0; i < rows.size(); i++) {
        if (rows[i].n >= kTrimMaxSamples) throw Error(PTTS_EINVAL, strfmt("ptts-hip: trim: row %zu has %lld samples, a row must stay below 2^31", i, (long long)rows[i].n));
        rows[i].info = info + i;
        rows[i].tiles = t;
        t += scan_tiles(std::max<int64_t>(rows[i].n, 0));
    }
    launch_tables(m.trim_ring, rows, key, kTrimMaxDesigns, same_bytes<TrimScan>, &TrimRow::design, "trim", s,
                  [&](size_t, int k, const TrimRow* rows_dev, int max_tiles, const TrimScan* designs_dev) { launch_trim(rows_dev, k, max_tiles, designs_dev, s); });
    return info;
}

// The tempo's tables: rows[i] states src, dst and n, key[i] its design; n_out (host arithmetic), the position tables (WORK_TEMPO_SCRATCH) and the row
// tables are made here, one launch of each kernel per table
void tempo_launch(Model& m, std::vector<TempoRow>& rows, const std::vector<const TempoScan*>& key, hipStream_t s) {
    size_t hops = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        if (rows[i].n >= kTempoMaxSamples) throw Error(PTTS_EINVAL, strfmt("ptts-hip: tempo: row %zu has %lld samples, a row must stay below 2^31 - %d", i, (long long)rows[i].n, kTempoRadius));
        rows[i].n_out = tempo_length(rows[i].n, key[i]->speed);
        hops += (size_t)tempo_hops(rows[i].n_out);
    }
    int32_t* p = m.work(WORK_TEMPO_SCRATCH, std::max<size_t>(hops, 1) * sizeof(int32_t)).as<int32_t>();
    for (TempoRow& r : rows) {
        r.p = p;
        p += tempo_hops(r.n_out);
    }
    launch_tables(m.tempo_ring, rows, key, kTempoMaxDesigns, same_bytes<TempoScan>, &TempoRow::design, "tempo", s,
                  [&](size_t first, int k, const TempoRow* rows_dev, int, const TempoScan* designs_dev) {
        int64_t tiles = 0;   // of the OUTPUT: a slowed row is longer than its input
        for (int i = 0; i < k; i++) tiles = std::max(tiles, scan_tiles(rows[first + (size_t)i].n_out));
        if (tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: tempo: too many samples for one launch");
        launch_tempo(rows_dev, k, (int)tiles, designs_dev, s);
    });
}

// A table that one model uploads once, on first use (runtime.h UploadedTable): `bytes` filled by fill(staged) in page-locked memory and queued on s, nothing
// waits on the host; launches on s follow it, another stream waits for `ready` (as rate_filter, resample.cpp)
template <class Fill>
const void* upload_once(std::unique_ptr<UploadedTable>& slot, size_t bytes, hipStream_t s, Fill&& fill) {
    if (slot) {
        if (slot->up != s) PTTS_HIP(hipStreamWaitEvent(s, slot->ready, 0));
        return slot->image.p;
    }
    std::unique_ptr<UploadedTable> f(new UploadedTable());
    PTTS_HIP(hipHostMalloc(&f->staged, bytes, hipHostMallocDefault));
    std::memset(f->staged, 0, bytes);
    fill(f->staged);
    f->image.ensure(bytes);
    PTTS_HIP(hipMemcpyAsync(f->image.p, f->staged, bytes, hipMemcpyHostToDevice, s));
    PTTS_HIP(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
    PTTS_HIP(hipEventRecord(f->ready, s));
    f->up = s;
    slot = std::move(f);
    return slot->image.p;
}

// the pitch table's image on the device: one per model whatever the pitches, made from pitch.cpp's table
const float* pitch_image(Model& m, hipStream_t s) {
    return static_cast<const float*>(upload_once(m.pitch_image, (size_t)kPitchImage * 2 * sizeof(float), s, [](void* to) {
        float* const staged = static_cast<float*>(to);
        const float* const h = pitch_table_h();
        const float* const hd = pitch_table_hd();
        for (int q = 0; q < kPitchEntries; q++) {
            staged[2 * (size_t)pitch_image_at(q)] = h[q];
            staged[2 * (size_t)pitch_image_at(q) + 1] = hd[q];
        }
    }));
}

// formant.cpp's float64 tables on the device, as they are: one copy per model
const double* formant_tables_device(Model& m, hipStream_t s) {
    return static_cast<const double*>(upload_once(m.formant_tables, (size_t)kFormantTableDoubles * sizeof(double), s, [](void* staged) {
        std::memcpy(staged, formant_tables(), (size_t)kFormantTableDoubles * sizeof(double));
    }));
}

// The tables of the pitch's resampling step: rows[i] states src, dst and n, key[i] its design (p is not 1000); n_out (host arithmetic), the table's
// image (first use: made and uploaded) and the row tables are made here, one launch per table
void pitch_launch(Model& m, std::vector<PitchRow>& rows, const std::vector<const PitchScan*>& key, hipStream_t s) {
    for (size_t i = 0; i < rows.size(); i++) {
        rows[i].n_out = pitch_resample_length(rows[i].n, key[i]->p);
        if (rows[i].n < 0 || rows[i].n_out >= kTempoMaxSamples)
            throw Error(PTTS_EINVAL, strfmt("ptts-hip: pitch: row %zu has %lld samples and %lld resampled, a row must stay below 2^31 - %d", i, (long long)rows[i].n,
                                            (long long)rows[i].n_out, kTempoRadius));
    }
    const float* const image = pitch_image(m, s);
    launch_tables(m.pitch_ring, rows, key, kPitchMaxDesigns, same_bytes<PitchScan>, &PitchRow::design, "pitch", s,
                  [&](size_t first, int k, const PitchRow* rows_dev, int, const PitchScan* designs_dev) {
        int64_t tiles = 0;   // of the OUTPUT
        for (int i = 0; i < k; i++) tiles = std::max(tiles, (rows[first + (size_t)i].n_out + kPitchTile - 1) / kPitchTile);
        launch_pitch(rows_dev, k, (int)tiles, designs_dev, image, s);
    });
}

// The formant kernels' tables: 256 rows a turn, launch(rows_dev, count, first) between the turn's stage() and done()
template <class Launch>
void formant_tables_launch(Model& m, const std::vector<FormantRow>& fr, hipStream_t s, Launch&& launch) {
    constexpr size_t kRows = RowRing<FormantRow>::kRows;
    for (size_t at = 0; at < fr.size(); at += kRows) {
        const int n = (int)std::min(kRows, fr.size() - at);
        launch(m.formant_ring.stage(fr.data() + at, n, s), n, at);
        m.formant_ring.done(s);
    }
}

// The pitch step of parts_launch: t and key are its rows with a pitch as part_stage made them (src: where the row stands; dst: PartRow::shifted), in the
// order of `rows`.  Rows that keep their formants (PartStages::formant) get their frames' coefficients and their residual first (k_formant_analyse,
// k_formant_whiten, one launch of each per table of such rows); k_pitch_resample then reads the residual and writes the resampled residual, in the one
// launch per table that serves every row with a pitch; k_formant_shape puts the envelopes back, into PartRow::shifted.  The three work buffers are
// made only when a row has the option: without one this is pitch_launch, and nothing else
void pitch_stage_launch(Model& m, const std::vector<PartRow>& rows, std::vector<PitchRow>& t, const std::vector<const PitchScan*>& key, hipStream_t s) {
    std::vector<FormantRow> fr;
    std::vector<size_t> at;   // where in t
    size_t k = 0, frames = 0, samples = 0, shifted = 0;
    for (const PartRow& r : rows) {
        if (!r.st.pitch) continue;
        const size_t mine = k++;
        if (!r.st.formant || t[mine].n <= 0) continue;
        FormantRow f{};
        f.n = t[mine].n;
        f.n_r = pitch_resample_length(f.n, key[mine]->p);
        f.K = (int32_t)formant_frames(f.n);
        f.p = key[mine]->p;
        if (f.n >= kTempoMaxSamples || f.n_r >= kTempoMaxSamples || f.p < kFormantMinPitch || f.p > kFormantMaxPitch)
            throw Error(PTTS_EINVAL, "ptts-hip: internal: a row that keeps its formants is outside what the option serves");
        frames += (size_t)f.K; samples += (size_t)f.n; shifted += (size_t)f.n_r;
        fr.push_back(f);
        at.push_back(mine);
    }
    if (fr.empty()) { pitch_launch(m, t, key, s); return; }
    float* coeffs = m.work(WORK_FORMANT_COEFFS, frames * kFormantOrder * sizeof(float)).as<float>();
    float* e = m.work(WORK_FORMANT_RESIDUAL, samples * sizeof(float)).as<float>();
    float* er = m.work(WORK_FORMANT_SHIFTED, shifted * sizeof(float)).as<float>();
    for (size_t i = 0; i < fr.size(); i++) {
        FormantRow& f = fr[i];
        PitchRow& p = t[at[i]];
        f.x = p.src; f.e = e; f.er = er; f.out = p.dst; f.coeffs = coeffs;
        p.src = e; p.dst = er;   // the resample runs on the residual
        coeffs += (size_t)f.K * kFormantOrder; e += f.n; er += f.n_r;
    }
    const double* const tables = formant_tables_device(m, s);
    formant_tables_launch(m, fr, s, [&](const FormantRow* dev, int n, size_t first) {
        int64_t K = 0, tiles = 0;
        for (int i = 0; i < n; i++) {
            K = std::max<int64_t>(K, fr[first + (size_t)i].K);
            tiles = std::max(tiles, (fr[first + (size_t)i].n + kFormantHop / 2 + kFormantHop - 1) / kFormantHop);
        }
        launch_formant_analyse(dev, n, K, tables, s);
        launch_formant_whiten(dev, n, tiles, s);
    });
    pitch_launch(m, t, key, s);
    formant_tables_launch(m, fr, s, [&](const FormantRow* dev, int n, size_t first) {
        int64_t tiles = 0;
        for (int i = 0; i < n; i++) tiles = std::max(tiles, (fr[first + (size_t)i].n_r + kFormantHop - 1) / kFormantHop);
        launch_formant_shape(dev, n, tiles, s);
    });
    for (size_t i = 0; i < fr.size(); i++) t[at[i]].dst = fr[i].out;   // where the row stands behind the step
}

// one stage of parts_launch behind the trim: the rows that have it, each reading where its predecessor left the row (PartRow::out, n_out) and
// writing its own destination, through the stage's table builder; then every such row stands at what the stage made.  False: no row has the stage
template <class Row, class Design, class Launch>
bool part_stage(std::vector<PartRow>& rows, const Design* PartStages::*which, float* PartRow::*dst, Launch&& launch) {
    std::vector<Row> t;
    std::vector<const Design*> key;
    std::vector<size_t> at;
    for (size_t i = 0; i < rows.size(); i++) {
        if (!(rows[i].st.*which)) continue;
        Row r{};
        r.src = rows[i].out; r.dst = rows[i].*dst; r.n = rows[i].n_out;
        t.push_back(r);
        key.push_back(rows[i].st.*which);
        at.push_back(i);
    }
    if (t.empty()) return false;
    launch(t, key);
    for (size_t k = 0; k < t.size(); k++) {
        rows[at[k]].out = t[k].dst;
        rows[at[k]].n_out = t[k].n_out;
    }
    return true;
}
}  // namespace

void parts_launch(Model& m, std::vector<PartRow>& rows, hipStream_t s, const std::function<void(const char*)>& phase, const char* unit) {
    std::vector<TrimRow> tr;
    std::vector<const TrimScan*> key;
    std::vector<size_t> at;
    for (size_t i = 0; i < rows.size(); i++) {
        PartRow& r = rows[i];
        r.out = r.src; r.n_out = r.n;
        if (!r.st.trim) continue;
        TrimRow t{};
        t.src = r.src; t.dst = r.trimmed; t.n = r.n;
        tr.push_back(t);
        key.push_back(r.st.trim);
        at.push_back(i);
    }
    if (!tr.empty()) {
        const ptts_trim_info* info_dev = trim_launch(m, tr, key, s);
        ptts_trim_info* const got = static_cast<ptts_trim_info*>(m.trim_info.ensure(tr.size() * sizeof(ptts_trim_info)));
        PTTS_HIP(hipMemcpyAsync(got, info_dev, tr.size() * sizeof(ptts_trim_info), hipMemcpyDeviceToHost, s));
        PTTS_HIP(hipStreamSynchronize(s));   // the lengths decide what the later stages read and what comes back
        for (size_t k = 0; k < tr.size(); k++) {
            PartRow& r = rows[at[k]];
            if (got[k].n_out < 0 || got[k].n_out > r.n) throw Error(PTTS_EINVAL, strfmt("ptts-hip: internal: a trimmed %s is longer than the %s", unit, unit));
            r.info = got[k];
            r.out = r.trimmed; r.n_out = got[k].n_out;
        }
        if (phase) phase("trim");
    }
    if (part_stage<PitchRow>(rows, &PartStages::pitch, &PartRow::shifted, [&](std::vector<PitchRow>& t, const std::vector<const PitchScan*>& k) { pitch_stage_launch(m, rows, t, k, s); }) && phase)
        phase("pitch");
    if (part_stage<TempoRow>(rows, &PartStages::tempo, &PartRow::scaled, [&](std::vector<TempoRow>& t, const std::vector<const TempoScan*>& k) { tempo_launch(m, t, k, s); }) && phase)
        phase("tempo");
}

void part_rows_device(Model& m, const PartStages* per_row, const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out,
                      ptts_trim_info* info) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    // the rows, then their trimmed, their resampled and their time-scaled forms; a row takes bytes only for the steps it has, and none where it
    // stays on the host
    const size_t R = (size_t)rows;
    std::vector<size_t> bytes(R * 4, 0);
    std::unique_ptr<bool[]> skip(new bool[R * 4 + 1]);
    for (size_t i = 0; i < R; i++) {
        const PartStages& st = per_row[i];
        // the longest each form can be: the trim only shortens, and the two length functions are monotone
        const int64_t n_t = std::max<int64_t>(n[i], 0);
        const int64_t n_r = st.pitch ? pitch_resample_length(n_t, st.pitch->p) : n_t;
        const int64_t n_f = st.tempo ? tempo_length(n_r, st.tempo->speed) : n_r;
        if (n_out) n_out[i] = n_f;
        if (info) info[i] = ptts_trim_info{0, n[i], n[i], 0, 0, 0};
        const bool on = (st.trim || st.pitch || st.tempo) && n_f > 0;
        skip[i] = !on;
        skip[R + i] = !(on && st.trim);
        skip[2 * R + i] = !(on && st.pitch);
        skip[3 * R + i] = !(on && st.tempo);
        if (!skip[i]) bytes[i] = (size_t)n[i] * sizeof(float);
        if (!skip[R + i]) bytes[R + i] = (size_t)n_t * sizeof(float);
        if (!skip[2 * R + i]) bytes[2 * R + i] = (size_t)n_r * sizeof(float);
        if (!skip[3 * R + i]) bytes[3 * R + i] = (size_t)n_f * sizeof(float);
    }
    PackedRows buf(m, WORK_HOST_ROWS, std::move(bytes), skip.get());
    std::vector<PartRow> pr;
    std::vector<int> row_of;
    for (int i = 0; i < rows; i++) {
        const PartStages& st = per_row[i];
        if (skip[(size_t)i]) {   // nothing to do on the device: a copy, or an empty result
            if (!st.trim && !st.pitch && !st.tempo && n[i] > 0 && out[i] != in[i]) std::memmove(out[i], in[i], (size_t)n[i] * sizeof(float));
            continue;
        }
        buf.upload(i, in[i], s);
        PartRow r{(const float*)buf.row(i), n[i], st};
        if (st.trim) r.trimmed = (float*)buf.row(rows + i);
        if (st.pitch) r.shifted = (float*)buf.row(2 * rows + i);
        if (st.tempo) r.scaled = (float*)buf.row(3 * rows + i);
        pr.push_back(r);
        row_of.push_back(i);
    }
    if (pr.empty()) return;
    parts_launch(m, pr, s);
    for (size_t k = 0; k < pr.size(); k++) {
        const int i = row_of[k];
        if (n_out) n_out[i] = pr[k].n_out;
        if (info && pr[k].st.trim) info[i] = pr[k].info;
        if (pr[k].n_out > 0) PTTS_HIP(hipMemcpyAsync(out[i], pr[k].out, (size_t)pr[k].n_out * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    PTTS_HIP(hipStreamSynchronize(s));
}

}  // namespace ptts
