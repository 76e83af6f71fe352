// dsp_device.cpp -- the host side of the device post-processing (dsp.hip): the row tables and scratch of the DSP kernels,
// their launches, and the round trip of host rows through them.  The coefficients come from dsp.cpp (dsp_scan_coeffs), made as dsp_dc_block makes
// them; what a row gets is resolved in dsp_spec.cpp.
#include <cmath>

#include "scan_block.h"
#include "runtime.h"

namespace ptts {

static_assert(sizeof(EqScan) == kDspEqBytes, "kernels.h sizes the DSP ring's tail by it");
static_assert(sizeof(CmpScan) == kCmpScanBytes, "kernels.h sizes the compressor ring's tail by it");
static_assert(sizeof(LimScan) == kLimScanBytes, "kernels.h sizes the limiter ring's tail by it");

namespace {
int64_t fade_samples(double ms, int64_t n) {   // dsp_fade_in / dsp_fade_out: min((int64)(ms / 1000 * 24000), n)
    if (!(ms > 0)) return 0;
    const double f = ms / 1000.0 * (double)kNativeRate;
    return f >= (double)n ? n : (int64_t)f;
}

// The compressor's tables (compressor.hip), in front of everything that measures or rewrites a row: the jobs whose spec has one, up to kRows
// rows with up to kCmpMaxDesigns distinct designs a table, which travel behind the rows in the same turn of the ring.  tiles: the rows' per-tile
// states are taken from it, cmp_state_doubles each
void cmp_launch(Model& m, const std::vector<DspJob>& jobs, double*& tiles, hipStream_t s) {
    constexpr int kRows = RowRing<CmpRow>::kRows;
    std::vector<CmpRow> rows;
    std::vector<const CmpScan*> row_design;
    for (const DspJob& j : jobs) {
        if (j.n <= 0 || !j.spec.compress) continue;
        const int64_t F = scan_tiles(j.n);
        CmpRow r{};
        r.x = j.x; r.n = j.n;
        r.p_tiles = tiles;
        r.s_tiles = tiles + scan_state_doubles<1>(F);
        tiles += cmp_state_doubles(F);
        rows.push_back(r);
        row_design.push_back(&j.spec.cmp);
    }
    std::vector<CmpScan> designs;
    for (size_t at = 0; at < rows.size();) {
        int n = 0;
        int64_t max_tiles = 0;
        designs.clear();
        for (; n < kRows && at + (size_t)n < rows.size(); n++) {
            CmpRow& r = rows[at + (size_t)n];
            const CmpScan& d = *row_design[at + (size_t)n];
            size_t k = 0;
            while (k < designs.size() && std::memcmp(&designs[k], &d, sizeof d) != 0) k++;
            if (k == designs.size()) {
                if (designs.size() == (size_t)kCmpMaxDesigns) break;   // the next table's
                designs.push_back(d);
            }
            r.design = (int32_t)k;
            max_tiles = std::max(max_tiles, scan_tiles(r.n));
        }
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: compressor: too many samples for one launch");
        const void* designs_dev = nullptr;
        const CmpRow* rows_dev = m.cmp_ring.stage(rows.data() + at, n, s, designs.data(), designs.size() * sizeof(CmpScan), &designs_dev);
        launch_compressor(rows_dev, n, (int)max_tiles, static_cast<const CmpScan*>(designs_dev), s);
        m.cmp_ring.done(s);
        at += (size_t)n;
    }
}

// The limiter's tables (limiter.hip) for the limiter rows of one DSP table, behind that table's last kernel and in front of its true-peak pair:
// up to kLimMaxDesigns distinct designs a table, which travel behind the rows in the same turn of the ring
void lim_launch(Model& m, std::vector<LimRow>& rows, const std::vector<const LimScan*>& row_design, hipStream_t s) {
    constexpr int kRows = RowRing<LimRow>::kRows;
    std::vector<LimScan> designs;
    for (size_t at = 0; at < rows.size();) {
        int n = 0;
        int64_t max_tiles = 0;
        designs.clear();
        for (; n < kRows && at + (size_t)n < rows.size(); n++) {
            LimRow& r = rows[at + (size_t)n];
            const LimScan& d = *row_design[at + (size_t)n];
            size_t k = 0;
            while (k < designs.size() && std::memcmp(&designs[k], &d, sizeof d) != 0) k++;
            if (k == designs.size()) {
                if (designs.size() == (size_t)kLimMaxDesigns) break;   // the next table's
                designs.push_back(d);
            }
            r.design = (int32_t)k;
            max_tiles = std::max(max_tiles, scan_tiles(r.n));
        }
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: limiter: too many samples for one launch");
        const void* designs_dev = nullptr;
        const LimRow* rows_dev = m.lim_ring.stage(rows.data() + at, n, s, designs.data(), designs.size() * sizeof(LimScan), &designs_dev);
        launch_limiter(rows_dev, n, (int)max_tiles, static_cast<const LimScan*>(designs_dev), s);
        m.lim_ring.done(s);
        at += (size_t)n;
    }
}
}  // namespace

void dsp_launch(Model& m, std::vector<DspJob>& jobs, hipStream_t s, bool apply) {
    static const DspScan scan = dsp_scan_coeffs(kNativeRate);
    if (jobs.empty()) return;
    constexpr int kRows = RowRing<DspRow>::kRows;
    // scratch: a peak word and a true-peak word per row, then the per-tile states of each compressor row, each DC row and each equaliser row, the block of each loudness row (scan_block.h) and each limiter row's states and gains (limiter.h)
    size_t tile_doubles = 0;
    for (size_t k = 0; k < jobs.size(); k++) {
        const DspJob& j = jobs[k];
        if (j.n <= 0) continue;
        if (j.spec.dc_block) tile_doubles += scan_state_doubles<DspScan::N>(scan_tiles(j.n));
        if (j.spec.loud) tile_doubles += loud_doubles(scan_tiles(j.n));
        if (j.spec.eq) tile_doubles += (size_t)scan_tiles(j.n) * 4 * (size_t)j.spec.eq->S;
        if (j.spec.compress && apply) tile_doubles += cmp_state_doubles(scan_tiles(j.n));
        if (j.spec.limit && apply) tile_doubles += lim_scratch_doubles(j.n);
    }
    const size_t peak_bytes = (2 * jobs.size() * sizeof(uint32_t) + 255) & ~(size_t)255;   // [jobs] sample peaks, then [jobs] true peaks
    char* scratch = m.work(WORK_DSP_SCRATCH, peak_bytes + std::max<size_t>(tile_doubles, 1) * sizeof(double)).as<char>();
    uint32_t* peaks = reinterpret_cast<uint32_t*>(scratch);
    double* tiles = reinterpret_cast<double*>(scratch + peak_bytes);
    PTTS_HIP(hipMemsetAsync(peaks, 0, peak_bytes, s));
    if (apply) cmp_launch(m, jobs, tiles, s);   // the first stage: what follows measures and rewrites the compressed samples (a measurement alone has no compressor: nothing may be rewritten)
    std::vector<DspRow> rows;
    std::vector<const EqScan*> row_eq;
    std::vector<const DspSpec*> row_spec;
    rows.reserve(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) {
        DspJob& j = jobs[k];
        const DspSpec& sp = j.spec;
        j.loud_out = nullptr;
        j.tp_out = nullptr;
        if (j.n <= 0 || !sp.rest()) continue;   // (a compressor alone: no row of the DSP table)
        DspRow r{};
        r.x = j.x; r.n = j.n;
        r.fade_in = fade_samples(sp.fade_in_ms, j.n);
        r.fade_out = fade_samples(sp.fade_out_ms, j.n);
        r.peak = peaks + k;
        r.flags = (sp.normalize ? DSP_NORMALIZE : 0) | (sp.dc_block ? DSP_DC : 0) | (sp.loud ? DSP_LOUD : 0);
        if (r.flags & DSP_DC) { r.tiles = tiles; tiles += scan_state_doubles<DspScan::N>(scan_tiles(j.n)); }
        if (sp.loud) {
            r.loud = j.loud_out = tiles;
            r.target = sp.target_power;
            tiles += loud_doubles(scan_tiles(j.n));
        }
        if (sp.eq && apply) {
            r.flags |= DSP_EQ;
            r.eq_tiles = tiles;
            tiles += (size_t)scan_tiles(j.n) * 4 * (size_t)sp.eq->S;
        }
        if (sp.true_peak) {
            r.flags |= DSP_TP;
            r.tp = j.tp_out = peaks + jobs.size() + k;
            r.ceiling = sp.ceiling;
        }
        rows.push_back(r);
        row_eq.push_back(sp.eq);
        row_spec.push_back(&sp);
    }
    // a table: up to kRows rows with up to kDspMaxEq distinct equalisers, which travel behind the rows in the same turn of the ring
    std::vector<EqScan> eqs;
    std::vector<const EqScan*> eq_of;
    std::vector<LimRow> lim_rows;
    std::vector<const LimScan*> lim_design_of;
    for (size_t at = 0; at < rows.size();) {
        int n = 0;
        int64_t max_tiles = 0;
        DspLaunch p{false, false, false, apply, &scan, &loud_scan()};
        eqs.clear();
        eq_of.clear();
        lim_rows.clear();
        lim_design_of.clear();
        for (; n < kRows && at + (size_t)n < rows.size(); n++) {
            DspRow& r = rows[at + (size_t)n];
            if (r.flags & DSP_EQ) {
                const EqScan* e = row_eq[at + (size_t)n];
                size_t at_eq = 0;
                while (at_eq < eq_of.size() && eq_of[at_eq] != e) at_eq++;
                if (at_eq == eq_of.size()) {
                    if (eq_of.size() == (size_t)kDspMaxEq) break;   // the next table's
                    eq_of.push_back(e);
                    eqs.push_back(*e);
                }
                r.eq = (int32_t)at_eq;
                p.any_eq = true;
            }
            max_tiles = std::max(max_tiles, scan_tiles(r.n));
            p.any_norm = p.any_norm || (r.flags & DSP_NORMALIZE);
            p.any_dc = p.any_dc || (r.flags & DSP_DC);
            p.any_loud = p.any_loud || (r.flags & DSP_LOUD);
            p.any_tp = p.any_tp || (r.flags & DSP_TP);
        }
        if (apply) for (int k = 0; k < n; k++) {   // (a measurement alone has no limiter: nothing may be rewritten)
            const DspSpec& sp = *row_spec[at + (size_t)k];
            if (!sp.limit) continue;
            const DspRow& r = rows[at + (size_t)k];
            LimRow q{};
            q.x = r.x; q.n = r.n;
            q.p_tiles = tiles;
            q.r = reinterpret_cast<float*>(tiles + scan_state_doubles<1>(scan_tiles(r.n)));
            tiles += lim_scratch_doubles(r.n);
            lim_rows.push_back(q);
            lim_design_of.push_back(&sp.lim);
        }
        p.tp_later = !lim_rows.empty();
        p.taps = &tp_taps();
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: dsp: too many samples for one launch");
        const void* eqs_dev = nullptr;
        const DspRow* rows_dev = m.dsp_ring.stage(rows.data() + at, n, s, eqs.data(), eqs.size() * sizeof(EqScan), &eqs_dev);
        p.eqs = static_cast<const EqScan*>(eqs_dev);
        launch_dsp(rows_dev, n, (int)max_tiles, p, s);
        if (p.tp_later) {   // behind the fades, in front of the ceiling
            lim_launch(m, lim_rows, lim_design_of, s);
            if (p.any_tp) {
                launch_tp_peak(rows_dev, n, (int)max_tiles, *p.taps, s);
                launch_tp_scale(rows_dev, n, (int)max_tiles, s);
            }
        }
        m.dsp_ring.done(s);
        at += (size_t)n;
    }
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

}  // namespace ptts
