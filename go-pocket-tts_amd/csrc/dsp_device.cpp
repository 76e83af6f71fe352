// dsp_device.cpp -- the host side of the device post-processing (dsp.hip): checks of a ptts_dsp_opts, the row
// tables and scratch of the DSP kernels, their launches.  The coefficients come from dsp.cpp (dsp_scan_coeffs), made as dsp_dc_block makes them.
#include <cmath>

#include "scan_block.h"
#include "eq.h"
#include "true_peak.h"
#include "runtime.h"

namespace ptts {

static_assert(sizeof(EqScan) == kDspEqBytes, "kernels.h sizes the DSP ring's tail by it");

std::string dsp_opts_error(const ptts_dsp_opts& o) {
    if (std::isnan(o.fade_in_ms) || o.fade_in_ms < 0) return strfmt("dsp: fade_in_ms %g is negative or not a number", o.fade_in_ms);
    if (std::isnan(o.fade_out_ms) || o.fade_out_ms < 0) return strfmt("dsp: fade_out_ms %g is negative or not a number", o.fade_out_ms);
    if (o.eq && !eq_lookup(o.eq)) return strfmt("dsp: eq %p is not a live handle of ptts_eq_create", (const void*)o.eq);
    DspExt ext;   // (no reserved word is left to check: whatever lies in reserved[2..3] is a handle the registry knows, or refused unread)
    if (o.ext && !ext_lookup(o.ext, &ext)) return strfmt("dsp: ext %p (reserved[2..3]) is not a live handle of ptts_dsp_ext_create", (const void*)o.ext);
    return std::string();
}

bool dsp_ext_active(const ptts_dsp_ext* e) {
    DspExt ext;
    return ext_lookup(e, &ext) && ext.true_peak;
}

namespace {
int64_t fade_samples(double ms, int64_t n) {   // dsp_fade_in / dsp_fade_out: min((int64)(ms / 1000 * 24000), n)
    if (!(ms > 0)) return 0;
    const double f = ms / 1000.0 * (double)kNativeRate;
    return f >= (double)n ? n : (int64_t)f;
}
}  // namespace

void dsp_launch(Model& m, std::vector<DspJob>& jobs, hipStream_t s, bool apply) {
    static const DspScan scan = dsp_scan_coeffs(kNativeRate);
    if (jobs.empty()) return;
    constexpr int kRows = RowRing<DspRow>::kRows;
    // a row's equaliser: the job's own, or its options' (a handle freed since the request was checked: PTTS_EINVAL, nothing is launched)
    std::vector<const EqScan*> job_eq(jobs.size(), nullptr);
    for (size_t k = 0; k < jobs.size(); k++) {
        const DspJob& j = jobs[k];
        job_eq[k] = j.eq;
        if (!j.eq && j.opts && j.opts->eq && !(job_eq[k] = eq_lookup(j.opts->eq))) throw Error(PTTS_EINVAL, "ptts-hip: " + dsp_opts_error(*j.opts));
    }
    // a row's ceiling: the job's own, or its options' (the same rule for a handle freed since; the ceiling is copied by value)
    std::vector<DspExt> job_tp(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) {
        const DspJob& j = jobs[k];
        job_tp[k] = DspExt{j.tp, j.ceiling};
        if (!j.tp && j.opts && j.opts->ext && !ext_lookup(j.opts->ext, &job_tp[k])) throw Error(PTTS_EINVAL, "ptts-hip: " + dsp_opts_error(*j.opts));
    }
    // scratch: a peak word and a true-peak word per row, then the per-tile states of each DC row and each equaliser row and the block of each loudness row (scan_block.h)
    size_t tile_doubles = 0;
    for (size_t k = 0; k < jobs.size(); k++) {
        const DspJob& j = jobs[k];
        if (j.n <= 0) continue;
        if (j.opts && j.opts->dc_block) tile_doubles += scan_state_doubles<DspScan::N>(scan_tiles(j.n));
        if (j.loud) tile_doubles += loud_doubles(scan_tiles(j.n));
        if (job_eq[k]) tile_doubles += (size_t)scan_tiles(j.n) * 4 * (size_t)job_eq[k]->S;
    }
    const size_t peak_bytes = (2 * jobs.size() * sizeof(uint32_t) + 255) & ~(size_t)255;   // [jobs] sample peaks, then [jobs] true peaks
    char* scratch = m.work(29, peak_bytes + std::max<size_t>(tile_doubles, 1) * sizeof(double)).as<char>();
    uint32_t* peaks = reinterpret_cast<uint32_t*>(scratch);
    double* tiles = reinterpret_cast<double*>(scratch + peak_bytes);
    PTTS_HIP(hipMemsetAsync(peaks, 0, peak_bytes, s));
    std::vector<DspRow> rows;
    std::vector<const EqScan*> row_eq;
    rows.reserve(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) {
        DspJob& j = jobs[k];
        j.loud_out = nullptr;
        j.tp_out = nullptr;
        const bool on = dsp_active(j.opts);
        if (j.n <= 0 || !(on || j.loud || job_eq[k] || job_tp[k].true_peak)) continue;
        DspRow r{};
        r.x = j.x; r.n = j.n;
        r.fade_in = on ? fade_samples(j.opts->fade_in_ms, j.n) : 0;
        r.fade_out = on ? fade_samples(j.opts->fade_out_ms, j.n) : 0;
        r.peak = peaks + k;
        r.flags = (on && j.opts->normalize ? DSP_NORMALIZE : 0) | (on && j.opts->dc_block ? DSP_DC : 0) | (j.loud ? DSP_LOUD : 0);
        if (r.flags & DSP_DC) { r.tiles = tiles; tiles += scan_state_doubles<DspScan::N>(scan_tiles(j.n)); }
        if (j.loud) {
            r.loud = j.loud_out = tiles;
            r.target = j.target_power;
            tiles += loud_doubles(scan_tiles(j.n));
        }
        if (job_eq[k] && apply) {
            r.flags |= DSP_EQ;
            r.eq_tiles = tiles;
            tiles += (size_t)scan_tiles(j.n) * 4 * (size_t)job_eq[k]->S;
        }
        if (job_tp[k].true_peak) {
            r.flags |= DSP_TP;
            r.tp = j.tp_out = peaks + jobs.size() + k;
            r.ceiling = job_tp[k].ceiling;
        }
        rows.push_back(r);
        row_eq.push_back(job_eq[k]);
    }
    // a table: up to kRows rows with up to kDspMaxEq distinct equalisers, which travel behind the rows in the same turn of the ring
    std::vector<EqScan> eqs;
    std::vector<const EqScan*> eq_of;
    for (size_t at = 0; at < rows.size();) {
        int n = 0;
        int64_t max_tiles = 0;
        DspLaunch p{false, false, false, apply, &scan, &loud_scan()};
        eqs.clear();
        eq_of.clear();
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
        p.taps = &tp_taps();
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: dsp: too many samples for one launch");
        const void* eqs_dev = nullptr;
        const DspRow* rows_dev = m.dsp_ring.stage(rows.data() + at, n, s, eqs.data(), eqs.size() * sizeof(EqScan), &eqs_dev);
        p.eqs = static_cast<const EqScan*>(eqs_dev);
        launch_dsp(rows_dev, n, (int)max_tiles, p, s);
        m.dsp_ring.done(s);
        at += (size_t)n;
    }
}

// ptts_true_peak_rows: rows packed 256-byte aligned in one device buffer, the measuring launch of a request's ceiling
void true_peak_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, float* peaks) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> off((size_t)rows);
    size_t bytes = 0;
    for (int i = 0; i < rows; i++) { off[(size_t)i] = bytes; bytes += ((size_t)n[i] * sizeof(float) + 255) & ~(size_t)255; }
    char* buf = m.work(30, std::max<size_t>(bytes, 256)).as<char>();
    std::vector<DspJob> jobs;
    std::vector<int> job_row;
    for (int i = 0; i < rows; i++) {
        peaks[i] = 0.0f;
        if (n[i] <= 0) continue;
        PTTS_HIP(hipMemcpyAsync(buf + off[(size_t)i], in[i], (size_t)n[i] * sizeof(float), hipMemcpyHostToDevice, s));
        DspJob j{(float*)(buf + off[(size_t)i]), n[i], nullptr};
        j.tp = true;
        jobs.push_back(j);
        job_row.push_back(i);
    }
    dsp_launch(m, jobs, s, false);
    for (size_t k = 0; k < jobs.size(); k++) PTTS_HIP(hipMemcpyAsync(peaks + job_row[k], jobs[k].tp_out, sizeof(float), hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipStreamSynchronize(s));
}

// ptts_loudness_rows / ptts_loudness_normalize_rows: rows packed 256-byte aligned in one device buffer, the launches of a request's `loudness`
void loudness_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, double target_lufs, float* const* out, double* M,
                          std::vector<double>* sub) {
    std::lock_guard<std::mutex> lock(m.mu);
    m.use_device();
    hipStream_t s = m.stream;
    std::vector<size_t> off((size_t)rows);
    size_t bytes = 0;
    for (int i = 0; i < rows; i++) { off[(size_t)i] = bytes; bytes += ((size_t)n[i] * sizeof(float) + 255) & ~(size_t)255; }
    char* buf = m.work(30, std::max<size_t>(bytes, 256)).as<char>();
    const double T = out ? loud_target_power(target_lufs) : 1.0;
    std::vector<DspJob> jobs;
    std::vector<int> job_row;
    for (int i = 0; i < rows; i++) {
        if (M) M[i] = 0.0;
        if (sub) sub[i].clear();
        if (n[i] <= 0) continue;
        PTTS_HIP(hipMemcpyAsync(buf + off[(size_t)i], in[i], (size_t)n[i] * sizeof(float), hipMemcpyHostToDevice, s));
        DspJob j{(float*)(buf + off[(size_t)i]), n[i], nullptr};
        j.loud = true; j.target_power = T;
        jobs.push_back(j);
        job_row.push_back(i);
    }
    dsp_launch(m, jobs, s, out != nullptr);
    for (size_t k = 0; k < jobs.size(); k++) {
        const int i = job_row[k];
        const int64_t F = scan_tiles(n[i]);
        if (M) PTTS_HIP(hipMemcpyAsync(M + i, jobs[k].loud_out, sizeof(double), hipMemcpyDeviceToHost, s));
        if (sub) {
            sub[i].resize((size_t)F * kLoudSubsPerTile);
            PTTS_HIP(hipMemcpyAsync(sub[i].data(), loud_subs(jobs[k].loud_out, F), sub[i].size() * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        if (out) PTTS_HIP(hipMemcpyAsync(out[i], buf + off[(size_t)i], (size_t)n[i] * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    PTTS_HIP(hipStreamSynchronize(s));
}

}  // namespace ptts
