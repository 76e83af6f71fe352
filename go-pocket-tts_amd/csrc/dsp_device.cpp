// dsp_device.cpp -- the host side of the device post-processing (dsp.hip): checks of a ptts_dsp_opts, the row
// tables and scratch of the DSP kernels, their launches.  The coefficients come from dsp.cpp (dsp_scan_coeffs), made as dsp_dc_block makes them.
#include <cmath>

#include "dsp_block.h"
#include "runtime.h"

namespace ptts {

std::string dsp_opts_error(const ptts_dsp_opts& o) {
    if (std::isnan(o.fade_in_ms) || o.fade_in_ms < 0) return strfmt("dsp: fade_in_ms %g is negative or not a number", o.fade_in_ms);
    if (std::isnan(o.fade_out_ms) || o.fade_out_ms < 0) return strfmt("dsp: fade_out_ms %g is negative or not a number", o.fade_out_ms);
    for (int i = 0; i < 4; i++)
        if (o.reserved[i]) return strfmt("dsp: reserved[%d] is %d, must be 0", i, o.reserved[i]);
    return std::string();
}

DspRing::~DspRing() {
    for (hipEvent_t e : done) if (e) (void)hipEventDestroy(e);
    if (host) (void)hipHostFree(host);
}

namespace {
int64_t fade_samples(double ms, int64_t n) {   // dsp_fade_in / dsp_fade_out: min((int64)(ms / 1000 * 24000), n)
    if (!(ms > 0)) return 0;
    const double f = ms / 1000.0 * (double)kNativeRate;
    return f >= (double)n ? n : (int64_t)f;
}
}  // namespace

void dsp_launch(Model& m, const std::vector<DspJob>& jobs, hipStream_t s) {
    static const DspScan scan = dsp_scan_coeffs(kNativeRate);
    DspRing& R = m.dsp_ring;
    constexpr int kRows = DspRing::kRows;
    if (!R.host) {
        PTTS_HIP(hipHostMalloc((void**)&R.host, sizeof(DspRow) * kRows * DspRing::kRing, hipHostMallocDefault));
        R.dev.ensure(sizeof(DspRow) * kRows * DspRing::kRing);
    }
    // scratch: a peak word per row, then [tiles][4] doubles per DC row
    size_t tile_doubles = 0;
    for (const DspJob& j : jobs)
        if (j.opts->dc_block) tile_doubles += (size_t)((j.n + kDspTile - 1) / kDspTile) * 4;
    const size_t peak_bytes = (jobs.size() * sizeof(uint32_t) + 255) & ~(size_t)255;
    char* scratch = m.work(29, peak_bytes + std::max<size_t>(tile_doubles, 1) * sizeof(double)).as<char>();
    uint32_t* peaks = reinterpret_cast<uint32_t*>(scratch);
    double* tiles = reinterpret_cast<double*>(scratch + peak_bytes);
    PTTS_HIP(hipMemsetAsync(peaks, 0, peak_bytes, s));
    std::vector<DspRow> rows;
    rows.reserve(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) {
        const DspJob& j = jobs[k];
        if (j.n <= 0 || !dsp_active(j.opts)) continue;
        DspRow r{};
        r.x = j.x; r.n = j.n;
        r.fade_in = fade_samples(j.opts->fade_in_ms, j.n);
        r.fade_out = fade_samples(j.opts->fade_out_ms, j.n);
        r.peak = peaks + k;
        r.flags = (j.opts->normalize ? DSP_NORMALIZE : 0) | (j.opts->dc_block ? DSP_DC : 0);
        if (j.opts->dc_block) { r.tiles = tiles; tiles += (size_t)((j.n + kDspTile - 1) / kDspTile) * 4; }
        rows.push_back(r);
    }
    for (size_t at = 0; at < rows.size(); at += kRows) {
        const int n = (int)std::min<size_t>(kRows, rows.size() - at);
        int64_t max_tiles = 0;
        bool any_norm = false, any_dc = false;
        for (int i = 0; i < n; i++) {
            const DspRow& r = rows[at + (size_t)i];
            max_tiles = std::max(max_tiles, (r.n + kDspTile - 1) / kDspTile);
            any_norm = any_norm || (r.flags & DSP_NORMALIZE);
            any_dc = any_dc || (r.flags & DSP_DC);
        }
        if (max_tiles > INT32_MAX) throw Error(PTTS_EINVAL, "ptts-hip: dsp: too many samples for one launch");
        const int t = R.turn;
        R.turn = (t + 1) % DspRing::kRing;
        if (R.done[t]) PTTS_HIP(hipEventSynchronize(R.done[t]));   // the launches that last read this turn's table have run
        else PTTS_HIP(hipEventCreateWithFlags(&R.done[t], hipEventDisableTiming));
        DspRow* h = R.host + (size_t)t * kRows;
        DspRow* d = R.dev.as<DspRow>() + (size_t)t * kRows;
        std::memcpy(h, rows.data() + at, (size_t)n * sizeof(DspRow));
        PTTS_HIP(hipMemcpyAsync(d, h, (size_t)n * sizeof(DspRow), hipMemcpyHostToDevice, s));
        launch_dsp(d, n, (int)max_tiles, any_norm, any_dc, scan, s);
        PTTS_HIP(hipEventRecord(R.done[t], s));
    }
}

}  // namespace ptts
