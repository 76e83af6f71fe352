// capi_hooks.cpp -- extern "C" test and measurement hooks (include/ptts_debug.h).  NOT part of libptts_hip.so: the Makefile links this file into
// libptts_hooks.so, which depends on libptts_hip.so and is loaded by the tests, tools/ and bench.py's measurement passes only.  The library a host of the
// reference links therefore exports no fault injection, no micro-benchmarks and no launch census.
#include "capi_internal.h"
#include "launch_args.h"
#include "../../include/ptts_debug.h"
#include "scan_block.h"
#include "true_peak.h"

#include <memory>

// How to add a kernel hook (ptts_debug_<kernel> on a ptts_<kernel>_args of host operands).  Keep this order: (1) every argument and bound check -- the
// kernels bound few of their loads, so whatever a launch can touch is checked against the caller's sizes first (check_rows for a RowMap); (2)
// require_device(); (3) the operands through a Stage: in() uploads (a null host pointer stays a null device pointer), out() allocates a result pre-filled
// with 0xff bytes, so whatever the kernel does not store comes back as NaN / FILL and the buffer comes back whole; (4) the kernel's own *_supported
// predicate; (5) the launch inside LaunchScope::run, which counts it in a private census, restores the caller's census also on a throw and merges into it
// only after the launcher returned; (6) hipGetLastError / hipDeviceSynchronize; (7) down() per result, put_str() for every string result.  A forcing global
// (g_gemm3_cfg, g_skinny_stamps, ...) is set through Scoped alone.  What is not a plain upload stays written out in the hook: an in-place residual, NaN
// slack rows, an offset into a buffer.
using namespace ptts;
using namespace ptts::capi;

namespace {

// sets a variable for a scope; the old value comes back when the scope is left, by a throw too
template <class T> class Scoped {
    T& var_;
    T old_;
public:
    Scoped(T& var, T value) : var_(var), old_(var) { var = value; }
    ~Scoped() { var_ = old_; }
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
};

using Census = std::map<std::string, int64_t>;

std::string census_str(const Census& c) {   // "k=v;" per kernel
    std::string s;
    for (const auto& kv : c) s += kv.first + "=" + std::to_string(kv.second) + ";";
    return s;
}

// a capped C string result: at most cap - 1 characters and the terminator; nothing for a null buffer or a cap below 1
void put_str(char* dst, int64_t cap, const std::string& s) {
    if (!dst || cap <= 0) return;
    const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1);
    std::memcpy(dst, s.data(), n);
    dst[n] = 0;
}

// the launches of one hook call: run() notes them in a census of its own and, once the launcher has returned, adds them to a census the caller switched on
// (ptts_debug_launch_counts).  A launcher that throws leaves the caller's census as it was.
class LaunchScope {
    Census seen_;
public:
    template <class F> void run(F&& launch) {
        Census now;
        Census* const callers = g_launch_census;
        {
            Scoped<Census*> install(g_launch_census, &now);
            launch();
        }
        for (const auto& kv : now) {
            seen_[kv.first] += kv.second;
            if (callers) (*callers)[kv.first] += kv.second;
        }
    }
    int64_t count(const char* kernel) const { const auto it = seen_.find(kernel); return it == seen_.end() ? 0 : it->second; }
    int64_t total() const { int64_t all = 0; for (const auto& kv : seen_) all += kv.second; return all; }
    std::string str() const { return census_str(seen_); }
};

// the device buffers of one hook call, freed when it ends
class Stage {
    std::vector<std::unique_ptr<Tmp>> bufs_;
    void* alloc(size_t bytes) { bufs_.emplace_back(new Tmp(bytes)); return bufs_.back()->p; }
public:
    void* in_bytes(const void* host, size_t bytes) {   // (the KV caches: elements of 2 or 4 bytes)
        if (!host) return nullptr;
        void* d = alloc(bytes);
        up(d, host, bytes);
        return d;
    }
    template <class T> T* in(const T* host, size_t count) { return static_cast<T*>(in_bytes(host, count * sizeof(T))); }
    template <class T = float> T* out(size_t count) {
        void* d = alloc(count * sizeof(T));
        if (count) PTTS_HIP(hipMemset(d, 0xff, count * sizeof(T)));
        return static_cast<T*>(d);
    }
};

// a RowMap against its buffer: row m's `width` elements start at off + the map's offset of m and must end inside `elems`; disjoint: no two rows overlap
// (two lanes would store to one element)
void check_rows(const char* hook, const char* what, int64_t M, int64_t elems, const RowMap& map, int64_t off, int64_t width, bool disjoint) {
    std::vector<int64_t> start((size_t)M);
    for (int64_t m = 0; m < M; m++) {
        const int64_t o = off + (map.rows_per_batch ? (m / map.rows_per_batch) * map.batch_stride + (m % map.rows_per_batch) * map.ld : m * map.ld);
        if (o < 0 || o + width > elems)
            throw Error(PTTS_EINVAL, strfmt("%s: row %lld of %s ends at element %lld of %lld", hook, (long long)m, what, (long long)(o + width), (long long)elems));
        start[(size_t)m] = o;
    }
    if (!disjoint) return;
    std::sort(start.begin(), start.end());
    for (size_t i = 1; i < start.size(); i++)
        if (start[i] - start[i - 1] < width) throw Error(PTTS_EINVAL, strfmt("%s: rows of %s overlap (elements %lld and %lld)", hook, what, (long long)start[i - 1], (long long)start[i]));
}

// the operands of the two step-linear probes (ptts_debug_time_skinny, ptts_debug_skinny_stamps): 0x3c bytes everywhere
struct SkinnyProbe {
    Tmp dA, dW, dWt, dC, dlnw;
    GemmArgs g;
    SkinnyFuse fu;
    SkinnyProbe(int M, int N, int K, int w_bf16, int splitk, int fuse_ln)
        : dA((size_t)M * K * 4), dW((size_t)N * K * 4), dWt(step_tiled_bytes((size_t)N, (size_t)K, w_bf16 ? 2 : 4)), dC((size_t)M * N * 4 * (splitk > 1 ? splitk : 1)),
          dlnw((size_t)K * 4) {
        PTTS_HIP(hipMemset(dA.p, 0x3c, (size_t)M * K * 4));
        PTTS_HIP(hipMemset(dW.p, 0x3c, (size_t)N * K * (w_bf16 ? 2 : 4)));
        PTTS_HIP(hipMemset(dlnw.p, 0x3c, (size_t)K * 4));
        PTTS_HIP(hipMemset(dWt.p, 0x3c, step_tiled_bytes((size_t)N, (size_t)K, w_bf16 ? 2 : 4)));
        g.A = dA.as<float>(); g.amap = RowMap{K, 0, 0};
        g.W = dW.p; g.w_bf16 = w_bf16; g.ldw = K; g.Wt = dWt.p;
        g.C = dC.as<float>(); g.cmap = RowMap{N, 0, 0};
        g.M = M; g.N = N; g.K = K;
        if (fuse_ln) { fu.ln = 1; fu.ln_w = dlnw.as<float>(); fu.ln_b = dlnw.as<float>(); }
        if (!(fuse_ln ? skinny_fuse_supported(g, fu) : skinny_supported(g, splitk))) throw Error(PTTS_EINVAL, "shape not supported");
    }
    void launch(int splitk) { launch_skinny(g, fu, splitk, dC.as<float>(), nullptr); }
};

}  // namespace

extern "C" {

int ptts_decode_stages(ptts_model* h, const float* latents, int32_t n_utt, int32_t frames, float* pcm, float* mimi_latent, float* transformer_out) {
    return decode_stages(h, latents, n_utt, frames, pcm, mimi_latent, transformer_out);
}

int ptts_debug_encode_stages(ptts_model* h, const float* pcm, int64_t n_samples, float* const* stages, int64_t* shapes) {
    if (stages || !shapes) {
        float* lat = stages ? stages[kEncStages - 1] : nullptr;
        std::vector<float> own;
        if (stages && !lat && h && h->m) {   // (the latent is always produced: a temporary buffer when stage 9 is not asked for)
            own.resize((size_t)std::max<int64_t>(ptts_mimi_encode_frames(n_samples), 1) * h->m->d.mimi_dim);
            lat = own.data();
        }
        const int rc = encode_stages(h, &pcm, &n_samples, 1, &lat, stages ? stages : nullptr);
        if (rc != PTTS_OK || !shapes) return rc;
    }
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        require_encoder(h->m->d);
        mimi_encode_stage_shapes(h->m->d, n_samples, shapes);
    });
}

const char* ptts_debug_last_attention_kernel(void) { return g_last_attn_kernel; }

int ptts_debug_flow_cluster_inject(ptts_model* h, int32_t block) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        if (block < 0 || block > h->m->d.flow_depth) throw Error(PTTS_EINVAL, "ptts-hip: flow-net block out of range");
        std::lock_guard<std::mutex> lock(h->m->mu);
        h->m->fc_inject = block;
    });
}

// k_flow_cluster on host operands: a SEQUENCE of launches on one granule buffer and one set of tag words, FlowClusterArgs filled as step.cpp step_flow
// fills them.  The kernel's workgroups spin on each other, so nothing is launched that the batch set-up would not launch: flow_cluster_fits and
// flow_cluster_supported are asked, inject and stamps stay at their defaults (there is no argument that reaches them).
int ptts_debug_flow_cluster(const ptts_flow_cluster_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_flow_cluster: null argument");
        const ptts_flow_cluster_args& t = *pa;
        constexpr int C = 512, kSlack = 3;
        constexpr int kMaxRows = kFlowClusterMaxTiles * kFlowClusterRows;
        if (t.rows < 1 || t.rows > kMaxRows) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: %d rows, the kernel takes 1..%d", t.rows, kMaxRows));
        if (t.depth < 1 || t.depth > FC_MAX_DEPTH) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: depth %d outside 1..%d", t.depth, FC_MAX_DEPTH));
        if (t.ldmod % 4 != 0 || t.ldmod < (int64_t)3 * t.depth * C)
            throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: ldmod %lld: a multiple of 4 and at least 3 depth 512 = %d", (long long)t.ldmod, 3 * t.depth * C));
        if (t.ldmod > (1 << 16)) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: ldmod %lld above 65536", (long long)t.ldmod));
        if (t.n_launch < 1 || t.n_launch > 8) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: %d launches, the hook takes 1..8", t.n_launch));
        if (t.in_place != 0 && t.in_place != 1) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: in_place %d is neither 0 nor 1", t.in_place));
        if (!t.fx || !t.ada || !t.ln_w || !t.ln_b || !t.b0 || !t.b2 || !t.eps || !t.w0 || !t.w2 || !t.launch_rows || !t.out || !t.state || (!t.in_place && !t.fx_back))
            throw Error(PTTS_EINVAL, "ptts_debug_flow_cluster: null operand");
        for (int i = 0; i < t.n_launch; i++)
            if (t.launch_rows[i] < 1 || t.launch_rows[i] > t.rows)
                throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: launch %d of %d rows, the operands hold %d", i, t.launch_rows[i], t.rows));
        if (t.tag_base0 & 1u) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: tag_base0 %u is odd (a launch's base is even: h tags are odd, x tags even)", t.tag_base0));
        const int rows = t.rows, depth = t.depth, L = t.n_launch;
        // weights: rounded to bf16 and tiled by the loader's packer (what Lin::wt holds)
        const size_t wbytes = step_tiled_bytes((size_t)C, (size_t)C, 2);
        std::vector<uint8_t> wt((size_t)2 * depth * wbytes);
        for (int r = 0; r < depth; r++) {
            pack_step_tiled(t.w0 + (size_t)r * C * C, (size_t)C, (size_t)C, true, wt.data() + (size_t)(2 * r) * wbytes);
            pack_step_tiled(t.w2 + (size_t)r * C * C, (size_t)C, (size_t)C, true, wt.data() + (size_t)(2 * r + 1) * wbytes);
        }
        require_device();
        int device = 0;
        PTTS_HIP(hipGetDevice(&device));
        if (!flow_cluster_fits(rows, device)) throw Error(PTTS_EINVAL, strfmt("ptts_debug_flow_cluster: the grid of %d rows is not resident at once on this device (flow_cluster_fits)", rows));
        const size_t row_bytes = (size_t)C * 4, buf_rows = (size_t)rows + kSlack, vec =(size_t)depth * C;
        Stage st;
        Tmp dX(flow_cluster_xbuf_bytes(rows)), dSync(kFlowClusterSyncBytes);
        const uint8_t* dW = st.in(wt.data(), wt.size());
        float* dAda = st.out(buf_rows * (size_t)t.ldmod);   // (NaN slack rows behind `rows`)
        up(dAda, t.ada, (size_t)rows * t.ldmod * 4);
        const float *dLw = st.in(t.ln_w, vec), *dLb = st.in(t.ln_b, vec), *dB0 = st.in(t.b0, vec), *dB2 = st.in(t.b2, vec);
        // every launch its own copy of the rows it takes: NaN behind them (in place that is what the rows at and beyond launch_rows keep)
        float *dIn = st.out((size_t)L * buf_rows * C), *dOut = st.out((size_t)L * buf_rows * C);
        for (int i = 0; i < L; i++) up(dIn + (size_t)i * buf_rows * C, t.fx, (size_t)t.launch_rows[i] * row_bytes);
        // the exchange state as batch.cpp sets it up (zeroes), then the tag words at tag_base0
        PTTS_HIP(hipMemset(dX.p, 0, flow_cluster_xbuf_bytes(rows))); PTTS_HIP(hipMemset(dSync.p, 0, kFlowClusterSyncBytes));
        std::vector<uint32_t> sync(kFlowClusterSyncBytes / 4, 0u);
        for (int tile = 0; tile < kFlowClusterMaxTiles; tile++) sync[(size_t)tile * 32] = t.tag_base0;
        up(dSync.p, sync.data(), kFlowClusterSyncBytes);
        auto read_state = [&] {
            down(sync.data(), dSync.p, kFlowClusterSyncBytes);
            for (int tile = 0; tile < kFlowClusterMaxTiles; tile++) t.state[tile] = sync[(size_t)tile * 32];
            t.state[kFlowClusterMaxTiles] = sync[(size_t)32 * kFlowClusterMaxTiles];
        };
        LaunchScope launches;   // (one scope around the whole sequence: a launch that is refused or throws leaves a caller's census without the earlier ones too)
        int faulted = -1;
        launches.run([&] {
            for (int i = 0; i < L && faulted < 0; i++) {
                FlowClusterArgs fa;   // as step_flow fills them
                float* in = dIn + (size_t)i * buf_rows * C;
                fa.fx_in = in; fa.fx_out = t.in_place ? in : dOut + (size_t)i * buf_rows * C;
                fa.ada = dAda; fa.ldmod = t.ldmod; fa.rows = t.launch_rows[i]; fa.depth = depth;
                for (int r = 0; r < depth; r++) {
                    fa.eps[r] = t.eps[r]; fa.ln_w[r] = dLw + (size_t)r * C; fa.ln_b[r] = dLb + (size_t)r * C;
                    fa.w0[r] = dW + (size_t)(2 * r) * wbytes; fa.b0[r] = dB0 + (size_t)r * C;
                    fa.w2[r] = dW + (size_t)(2 * r + 1) * wbytes; fa.b2[r] = dB2 + (size_t)r * C;
                }
                fa.xbuf = dX.as<unsigned long long>(); fa.sync = dSync.as<unsigned>();
                if (!flow_cluster_supported(fa, C)) throw Error(PTTS_EINVAL, "ptts_debug_flow_cluster: refused by flow_cluster_supported");
                launch_flow_cluster(fa, nullptr);
                PTTS_HIP(hipGetLastError());
                PTTS_HIP(hipDeviceSynchronize());
                uint32_t fault = 0;
                down(&fault, dSync.as<uint32_t>() + (size_t)32 * kFlowClusterMaxTiles, 4);
                if (fault) faulted = i;   // (nothing is retried, nothing more is launched on this state)
            }
        });
        put_str(t.launched, t.launched_cap, launches.str());
        read_state();
        for (int i = 0; i < L; i++) {
            down(t.out + (size_t)i * rows * C, (t.in_place ? dIn : dOut) + (size_t)i * buf_rows * C, (size_t)rows * row_bytes);
            if (!t.in_place) down(t.fx_back + (size_t)i * rows * C, dIn + (size_t)i * buf_rows * C, (size_t)rows * row_bytes);
        }
        if (faulted >= 0)
            throw Error(PTTS_ENODEVICE, strfmt("ptts_debug_flow_cluster: the in-launch hand-off timed out (k_flow_cluster), launch %d of %d; nothing is retried", faulted, L));
    });
}

int64_t ptts_debug_resample_launches(int32_t reset) {
    return reset ? g_resample_launches.exchange(0) : g_resample_launches.load();
}

int ptts_debug_dsp_blocked_host(const float* in, int64_t n, float* out) {
    return guard([&] {
        if (n < 0 || (n > 0 && (!in || !out))) throw Error(PTTS_EINVAL, "ptts-hip: dsp: null argument");
        if (n > 0 && out != in) std::memmove(out, in, (size_t)n * sizeof(float));
        dsp_dc_block_blocked(out, n, kNativeRate);
    });
}

int ptts_debug_dsp_windows(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, const ptts_dsp_opts* opts, const int64_t* cuts, int32_t n_cuts,
                           float* const* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native: model is not fully initialized");
        if (rows < 0 || n_cuts < 0 || (rows > 0 && (!in || !n || !out)) || (n_cuts > 0 && !cuts)) throw Error(PTTS_EINVAL, "ptts-hip: dsp: windows: null argument");
        DspSpec spec;
        std::string e = dsp_resolve(opts, &spec);
        if (e.empty()) e = dsp_trim_refusal(spec);
        if (e.empty()) e = dsp_tempo_refusal(spec);
        if (e.empty()) e = dsp_pitch_refusal(spec);
        if (e.empty()) e = dsp_window_refusal(spec);   // only the causal stages, as the streamed joined call words it
        if (!e.empty()) throw Error(PTTS_EINVAL, "ptts-hip: " + e);
        for (int i = 0; i < rows; i++)
            if (n[i] < 0 || (n[i] > 0 && (!in[i] || !out[i]))) throw Error(PTTS_EINVAL, strfmt("ptts-hip: dsp: windows: row %d is negative or null", i));
        const int64_t fo = spec.fade_out_ms > 0 ? (int64_t)(spec.fade_out_ms / 1000.0 * (double)kNativeRate) : 0;
        for (int w = 0; w < n_cuts; w++) {
            if (cuts[w] <= (w ? cuts[w - 1] : 0) || cuts[w] % kDspTile != 0)
                throw Error(PTTS_EINVAL, strfmt("ptts-hip: dsp: windows: cut %d (%lld) is not an ascending multiple of %d above 0", w, (long long)cuts[w], kDspTile));
            for (int i = 0; i < rows; i++)
                if (cuts[w] < n[i] && cuts[w] > n[i] - fo)
                    throw Error(PTTS_EINVAL, strfmt("ptts-hip: dsp: windows: cut %d (%lld) lies in the fade out of row %d (%lld samples, the last %lld fade out)", w,
                                                    (long long)cuts[w], i, (long long)n[i], (long long)fo));
        }
        if (!spec.any()) {   // nothing switched on: a copy, no launch
            for (int i = 0; i < rows; i++) if (n[i] > 0 && out[i] != in[i]) std::memmove(out[i], in[i], (size_t)n[i] * sizeof(float));
            return;
        }
        dsp_windows_device(*h->m, in, n, rows, spec, cuts, n_cuts, out);
    });
}

int ptts_debug_loudness_energies(ptts_model* h, const float* const* in, const int64_t* n, int32_t rows, double* const* out) {
    return guard([&] {
        if (rows < 0 || (rows > 0 && (!in || !n || !out))) throw Error(PTTS_EINVAL, "ptts-hip: loudness: null argument");
        for (int i = 0; i < rows; i++)
            if (n[i] < 0 || (n[i] > 0 && !in[i]) || (n[i] >= kLoudSub && !out[i])) throw Error(PTTS_EINVAL, strfmt("ptts-hip: loudness: row %d is negative or null", i));
        std::vector<std::vector<double>> sub((size_t)rows);
        if (h) {
            if (!h->m) throw Error(PTTS_EINVAL, "native: model is not fully initialized");
            DspSpec spec;
            dsp_spec_loudness(spec, nullptr);
            dsp_rows_device(*h->m, in, n, rows, std::vector<DspSpec>((size_t)rows, spec).data(), false, {nullptr, nullptr, sub.data()});
        } else {
            for (int i = 0; i < rows; i++) loud_sub_energies(in[i], n[i], sub[(size_t)i]);
        }
        for (int i = 0; i < rows; i++)
            if (n[i] >= kLoudSub) std::memcpy(out[i], sub[(size_t)i].data(), (size_t)(n[i] / kLoudSub) * sizeof(double));
    });
}

int ptts_debug_kweighting(int32_t sample_rate, double out[10]) {
    return guard([&] {
        if (!out || sample_rate <= 0) throw Error(PTTS_EINVAL, "ptts-hip: loudness: bad argument");
        loud_kweight_coeffs(sample_rate, out);
    });
}

int64_t ptts_debug_dsp_opts_error(const ptts_dsp_opts* opts, char* out, int64_t cap) {
    const std::string s = opts ? dsp_opts_error(*opts) : std::string();
    put_str(out, cap, s);
    return (int64_t)s.size();
}

int ptts_debug_true_peak_taps(float* out, int32_t* L, int32_t* K, int32_t* dlo) {
    if (L) *L = kTpPhases;
    if (K) *K = kTpTaps;
    if (dlo) *dlo = kTpDlo;
    const TpTaps& t = tp_taps();
    if (out)
        for (int p = 0; p < kTpPhases; p++)
            for (int k = 0; k < kTpTaps; k++) out[p * kTpTaps + k] = t.h[k][p];
    return PTTS_OK;
}

int ptts_debug_true_peak_oversample(const float* samples, int64_t n, float* y) {
    return guard([&] {
        if (n < 0 || (n > 0 && (!samples || !y))) throw Error(PTTS_EINVAL, "ptts-hip: true peak: null argument");
        (void)tp_measure(samples, n, y);
    });
}

int64_t ptts_debug_launch_counts(int32_t on, char* out, int64_t cap) {
    static thread_local Census census;
    const std::string s = census_str(census);
    put_str(out, cap, s);
    census.clear();
    g_launch_census = on ? &census : nullptr;
    return (int64_t)s.size();
}

// timing aid (tools/microbench.py): `iters` back-to-back launches of the step linear on random operands
int ptts_debug_time_skinny(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t splitk, int32_t fuse_ln, int32_t iters, float* avg_us) {
    return guard([&] {
        require_device();
        SkinnyProbe p(M, N, K, w_bf16, splitk, fuse_ln);
        hipEvent_t e0, e1;
        PTTS_HIP(hipEventCreate(&e0)); PTTS_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 5; i++) p.launch(splitk);
        PTTS_HIP(hipDeviceSynchronize());
        PTTS_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; i++) p.launch(splitk);
        PTTS_HIP(hipEventRecord(e1, nullptr));
        PTTS_HIP(hipEventSynchronize(e1));
        float ms = 0;
        PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = ms * 1e3f / (float)iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    });
}

// debug: one stamped launch of the step linear (after warm-up); out receives 8 ticks per block, *n_blocks the block count
int ptts_debug_skinny_stamps(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t splitk, int32_t fuse_ln, uint64_t* out, int32_t max_blocks,
                             int32_t* n_blocks) {
    return guard([&] {
        require_device();
        SkinnyProbe p(M, N, K, w_bf16, splitk, fuse_ln);
        const int blocks = ((N + 15) / 16) * ((M + 15) / 16) * (splitk > 1 ? splitk : 1);   // upper bound: the narrow-block variant has N/16 column blocks
        Tmp dS((size_t)blocks * 8 * 8);
        PTTS_HIP(hipMemset(dS.p, 0, (size_t)blocks * 64));
        for (int i = 0; i < 3; i++) p.launch(splitk);
        PTTS_HIP(hipDeviceSynchronize());
        {
            Scoped<unsigned long long*> stamped(g_skinny_stamps, dS.as<unsigned long long>());
            p.launch(splitk);
        }
        PTTS_HIP(hipDeviceSynchronize());
        *n_blocks = blocks;
        down(out, dS.p, (size_t)std::min(blocks, max_blocks) * 64);
    });
}

// debug: one whole AR step of a prompted batch with every stampable launch of the step linear stamped in place (cold caches, the
// real operands).  out: [cap_blocks][8] ticks; desc: [cap_desc][8] = M, N, K, prologue, NJ, CG, blocks, splitk per launch
int ptts_debug_step_stamps(ptts_batch* hb, int32_t lsd_steps, uint64_t* out, int64_t cap_blocks, int32_t* desc, int32_t cap_desc, int32_t* n_desc) {
    return guard([&] {
        if (!hb || !hb->b || !out || !desc || !n_desc) throw Error(PTTS_EINVAL, "ptts-hip: null argument");
        Model& m = *hb->m;
        Batch& b = *hb->b;
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        for (int i = 0; i < b.B; i++)
            if (b.kv_len_host[i] + 1 > b.cap) throw Error(PTTS_EINVAL, "ptts-hip: KV capacity exhausted");
        m.tcomb_for(lsd_steps);
        Tmp ds((size_t)cap_blocks * 64);
        PTTS_HIP(hipMemsetAsync(ds.p, 0, (size_t)cap_blocks * 64, m.stream));
        PTTS_HIP(hipMemsetAsync(b.cur.p, 0, (size_t)b.B * m.d.ldim * sizeof(float), m.stream));
        SkinnyStampLog lg;
        lg.base = ds.as<unsigned long long>(); lg.cap_blocks = (size_t)cap_blocks;
        {
            Scoped<SkinnyStampLog*> logged(g_skinny_stamp_log, &lg);
            step_core(b, lsd_steps);
        }
        for (int i = 0; i < b.B; i++) b.kv_len_host[i] += 1;
        PTTS_HIP(hipMemcpyAsync(b.st.kv_len, b.kv_len_host.data(), (size_t)b.B * sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
        PTTS_HIP(hipStreamSynchronize(m.stream));
        if (b.fc_ok) {   // (a stamped step whose cluster hand-off timed out measured nothing)
            unsigned fault = 0;
            down(&fault, b.fc_fault(), sizeof fault);
            if (fault) flow_cluster_fault(b);
        }
        down(out, ds.p, lg.used_blocks * 64);
        const int n = (int)std::min<size_t>(lg.desc.size(), (size_t)cap_desc);
        for (int i = 0; i < n; i++) std::memcpy(desc + 8 * i, &lg.desc[(size_t)i], 32);
        *n_desc = n;
    });
}

// debug: time one many-row GEMM variant (2 = k_gemm2, 3 = k_gemm3) and compare it with the other one on pseudo-random data
int ptts_debug_gemm(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t variant, int32_t epi_flags, int32_t iters, float* avg_us, float* maxdiff) {
    return guard([&] {
        require_device();
        // epi_flags: the epilogue form in the low byte; 0x100: RoPE on the first two thirds of the columns (positions restart every
        // 2000 rows: the decoder's qkv projection); 0x200: the residual is read from the output buffer itself (the decoder's
        // out_proj / linear2), 0x400: activations behind a prologue ELU, 0x800: a per-column scale
        const int epi = epi_flags & 0xff;
        const bool rope = epi_flags & 0x100, inplace = epi_flags & 0x200;
        const size_t na = (size_t)M * K, nw = (size_t)N * K, nc1 = (size_t)M * N;
        const int S = (epi_flags & 0x4000) ? K / 1024 : 1;   // 0x4000: split-K in 1024-deep slices (raw sums, plane z at C + z M N)
        if (S < 1 || (S > 1 && K % 1024)) throw Error(PTTS_EINVAL, "split-K probe needs K % 1024 == 0");
        const size_t nc = nc1 * (size_t)S;       // values compared: every plane
        std::vector<float> ha(na), hw(nw), hb((size_t)N);
        uint32_t st = 12345u;
        auto rnd = [&] { st = st * 1664525u + 1013904223u; return ((float)(st >> 8) / 8388608.0f) - 1.0f; };
        for (auto& x : ha) x = rnd();
        for (auto& x : hw) x = rnd() * 0.05f;
        for (auto& x : hb) x = rnd();
        Tmp dA(na * 4), dW(nw * 4), dB((size_t)N * 4), dC(nc * 4), dC2(nc * 4), dR(nc * 4), dCos(2000 * 32 * 4), dSin(2000 * 32 * 4);
        up(dA.p, ha.data(), na * 4); up(dB.p, hb.data(), (size_t)N * 4);
        if (w_bf16) {
            std::vector<uint16_t> hw16(nw);
            for (size_t i = 0; i < nw; i++) hw16[i] = f32_to_bf16_rne(hw[i]);
            up(dW.p, hw16.data(), nw * 2);
        } else up(dW.p, hw.data(), nw * 4);
        if (inplace) {   // a residual with content: the first nc values of the activations' generator, continued
            std::vector<float> hr(nc);
            for (auto& x : hr) x = rnd();
            up(dR.p, hr.data(), nc * 4);
        } else PTTS_HIP(hipMemset(dR.p, 0, nc * 4));
        if (rope) {
            std::vector<float> hc(2000 * 32), hs(2000 * 32);
            for (size_t i = 0; i < hc.size(); i++) { const float ang = rnd() * 3.14159265f; hc[i] = std::cos(ang); hs[i] = std::sin(ang); }
            up(dCos.p, hc.data(), hc.size() * 4); up(dSin.p, hs.data(), hs.size() * 4);
        }
        GemmArgs g;
        g.A = dA.as<float>(); g.amap = RowMap{K, 0, 0};
        g.W = dW.p; g.w_bf16 = w_bf16; g.ldw = K; g.bias = dB.as<float>();
        g.C = dC.as<float>(); g.cmap = RowMap{N, 0, 0};
        g.R = dR.as<float>(); g.epi = epi;
        g.M = M; g.N = N; g.K = K;
        if (epi_flags & 0x400) g.aop = AOP_ELU;
        if (S > 1) { g.kslice = 1024; g.zstride = (int64_t)nc1; g.bias = nullptr; }
        if (epi_flags & 0x800) g.scale = dB.as<float>();   // a per-column scale (the decoder's layer scale): the bias values serve
        if (rope) {
            g.rope_cos = dCos.as<float>(); g.rope_sin = dSin.as<float>(); g.rope_cols = N / 3 * 2; g.rope_hd = 64; g.rope_pos0 = 0; g.rope_rows_per_seg = 2000;
            g.bias = nullptr;
        }
        if (!gemm3_supported(g)) throw Error(PTTS_EINVAL, "shape not supported");
        // variant 2: k_gemm2, 3: k_gemm3 (30 + cfg: a forced shape), 40: whatever launch_gemm dispatches (k_gemm_wres where it applies),
        // 50 + cfg: k_gemm5
        auto run = [&](int v, float* c) {
            GemmArgs h = g; h.C = c;
            if (inplace) { PTTS_HIP(hipMemcpyAsync(c, dR.p, nc * 4, hipMemcpyDeviceToDevice, nullptr)); h.R = c; }
            if (v == 40) { if (rope) { if (!launch_gemm_rope(h, nullptr)) throw Error(PTTS_EINVAL, "no RoPE epilogue for this shape"); } else launch_gemm(h, nullptr); }
            else if (v >= 50) { if (!gemm5_supported(h)) throw Error(PTTS_EINVAL, "shape not supported by k_gemm5"); Scoped<int> cfg(g_gemm5_cfg, v - 50); launch_gemm5(h, nullptr); }
            else if (v >= 3) { Scoped<int> cfg(g_gemm3_cfg, v >= 30 ? v - 30 : 0); launch_gemm3(h, nullptr); }
            else { if (!gemm2_supported(h)) throw Error(PTTS_EINVAL, "shape not supported by k_gemm2"); launch_gemm2(h, nullptr); }
        };
        hipEvent_t e0, e1;
        PTTS_HIP(hipEventCreate(&e0)); PTTS_HIP(hipEventCreate(&e1));
        for (int i = 0; i < 2; i++) run(variant, dC.as<float>());
        PTTS_HIP(hipDeviceSynchronize());
        PTTS_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; i++) run(variant, dC.as<float>());
        PTTS_HIP(hipEventRecord(e1, nullptr));
        PTTS_HIP(hipEventSynchronize(e1));
        float ms = 0;
        PTTS_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = ms * 1e3f / (float)iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *maxdiff = -1.0f;
        if (nc <= ((size_t)200 << 20)) {
            // against k_gemm3 (k_gemm2 for k_gemm3 itself): the same k order, so equal bits are expected; and the variant against itself,
            // three more runs (a race shows as a difference between runs)
            run(variant >= 40 ? 3 : (variant >= 3 ? 2 : 3), dC2.as<float>());
            PTTS_HIP(hipDeviceSynchronize());
            std::vector<float> c1(nc), c2(nc);
            down(c1.data(), dC.p, nc * 4); down(c2.data(), dC2.p, nc * 4);
            float md = 0;
            size_t nbad = 0;
            for (size_t i = 0; i < nc; i++) {
                float d = std::fabs(c1[i] - c2[i]);
                if (!(d <= md)) md = d;
                if (d != 0 && nbad++ < 12) fprintf(stderr, "ptts_debug_gemm: variant %d vs reference at plane %zu row %zu column %zu: %.9g vs %.9g\n", variant, i / nc1, (i % nc1) / N, i % N, c1[i], c2[i]);
            }
            if (nbad) fprintf(stderr, "ptts_debug_gemm: %zu of %zu values differ from the reference kernel's\n", nbad, nc);
            for (int rep = 0; rep < 3; rep++) {
                run(variant, dC2.as<float>());
                PTTS_HIP(hipDeviceSynchronize());
                down(c2.data(), dC2.p, nc * 4);
                if (memcmp(c1.data(), c2.data(), nc * 4) != 0) {
                    size_t bad = 0, first = nc;
                    for (size_t i = 0; i < nc; i++) if (memcmp(&c1[i], &c2[i], 4) != 0) { if (first == nc) first = i; bad++; }
                    fprintf(stderr, "ptts_debug_gemm: variant %d differs from itself between runs: %zu of %zu values, first at row %zu column %zu\n", variant, bad, nc, first / N, first % N);
                    md = 1e30f;
                }
            }
            *maxdiff = md;
        }
    });
}

// The AR step's 128+-row linears (csrc/tall.hip) on host operands: ONE launch of k_rowprep, ONE of k_tall, or the two chained.  Neither kernel bounds a load or
// a store by a buffer size, so every leading dimension and stride is checked against the buffers allocated here (`rows` rows each) before anything is uploaded;
// the widths themselves (D = 512 / 1024, K % 128, N % 4) are the predicates' to refuse.
int ptts_debug_tall(const ptts_tall_args* pa) {
    return guard([&] {
        const char* const me = "ptts_debug_tall";
        if (!pa) throw Error(PTTS_EINVAL, strfmt("%s: null argument", me));
        const ptts_tall_args& t = *pa;
        put_str(t.launched, t.launched_cap, "");
        const bool prep = t.op == PTTS_TALL_ROWPREP || t.op == PTTS_TALL_BOTH, prod = t.op == PTTS_TALL_TALL || t.op == PTTS_TALL_BOTH;
        if (!prep && !prod) throw Error(PTTS_EINVAL, strfmt("%s: unknown op %d", me, t.op));
        if (!t.x || t.M < 1 || t.rows < t.M || t.rows > 1024 || t.K < 1 || t.K > 8192)
            throw Error(PTTS_EINVAL, strfmt("%s: bad arguments (x, 1 <= M <= rows <= 1024, 1 <= K <= 8192)", me));
        const int M = t.M, K = t.K, N = t.N, S = t.splitk;
        const size_t rows = (size_t)t.rows;
        if (prep) {
            if (t.ldx < K || t.ldy < K) throw Error(PTTS_EINVAL, strfmt("%s: ldx %lld or ldy %lld below the row width %d", me, (long long)t.ldx, (long long)t.ldy, K));
            if (t.psplit < 0 || t.psplit > 16 || (t.psplit > 0) != (t.planes != nullptr)) throw Error(PTTS_EINVAL, strfmt("%s: psplit %d does not fit planes", me, t.psplit));
            if (t.pbias && !t.planes) throw Error(PTTS_EINVAL, strfmt("%s: pbias without planes (k_rowprep would ignore it)", me));
            if (t.psplit > 0 && t.pstride < (int64_t)rows * K) throw Error(PTTS_EINVAL, strfmt("%s: pstride %lld below rows K = %lld", me, (long long)t.pstride, (long long)rows * K));
        }
        if (prod) {
            if (!t.W || N < 1 || N > 8192) throw Error(PTTS_EINVAL, strfmt("%s: bad arguments (W, 1 <= N <= 8192)", me));
            if (t.form != 0 && t.form != 32 && t.form != 64) throw Error(PTTS_EINVAL, strfmt("%s: form %d: k_tall has blocks of 32 and 64 rows", me, t.form));
            if (S < 1 || S > 16) throw Error(PTTS_EINVAL, strfmt("%s: splitk %d outside [1, 16]", me, S));
            if (prep ? t.lda != t.ldy : t.lda < K) throw Error(PTTS_EINVAL, strfmt("%s: lda %lld (at least K; chained: ldy)", me, (long long)t.lda));
            if (t.R && t.ldr < N) throw Error(PTTS_EINVAL, strfmt("%s: ldr %lld below N", me, (long long)t.ldr));
            if ((t.ch != nullptr) != (t.cl != nullptr) || (t.ch && t.ldp < N)) throw Error(PTTS_EINVAL, strfmt("%s: ch / cl / ldp %lld do not fit", me, (long long)t.ldp));
            if ((S > 1 || !t.ch) && !t.out) throw Error(PTTS_EINVAL, strfmt("%s: no result buffer", me));
            if (S > 1 && t.zstride < (int64_t)rows * N) throw Error(PTTS_EINVAL, strfmt("%s: zstride %lld below rows N = %lld", me, (long long)t.zstride, (long long)rows * N));
            if (S == 1 && !t.ch && t.ldc < N) throw Error(PTTS_EINVAL, strfmt("%s: ldc %lld below N", me, (long long)t.ldc));
        }
        require_device();
        Stage st;
        PrepArgs p;
        TallArgs g;
        uint16_t *dYh = nullptr, *dYl = nullptr, *dCh = nullptr, *dCl = nullptr;
        float *dXo = nullptr, *dYo = nullptr, *dOut = nullptr;
        size_t out_elems = 0;
        int form = 0, grid[3] = {rowprep_blocks(M), 1, 1};
        if (prep) {
            dYh = st.out<uint16_t>(rows * t.ldy); dYl = st.out<uint16_t>(rows * t.ldy);
            dXo = st.out(rows * K); dYo = st.out(rows * K);
            p.x = st.in(t.x, rows * t.ldx); p.ldx = t.ldx;
            if (t.psplit > 0) p.pend = PendingSum{st.in(t.planes, (size_t)t.psplit * t.pstride), t.psplit, t.pstride, st.in(t.pbias, (size_t)K)};
            p.x_out = t.want_x_out ? dXo : nullptr; p.y_out = t.want_y_out ? dYo : nullptr;
            p.ln_w = st.in(t.ln_w, (size_t)K); p.ln_b = st.in(t.ln_b, (size_t)K); p.eps = t.eps;
            p.yh = dYh; p.yl = dYl; p.ldy = t.ldy; p.M = M; p.D = K;
            if (!rowprep_supported(p)) throw Error(PTTS_EINVAL, strfmt("%s: refused by rowprep_supported", me));
        }
        if (prod) {
            // the weights in the step kernels' fragment order, rounded to bf16: the loader's packer
            std::vector<uint8_t> wt(step_tiled_bytes((size_t)N, (size_t)K, 2));
            pack_step_tiled(t.W, (size_t)N, (size_t)K, true, wt.data());
            if (prep) { g.ah = dYh; g.al = dYl; }
            else {   // the rows as they are: split on the host the way the kernels split (hi = bf16(x), lo = bf16(x - hi))
                const size_t n = rows * t.lda;
                std::vector<uint16_t> hi(n), lo(n);
                for (size_t i = 0; i < n; i++) { hi[i] = f32_to_bf16_rne(t.x[i]); lo[i] = f32_to_bf16_rne(t.x[i] - bf16_to_f32(hi[i])); }
                g.ah = st.in(hi.data(), n); g.al = st.in(lo.data(), n);
            }
            g.lda = t.lda; g.Wt = st.in(wt.data(), wt.size()); g.bias = st.in(t.bias, (size_t)N);
            if (t.R) { g.R = st.in(t.R, rows * t.ldr); g.ldr = t.ldr; }
            g.M = M; g.N = N; g.K = K; g.epi = t.epi;
            if (S > 1) { out_elems = (size_t)S * t.zstride; dOut = st.out(out_elems); g.splitk = S; g.partial = dOut; g.zstride = t.zstride; }
            else if (!t.ch) { out_elems = rows * t.ldc; dOut = st.out(out_elems); g.C = dOut; g.ldc = t.ldc; }
            if (t.ch) { dCh = st.out<uint16_t>(rows * t.ldp); dCl = st.out<uint16_t>(rows * t.ldp); g.ch = dCh; g.cl = dCl; g.ldp = t.ldp; }
            if (!tall_supported(g)) throw Error(PTTS_EINVAL, strfmt("%s: refused by tall_supported", me));
            form = t.form ? t.form : tall_rows(M);
            tall_grid(g, form, grid);
        }
        LaunchScope launches;
        launches.run([&] {
            if (prep) launch_rowprep(p, nullptr);
            if (prod) launch_tall_as(g, form, nullptr);
        });
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        put_str(t.launched, t.launched_cap, launches.str());
        if (t.form_out) *t.form_out = form;
        if (t.grid) for (int i = 0; i < 3; i++) t.grid[i] = grid[i];
        if (prep) {
            if (t.x_out) down(t.x_out, dXo, rows * K * 4);
            if (t.y_out) down(t.y_out, dYo, rows * K * 4);
            if (t.yh) down(t.yh, dYh, rows * t.ldy * 2);
            if (t.yl) down(t.yl, dYl, rows * t.ldy * 2);
        }
        if (dOut && t.out) down(t.out, dOut, out_elems * 4);
        if (dCh) { down(t.ch, dCh, rows * t.ldp * 2); down(t.cl, dCl, rows * t.ldp * 2); }
    });
}

// The step linear (csrc/skinny.hip) on host operands.  The weights go through the loader's own packers (model.h).
int ptts_debug_step_linear(const ptts_step_linear_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_step_linear: null argument");
        const ptts_step_linear_args& t = *pa;
        if (!t.x || !t.W || !t.C || t.M <= 0 || t.N <= 0 || t.K <= 0 || t.lda < t.K || t.ldc < t.N || t.wfmt < 0 || t.wfmt > 2 || t.epi < EPI_NONE || t.epi > EPI_RESADD_ELU ||
            t.splitk < 1 || t.splitk > 64 || t.psplit < 0 || (t.path != 0 && t.path != 1) || (t.zrows != 0 && t.zrows < t.M))
            throw Error(PTTS_EINVAL, "ptts_debug_step_linear: bad arguments");
        const int M = t.M, N = t.N, K = t.K, S = t.splitk;
        const bool fused = t.ln || t.planes || t.shift || t.mscale || t.ln_w || t.ln_b || t.pgate;
        if ((t.epi >= EPI_RESADD && !t.R) || (t.epi == EPI_SCALE_RESADD && !t.scale) || (t.epi == EPI_GATE_RESADD && (!t.gate || t.ldg < N)) || (t.tail && !t.tail_out) ||
            (t.planes && t.psplit < 1) || ((t.shift || t.mscale) && t.ldmod < K) || (fused && S > 1) || (t.tail && S > 1) || (t.path == 1 && (fused || S > 1)) ||
            (t.wfmt == 2 && (!t.w_eff || !t.w_scale)))
            throw Error(PTTS_EINVAL, "ptts_debug_step_linear: operands do not fit the form asked for");
        const size_t nk = (size_t)N * K, mk = (size_t)M * K;
        // weights: the loader's packers
        std::vector<float> rm(t.W, t.W + nk), wscale;
        std::vector<uint8_t> wt(step_tiled_bytes((size_t)N, (size_t)K, t.wfmt == 2 ? 1 : (t.wfmt == 1 ? 2 : 4)));
        std::vector<uint16_t> rm16;
        if (t.wfmt == 2) {
            std::vector<int8_t> q;
            quantize_rows(rm, (size_t)N, (size_t)K, wscale, q);   // rm -> W^
            pack_step_tiled_i8(q.data(), (size_t)N, (size_t)K, wt.data());
            std::memcpy(t.w_eff, rm.data(), nk * 4);
            std::memcpy(t.w_scale, wscale.data(), (size_t)N * 4);
        } else {
            pack_step_tiled(rm.data(), (size_t)N, (size_t)K, t.wfmt == 1, wt.data());
            if (t.wfmt == 1) { rm16.resize(nk); for (size_t i = 0; i < nk; i++) rm16[i] = f32_to_bf16_rne(rm[i]); }
        }
        require_device();
        const int64_t zrows = t.zrows ? t.zrows : M;
        const size_t c_elems = (size_t)M * t.ldc, p_elems = (size_t)S * zrows * N, mod_elems = (size_t)M * std::max(t.ldmod, 1);
        Stage st;
        float *dC = st.out(c_elems), *dPart = st.out(p_elems), *dTail = st.out((size_t)M), *dXo = st.out(mk), *dYo = st.out(mk);
        GemmArgs g;
        g.A = st.in(t.x, (size_t)M * t.lda); g.amap = RowMap{t.lda, 0, 0};
        g.W = t.wfmt == 1 ? (const void*)st.in(rm16.data(), nk) : st.in(rm.data(), nk);
        g.w_bf16 = t.wfmt == 1; g.ldw = K; g.Wt = st.in(wt.data(), wt.size());
        if (t.wfmt == 2) { g.wt_i8 = 1; g.wscale = st.in(wscale.data(), (size_t)N); }
        g.bias = st.in(t.bias, (size_t)N);
        g.addvec = st.in(t.addvec, (size_t)(t.tail ? N - 1 : N));
        g.scale = st.in(t.scale, (size_t)N);
        if (t.gate) { g.gate = st.in(t.gate, (size_t)M * t.ldg); g.ldg = t.ldg; }
        g.C = dC; g.cmap = RowMap{t.ldc, 0, 0};
        if (t.R && t.r_in_c) {   // the in-place residual (R is C: every element read and written by the same lane)
            up(dC, t.R, c_elems * 4);
            g.R = dC;
        } else g.R = st.in(t.R, c_elems);
        g.alpha = t.alpha; g.epi = t.epi;
        if (t.tail) g.tail = dTail;
        if (t.zrows) g.zstride = zrows * N;
        g.M = M; g.N = N; g.K = K;
        SkinnyFuse fu;
        if (fused) {
            fu.ln = t.ln; fu.eps = t.eps;
            fu.ln_w = st.in(t.ln_w, (size_t)K); fu.ln_b = st.in(t.ln_b, (size_t)K);
            fu.shift = st.in(t.shift, mod_elems); fu.scale = st.in(t.mscale, mod_elems);
            fu.ldmod = t.ldmod;
            if (t.planes) fu.pend = PendingSum{st.in(t.planes, (size_t)t.psplit * mk), t.psplit, (int64_t)mk, st.in(t.pbias, (size_t)K)};
            if (t.pgate) { fu.pgate = dXo; fu.ldpg = 1; }   // (never launched: the step kernel takes no gated pending sum)
            fu.x_out = dXo; fu.y_out = dYo;
        }
        // refused before any launch: whatever the predicates of the kernel refuse
        if (t.path == 0) {
            if (!(fused ? skinny_fuse_supported(g, fu) : skinny_supported(g, S))) throw Error(PTTS_EINVAL, "ptts_debug_step_linear: not taken by the step kernel (skinny_supported / skinny_fuse_supported)");
        } else {
            GemmArgs c = g;
            c.M = std::min(M, 64);
            if (M > kSkinnyChunkRows || (M > 64 && t.tail) || !skinny_supported(c, 1)) throw Error(PTTS_EINVAL, "ptts_debug_step_linear: launch_gemm would not hand this product to the step kernel");
        }
        LaunchScope launches;
        launches.run([&] {
            if (t.path == 0) launch_skinny(g, fu, S, dPart, nullptr);
            else launch_gemm(g, nullptr);
        });
        PTTS_HIP(hipDeviceSynchronize());
        if (t.launches) { t.launches[0] = (int32_t)launches.count("k_skinny"); t.launches[1] = (int32_t)launches.total(); }
        down(t.C, S > 1 ? dPart : dC, (S > 1 ? p_elems : c_elems) * 4);
        if (t.tail_out) down(t.tail_out, dTail, (size_t)M * 4);
        if (t.x_out) down(t.x_out, dXo, mk * 4);
        if (t.y_out) down(t.y_out, dYo, mk * 4);
    });
}

// The opening and the closing of an AR step on host operands: ONE launcher call per op (include/ptts_debug.h).  None of these kernels bounds a load or a
// store by a buffer size -- the latent row at `step`, the noise row at `step` or `step + 1`, the rows of the two 32-deep linears -- so every counter is
// checked against the buffers allocated here before anything is uploaded.
int ptts_debug_step_edge(const ptts_step_edge_args* pa) {
    return guard([&] {
        const char* const me = "ptts_debug_step_edge";
        if (!pa) throw Error(PTTS_EINVAL, strfmt("%s: null argument", me));
        const ptts_step_edge_args& t = *pa;
        const int op = t.op;
        if (op < PTTS_STEP_EDGE_BEGIN || op > PTTS_STEP_EDGE_FIN_CHAIN) throw Error(PTTS_EINVAL, strfmt("%s: unknown op %d", me, op));
        const bool begin = op == PTTS_STEP_EDGE_BEGIN || op == PTTS_STEP_EDGE_BEGIN_LIN, fin = op == PTTS_STEP_EDGE_FIN || op == PTTS_STEP_EDGE_FIN_CHAIN;
        const bool chain = op == PTTS_STEP_EDGE_FIN_CHAIN, lins = op == PTTS_STEP_EDGE_BEGIN_LIN || chain;
        if (t.ldim < 4 || t.ldim > 64 || t.ldim % 4 != 0) throw Error(PTTS_EINVAL, strfmt("%s: ldim %d: a multiple of 4 up to 64", me, t.ldim));
        if (t.B < 1 || t.B > kStepMaxRows || t.rows < t.B || t.rows > 2 * kStepMaxRows) throw Error(PTTS_EINVAL, strfmt("%s: %d rows launched of %d held: 1..%d, held >= launched", me, t.B, t.rows, kStepMaxRows));
        if (t.S < 1 || t.S > 4096) throw Error(PTTS_EINVAL, strfmt("%s: %d frames per row outside 1..4096", me, t.S));
        const int B = t.B, rows = t.rows, ld = t.ldim;
        const int64_t need = (int64_t)t.S * ld;
        if (t.lat_stride < need || t.lat_stride > 4 * need + 64) throw Error(PTTS_EINVAL, strfmt("%s: lat_stride %lld below S ldim = %lld (or beyond 4 times that)", me, (long long)t.lat_stride, (long long)need));
        if (t.noise && (t.noise_stride < need || t.noise_stride > 4 * need + 64))
            throw Error(PTTS_EINVAL, strfmt("%s: noise_stride %lld below S ldim = %lld (or beyond 4 times that)", me, (long long)t.noise_stride, (long long)need));
        if (!t.kv_len || !t.active || !t.step || !t.countdown || !t.n_frames || !t.eos_step || !t.max_steps || !t.frames_after_eos || !t.broke || !t.n_active ||
            !t.eos_threshold || !t.latents || !t.bos || !t.in32 || !t.x0 || (!begin && !t.eos_logit) || (op == PTTS_STEP_EDGE_FINISH && !t.frame) ||
            (lins && (!t.w_in || !t.w_pj || !t.x || !t.fx)) || (fin && (!t.fx_in || !t.W || !t.shift || !t.mscale || !t.cur)))
            throw Error(PTTS_EINVAL, strfmt("%s: null operand", me));
        for (int r = 0; r < B; r++) {
            if (t.step[r] < 0 || t.step[r] > t.max_steps[r] || t.max_steps[r] > t.S)
                throw Error(PTTS_EINVAL, strfmt("%s: row %d: step %d, max_steps %d, %d frames held: 0 <= step <= max_steps <= S", me, r, t.step[r], t.max_steps[r], t.S));
            if (t.active[r] && t.step[r] >= t.max_steps[r]) throw Error(PTTS_EINVAL, strfmt("%s: row %d is active at step %d of %d", me, r, t.step[r], t.max_steps[r]));
        }
        if (lins && (t.d_in < 1 || t.d_in > 4096 || t.d_pj < 1 || t.d_pj > 4096 || (t.lin_bf16 != 0 && t.lin_bf16 != 1)))
            throw Error(PTTS_EINVAL, strfmt("%s: linears of %d and %d rows (1..4096 each), lin_bf16 %d", me, t.d_in, t.d_pj, t.lin_bf16));
        if (fin) {
            if (t.N != ld) throw Error(PTTS_EINVAL, strfmt("%s: N %d is not ldim %d (the frame is the whole row of C)", me, t.N, ld));
            if (t.K < 8 || t.K > 4096 || t.ldmod < t.K || t.ldmod > (1 << 16) || t.wfmt < 0 || t.wfmt > 2 || t.epi < EPI_NONE || t.epi > EPI_RESADD_ELU)
                throw Error(PTTS_EINVAL, strfmt("%s: K %d, ldmod %d, wfmt %d, epi %d do not fit", me, t.K, t.ldmod, t.wfmt, t.epi));
            if (chain && (t.lat_stride % 2 != 0 || t.lin_bf16 != (t.wfmt != 0 ? 1 : 0)))
                throw Error(PTTS_EINVAL, strfmt("%s: chained: lat_stride %lld must be even, the 32-deep linears bf16 exactly when the step weights are not f32", me, (long long)t.lat_stride));
        }
        const int N = t.N, K = t.K, d_in = lins ? t.d_in : 0, d_pj = lins ? t.d_pj : 0;
        const size_t nk = fin ? (size_t)N * K : 0, les = t.lin_bf16 ? 2 : 4;
        // the final linear: the loader's packers
        std::vector<float> rm, wscale;
        std::vector<uint8_t> wt;
        std::vector<uint16_t> rm16;
        if (fin) {
            rm.assign(t.W, t.W + nk);
            wt.resize(step_tiled_bytes((size_t)N, (size_t)K, t.wfmt == 2 ? 1 : (t.wfmt == 1 ? 2 : 4)));
            if (t.wfmt == 2) {
                std::vector<int8_t> q;
                quantize_rows(rm, (size_t)N, (size_t)K, wscale, q);   // rm -> W^
                pack_step_tiled_i8(q.data(), (size_t)N, (size_t)K, wt.data());
                if (t.w_eff) std::memcpy(t.w_eff, rm.data(), nk * 4);
                if (t.w_scale) std::memcpy(t.w_scale, wscale.data(), (size_t)N * 4);
            } else {
                pack_step_tiled(rm.data(), (size_t)N, (size_t)K, t.wfmt == 1, wt.data());
                if (t.wfmt == 1) { rm16.resize(nk); for (size_t i = 0; i < nk; i++) rm16[i] = f32_to_bf16_rne(rm[i]); }
            }
        }
        require_device();
        Stage st;
        const size_t R = (size_t)rows;
        // the state as the batch set-up lays it out: nine int32 arrays and n_active in one allocation, the thresholds in another
        std::vector<int32_t> hs(9 * R + 1);
        int32_t* const harr[9] = {t.kv_len, t.active, t.step, t.countdown, t.n_frames, t.eos_step, t.max_steps, t.frames_after_eos, t.broke};
        for (int i = 0; i < 9; i++) std::memcpy(hs.data() + (size_t)i * R, harr[i], R * 4);
        hs[9 * R] = t.n_active[0];
        int32_t* const ds = st.out<int32_t>(hs.size());
        up(ds, hs.data(), hs.size() * 4);
        float* const dthr = st.out(R);
        up(dthr, t.eos_threshold, R * 4);
        StepState s;
        s.kv_len = ds; s.active = ds + R; s.step = ds + 2 * R; s.countdown = ds + 3 * R; s.n_frames = ds + 4 * R; s.eos_step = ds + 5 * R;
        s.max_steps = ds + 6 * R; s.frames_after_eos = ds + 7 * R; s.broke = ds + 8 * R; s.n_active = ds + 9 * R; s.eos_threshold = dthr;
        float* const dLat = st.out(R * (size_t)t.lat_stride);
        up(dLat, t.latents, R * (size_t)t.lat_stride * 4);
        const float* const dNoise = st.in(t.noise, R * (size_t)t.noise_stride);
        const float* const dBos = st.in(t.bos, (size_t)ld);
        const float* const dLogit = st.in(t.eos_logit, R);
        float *dIn32 = st.out(R * ld), *dX0 = st.out(R * ld), *dX = st.out(R * (size_t)d_in), *dFx = st.out(R * (size_t)d_pj);
        StepOpenLinears lin;
        if (lins) {
            lin.w_in = st.in_bytes(t.w_in, (size_t)d_in * ld * les); lin.b_in = st.in(t.b_in, (size_t)d_in); lin.d_in = d_in; lin.x = dX;
            lin.w_pj = st.in_bytes(t.w_pj, (size_t)d_pj * ld * les); lin.b_pj = st.in(t.b_pj, (size_t)d_pj); lin.d_pj = d_pj; lin.fx = dFx;
            lin.w_bf16 = t.lin_bf16;
        }
        if (chain && !step_open_mfma_ok(lin, ld)) throw Error(PTTS_EINVAL, strfmt("%s: chained: the 32-deep linears are not taken by the matrix-core opening (step_open_mfma_ok)", me));
        const float* dFrame = op == PTTS_STEP_EDGE_FINISH ? st.in(t.frame, R * ld) : nullptr;
        GemmArgs g;
        SkinnyFuse fu;
        float* dCur = nullptr;
        if (fin) {
            dCur = st.out(R * N);
            up(dCur, t.cur, R * N * 4);
            g.A = st.in(t.fx_in, R * K); g.amap = RowMap{K, 0, 0};
            g.W = t.wfmt == 1 ? (const void*)st.in(rm16.data(), nk) : st.in(rm.data(), nk);
            g.w_bf16 = t.wfmt == 1; g.ldw = K; g.Wt = st.in(wt.data(), wt.size());
            if (t.wfmt == 2) { g.wt_i8 = 1; g.wscale = st.in(wscale.data(), (size_t)N); }
            g.bias = st.in(t.bias, (size_t)N);
            g.C = dCur; g.cmap = RowMap{N, 0, 0}; g.R = dCur;   // step_flow: current += flow / steps, in place
            g.alpha = t.alpha; g.epi = t.epi;
            g.M = B; g.N = N; g.K = K;
            // the record in device memory, as the batch set-up fills it: a chained step opens the next one in the OTHER copies of fx / cur
            StepFinish sf{s, dLogit, dLat, t.lat_stride, (int32_t)ld, StepChain{}};
            if (chain) sf.ch = StepChain{lin.w_in, lin.b_in, lin.x, lin.d_in, lin.w_pj, lin.b_pj, dFx, lin.d_pj, dBos, dX0, lin.w_bf16, 1};
            fu.ln = 1; fu.eps = t.eps;   // flowFinalLayer: LayerNorm without affine, then the modulation
            fu.shift = st.in(t.shift, R * (size_t)t.ldmod); fu.scale = st.in(t.mscale, R * (size_t)t.ldmod); fu.ldmod = t.ldmod;
            fu.fin = st.in(&sf, 1);
            if (chain) { fu.chain = 1; fu.chain_noise = dNoise; fu.chain_noise_stride = dNoise ? t.noise_stride : need; }
            if (!skinny_fuse_supported(g, fu)) throw Error(PTTS_EINVAL, strfmt("%s: not taken by the step kernel (skinny_fuse_supported)", me));
        }
        LaunchScope launches;
        launches.run([&] {
            if (begin) launch_step_begin(s, dLat, t.lat_stride, dBos, dNoise, dNoise ? t.noise_stride : need, ld, B, dIn32, dX0, lins ? &lin : nullptr, nullptr);
            else if (op == PTTS_STEP_EDGE_FINISH) launch_step_finish(s, dFrame, dLogit, ld, B, dLat, t.lat_stride, nullptr);
            else launch_skinny(g, fu, 1, nullptr, nullptr);
        });
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        put_str(t.launched, t.launched_cap, launches.str());
        down(hs.data(), ds, hs.size() * 4);
        for (int i = 0; i < 9; i++) std::memcpy(harr[i], hs.data() + (size_t)i * R, R * 4);
        t.n_active[0] = hs[9 * R];
        down(t.eos_threshold, dthr, R * 4);
        down(t.latents, dLat, R * (size_t)t.lat_stride * 4);
        down(t.in32, dIn32, R * ld * 4); down(t.x0, dX0, R * ld * 4);
        if (t.x) down(t.x, dX, R * (size_t)d_in * 4);
        if (t.fx) down(t.fx, dFx, R * (size_t)d_pj * 4);
        if (fin) down(t.cur, dCur, R * N * 4);
    });
}

// The step attention on host operands: ONE launch_attention call with the AttnArgs of the AR step, from the function step.cpp step_core builds them with (launch_args.h attn_step_args).  k_attn_step bounds none of its
// loads by a buffer size -- cache rows up to seg_len, prefix rows up to pre_len, the RoPE row at seg_len -- so every one of those is checked against the
// buffers allocated here before anything is uploaded; there is no way to ask for a launch without the checks.
int ptts_debug_attn_step(const ptts_attn_step_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_attn_step: null argument");
        const ptts_attn_step_args& t = *pa;
        if (!t.qkv || !t.cos_t || !t.sin_t || !t.seg_len || !t.active || !t.pre_len || !t.voice_of_row || !t.k || !t.v || !t.out || (t.kv_bf16 != 0 && t.kv_bf16 != 1) ||
            t.rows < 1 || t.rows > 1024 || t.heads < 1 || t.heads > 64 || t.cap < 1 || t.cap > 4096 || t.layers < 1 || t.layers > 64 || t.keys_now < 0 || t.n_pre < 0 ||
            t.n_pre > 4)
            throw Error(PTTS_EINVAL, "ptts_debug_attn_step: bad arguments");
        const int rows = t.rows, heads = t.heads, cap = t.cap, D = heads * 64, es = t.kv_bf16 ? 2 : 4;
        if (t.layer < 0 || t.layer >= t.layers) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: layer %d of %d", t.layer, t.layers));
        if (t.qkv_ld < 3 * (int64_t)D || t.out_ld < D) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: qkv_ld %lld / out_ld %lld below 3 d_model / d_model (%d)", (long long)t.qkv_ld, (long long)t.out_ld, D));
        for (int i = 0; i < t.n_pre; i++)
            if (!t.pre_k[i] || !t.pre_v[i] || t.pre_rows[i] < 1 || t.pre_rows[i] > cap) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: prefix buffer %d is null, empty or longer than the cache", i));
        for (int r = 0; r < rows; r++) {
            const int pos = t.seg_len[r], pre = t.pre_len[r], vo = t.voice_of_row[r];
            if (pos < 0 || pos >= cap) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: row %d at offset %d, the cache holds %d", r, pos, cap));
            if (vo < -1 || vo >= t.n_pre) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: row %d names prefix buffer %d of %d", r, vo, t.n_pre));
            if (pre < 0 || pre > pos) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: row %d: prefix of %d keys at offset %d", r, pre, pos));
            if (pre != 0 && (vo < 0 || pre != t.pre_rows[vo])) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: row %d: prefix of %d keys is not the length of the buffer it names", r, pre));
            if (t.keys_now > 0 && t.active[r] && pos + 1 > t.keys_now) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_step: row %d at offset %d is beyond keys_now %d", r, pos, t.keys_now));
        }
        require_device();
        const size_t tab = (size_t)cap * 32, out_elems = (size_t)rows * t.out_ld, kv_bytes = (size_t)rows * heads * cap * 64 * es;
        Stage st;
        std::vector<const void*> pre;   // [2 i]: keys of buffer i, [2 i + 1]: values
        for (int i = 0; i < t.n_pre; i++) {
            const size_t n = (size_t)t.layers * heads * t.pre_rows[i] * 64 * es;
            pre.push_back(st.in_bytes(t.pre_k[i], n));
            pre.push_back(st.in_bytes(t.pre_v[i], n));
        }
        std::vector<const void*> hk((size_t)rows, nullptr), hv((size_t)rows, nullptr);
        for (int r = 0; r < rows; r++)
            if (t.voice_of_row[r] >= 0) { hk[(size_t)r] = pre[(size_t)2 * t.voice_of_row[r]]; hv[(size_t)r] = pre[(size_t)2 * t.voice_of_row[r] + 1]; }
        void *dK = st.in_bytes(t.k, kv_bytes), *dV = st.in_bytes(t.v, kv_bytes);
        float* dO = st.out(out_elems);
        const StepAttnRows ar{st.in(t.qkv, (size_t)rows * t.qkv_ld), t.qkv_ld, D, st.in(t.cos_t, tab), st.in(t.sin_t, tab), st.in(t.seg_len, (size_t)rows),
                              st.in(t.active, (size_t)rows), st.in(hk.data(), (size_t)rows), st.in(hv.data(), (size_t)rows), st.in(t.pre_len, (size_t)rows), rows};
        const AttnArgs a = attn_step_args(KvLayer{dK, dV, t.kv_bf16, heads, cap, 64}, ar, t.layer, t.keys_now, dO, t.out_ld);   // step_core's launch form
        LaunchScope launches;
        launches.run([&] { launch_attention(a, nullptr); });
        PTTS_HIP(hipDeviceSynchronize());
        const bool step = std::string(g_last_attn_kernel) == "k_attn_step";
        put_str(t.kernel, t.kernel_cap, g_last_attn_kernel);
        if (t.info) {
            t.info[0] = step ? attn_step_launch_rounds(a) : 0;
            t.info[1] = (int32_t)launches.total(); t.info[2] = (int32_t)launches.count("k_attn_step"); t.info[3] = (int32_t)launches.count("k_attention");
        }
        down(t.out, dO, out_elems * 4); down(t.k, dK, kv_bytes); down(t.v, dV, kv_bytes);
    });
}

int ptts_debug_attn_step_rounds(int32_t keys, int32_t kv_bf16, int32_t* keys_per_round) {
    if (keys_per_round) *keys_per_round = attn_step_keys_per_round(kv_bf16 != 0);
    return attn_step_rounds(keys, kv_bf16 != 0);
}

// The window attention on host operands: ONE launch with the AttnArgs of mimi_range / the encoder (dense) or of the prompt prefill (ragged), from the functions those build them with (launch_args.h).  The kernels
// bound their key loads by positions alone (pos_base + rows, rag_pos0 + segment length), never by a buffer size, so those are checked against the buffers
// allocated here before anything is uploaded.
int ptts_debug_attn_window(const ptts_attn_window_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: null argument");
        const ptts_attn_window_args& t = *pa;
        if (!t.qkv || !t.out || (t.kv_bf16 != 0 && t.kv_bf16 != 1) || (t.ragged != 0 && t.ragged != 1)) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: bad arguments");
        if (t.form < 0 || t.form > 2) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: unknown form %d", t.form));
        if (t.heads < 1 || t.heads > 16 || t.segs < 1 || t.segs > 16)
            throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: %d heads, %d segments: the hook takes 1..16 of each", t.heads, t.segs));
        const int heads = t.heads, segs = t.segs, D = heads * 64, es = t.kv_bf16 ? 2 : 4;
        if (t.ld < (t.ragged ? 1 : 3) * (int64_t)D || t.out_ld < D)
            throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: ld %lld / out_ld %lld below the columns the launch reads / writes (d_model %d)", (long long)t.ld, (long long)t.out_ld, D));
        if (t.ld > (1 << 16) || t.out_ld > (1 << 16)) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: ld / out_ld above 65536");
        if (t.ld % 4 || t.out_ld % 4)
            throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: ld %lld / out_ld %lld: rows must keep 16-byte alignment (attn_window_supported)", (long long)t.ld, (long long)t.out_ld));
        int rows = 0;
        RaggedMeta meta;
        if (t.ragged) {
            if (!t.k || !t.v || !t.rag_off || !t.rag_pos0) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: ragged operands need k, v, rag_off and rag_pos0");
            if (t.form == 2) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: form 2 (k_attn_window_lds) takes dense operands only");
            if (t.cap < 1 || t.cap > 4096 || t.rows < 1 || t.rows > 4096) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: cap %d / rows %d outside 1..4096", t.cap, t.rows));
            if (t.rag_off[0] != 0 || t.rag_off[segs] != t.rows) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: rag_off runs from %d to %d, not from 0 to rows %d", t.rag_off[0], t.rag_off[segs], t.rows));
            rows = t.rows;
            for (int s = 0; s < segs; s++) {
                const int n = t.rag_off[s + 1] - t.rag_off[s];
                if (n < 0) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: rag_off decreases at segment %d", s));
                if (t.rag_pos0[s] < 0 || t.rag_pos0[s] + n > t.cap) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: segment %d: %d rows from position %d, the cache holds %d", s, n, t.rag_pos0[s], t.cap));
            }
            meta = ragged_meta(t.rag_off, t.rag_pos0, segs);   // batch_prompt's one-upload table
        } else {
            if (t.kv_bf16) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: the dense layout is f32 (attn_window_supported)");
            if (t.T1 < 1 || t.T1 > 4096) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: T1 %d outside 1..4096", t.T1));
            if (t.t0 < 0 || t.CT < 1 || (int64_t)t.t0 + t.CT > t.T1) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: chunk (%d, %d) leaves the %d rows of a segment", t.t0, t.CT, t.T1));
            if ((int64_t)segs * t.CT > 4096) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: %d rows, the hook takes 4096", segs * t.CT));
            if (t.context < 1) throw Error(PTTS_EINVAL, strfmt("ptts_debug_attn_window: the dense launch needs a window (context %d; attn_window_supported)", t.context));
            rows = segs * t.CT;
        }
        require_device();
        const size_t q_elems = (t.ragged ? (size_t)rows : (size_t)segs * t.T1) * t.ld, kv_bytes = (size_t)segs * heads * t.cap * 64 * es, out_elems = (size_t)rows * t.out_ld,
                     meta_bytes = std::max<size_t>(meta.table.size(), 1) * 4;
        Stage st;
        Tmp dMeta(meta_bytes);
        float *dQ = st.in(t.qkv, q_elems), *dO = st.out(out_elems);
        // the engine's own launch forms: batch_prompt's (ragged), mimi_range's (dense; encoder.cpp: t0 = 0, CT = T1, one segment)
        const AttnArgs a = t.ragged ? attn_ragged_args(KvLayer{st.in_bytes(t.k, kv_bytes), st.in_bytes(t.v, kv_bytes), t.kv_bf16, heads, t.cap, 64}, meta, dMeta.as<int32_t>(), dQ,
                                                       t.ld, t.context, dO, t.out_ld)
                                    : attn_dense_args(dQ, t.ld, D, segs, t.T1, t.t0, t.CT, heads, 64, t.context, dO, t.out_ld);
        if (!attn_window_supported(a) || (t.form && !attn_window_form_supported(a, t.form))) throw Error(PTTS_EINVAL, "ptts_debug_attn_window: refused by attn_window_supported");
        if (t.ragged) up(dMeta.p, meta.table.data(), meta.table.size() * 4);
        LaunchScope launches;
        launches.run([&] {
            if (t.form == 0) launch_attention(a, nullptr);
            else launch_attn_window_as(a, t.form, nullptr);
        });
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        put_str(t.kernel, t.kernel_cap,
                t.form == 0 ? g_last_attn_kernel
                : t.form == 2 ? "k_attn_window_lds<4>"
                : !t.ragged ? "k_attn_window<false,false>" : (t.kv_bf16 ? "k_attn_window<true,true>" : "k_attn_window<false,true>"));
        put_str(t.launched, t.launched_cap, launches.str());
        down(t.out, dO, out_elems * 4);
    });
}

// The many-row GEMMs on host operands: ONE launch of a named kernel.  These kernels clamp addresses instead of bounding their loads, so every element a row's
// read or store can touch is checked against the caller's buffer sizes here, before anything is uploaded.
int ptts_debug_gemm_rows(const ptts_gemm_rows_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: null argument");
        const ptts_gemm_rows_args& t = *pa;
        if (!t.A || !t.W || !t.C || t.M <= 0 || t.N <= 0 || t.K <= 0 || t.ldw < t.K || t.a_elems <= 0 || t.c_elems <= 0 || t.epi < EPI_NONE || t.epi > EPI_RESADD_ELU ||
            (t.aop != AOP_NONE && t.aop != AOP_ELU) || (t.w_bf16 != 0 && t.w_bf16 != 1) || t.a_ld < 1 || t.c_ld < 1 || t.a_rows_per_batch < 0 || t.c_rows_per_batch < 0 ||
            t.a_rows_per_batch > INT32_MAX || t.c_rows_per_batch > INT32_MAX || t.a_batch_stride < 0 || t.c_batch_stride < 0 || t.a_off < 0 || t.c_off < 0 || t.kslice < 0 ||
            t.zstride < 0 || t.win_taps < 0 || t.win_c < 0)
            throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: bad arguments");
        if (t.kernel < 0 || t.kernel > 5) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: unknown kernel");
        if ((t.epi >= EPI_RESADD && !t.R) || (t.epi == EPI_GATE_RESADD && (!t.gate || t.ldg < t.N)))
            throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: operands do not fit the epilogue asked for");
        const int M = t.M, N = t.N, K = t.K;
        const bool rope = t.rope_cos || t.rope_sin;
        if (rope && (!t.rope_cos || !t.rope_sin || t.n_pos < 1 || t.rope_hd < 4 || t.rope_hd % 4 || t.rope_cols < 0 || t.rope_cols > N || t.rope_pos0 < 0 || t.rope_rows_per_seg < 0))
            throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: bad RoPE arguments");
        const int planes = t.kslice ? (K + t.kslice - 1) / t.kslice : 1;
        // what would be ignored in silence: an rgl on another kernel than k_gemm_wres, a cfg on another than k_gemm3 / k_gemm5, a zstride without slices
        if (t.cfg && t.kernel != 3 && t.kernel != 5) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: cfg is k_gemm3's and k_gemm5's alone");
        if (t.rgl && t.kernel != 4) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: rgl is k_gemm_wres' alone");
        if (t.zstride && !t.kslice) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: zstride without kslice");
        // C's rows, segments and planes must not overlap: two blocks would store to one element (A's rows may: a convolution's windows)
        const int64_t c_seg = t.c_rows_per_batch ? (std::min<int64_t>(M, t.c_rows_per_batch) - 1) * t.c_ld + N : 0;   // one segment's extent
        const int64_t c_plane = t.c_rows_per_batch ? ((M - 1) / t.c_rows_per_batch) * t.c_batch_stride + ((M - 1) % t.c_rows_per_batch) * t.c_ld + N : (int64_t)(M - 1) * t.c_ld + N;
        if (t.c_ld < N || (t.c_rows_per_batch && M > t.c_rows_per_batch && t.c_batch_stride < c_seg) || (planes > 1 && t.zstride < c_plane))
            throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: rows, segments or planes of C overlap");
        // the maps against the buffers: the largest element any row's K-wide read (a clamped row is row M - 1) and N-wide store / residual read can touch
        const RowMap amap{t.a_ld, t.a_rows_per_batch, t.a_batch_stride}, cmap{t.c_ld, t.c_rows_per_batch, t.c_batch_stride};
        check_rows("ptts_debug_gemm_rows", "A", M, t.a_elems, amap, t.a_off, K, false);
        check_rows("ptts_debug_gemm_rows", "C", M, t.c_elems, cmap, t.c_off + (int64_t)(planes - 1) * t.zstride, N, false);   // (the last plane's rows)
        if (rope)
            for (int64_t m = 0; m < M; m++) {
                const int64_t pos = t.rope_row_pos ? t.rope_row_pos[m] : (int64_t)t.rope_pos0 + (t.rope_rows_per_seg ? m % t.rope_rows_per_seg : m);
                if (pos < 0 || pos >= t.n_pos) throw Error(PTTS_EINVAL, strfmt("ptts_debug_gemm_rows: row %lld at position %lld, the tables hold %d", (long long)m, (long long)pos, t.n_pos));
            }
        require_device();
        int dev = 0, cus = 0;
        PTTS_HIP(hipGetDevice(&dev));
        PTTS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const size_t nw = (size_t)N * t.ldw, half = (size_t)(rope ? t.rope_hd / 2 : 0), ntab = (size_t)std::max(t.n_pos, 1) * std::max<size_t>(half, 1);
        Stage st;
        float* dC = st.out((size_t)t.c_elems);
        GemmArgs g;
        g.A = st.in(t.A, (size_t)t.a_elems) + t.a_off; g.amap = amap;
        if (t.w_bf16) {
            std::vector<uint16_t> w16(nw);
            for (size_t i = 0; i < nw; i++) w16[i] = f32_to_bf16_rne(t.W[i]);
            g.W = st.in(w16.data(), nw);
        } else g.W = st.in(t.W, nw);
        g.w_bf16 = t.w_bf16; g.ldw = t.ldw;
        g.C = dC + t.c_off; g.cmap = cmap;
        g.bias = st.in(t.bias, (size_t)N); g.addvec = st.in(t.addvec, (size_t)N); g.scale = st.in(t.scale, (size_t)N);
        if (t.gate) { g.gate = st.in(t.gate, (size_t)M * t.ldg); g.ldg = t.ldg; }
        if (t.R) {   // r_in_c: the in-place residual (R is C: every element read and written by the same lane)
            if (t.r_in_c) up(dC, t.R, (size_t)t.c_elems * 4);
            g.R = (t.r_in_c ? dC : st.in(t.R, (size_t)t.c_elems)) + t.c_off;
        }
        if (rope) {
            g.rope_cos = st.in(t.rope_cos, ntab); g.rope_sin = st.in(t.rope_sin, ntab); g.rope_cols = t.rope_cols; g.rope_hd = t.rope_hd; g.rope_pos0 = t.rope_pos0;
            g.rope_rows_per_seg = t.rope_rows_per_seg;
            g.rope_row_pos = st.in(t.rope_row_pos, (size_t)M);
        }
        g.kslice = t.kslice; g.zstride = t.zstride; g.win_taps = t.win_taps; g.win_c = t.win_c;
        g.alpha = t.alpha; g.aop = t.aop; g.epi = t.epi; g.M = M; g.N = N; g.K = K;
        // refused before any launch: what the kernel's own predicate refuses, and a forced form its production guard would not allow
        const bool extra = rope || t.kslice;   // what only k_gemm3 / k_gemm5 implement: another kernel would ignore it in silence
        int rgl = 0;
        switch (t.kernel) {
            case 0:
                if (extra && !gemm5_supported(g) && !gemm3_supported(g)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: no kernel with RoPE / split-K takes this shape");
                if (!extra && gemm_wres_supported(g)) rgl = gemm_wres_rgl(g);
                break;
            case 1:
                if (extra || gemm_wres_supported(g) || gemm5_supported(g) || gemm3_supported(g) || gemm2_supported(g))
                    throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: launch_gemm does not leave this shape to k_gemm");
                break;
            case 2:
                if (extra || !gemm2_supported(g)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: refused by gemm2_supported");
                break;
            case 3:
                if (!gemm3_supported(g)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: refused by gemm3_supported");
                if (!(t.cfg >= 0 && t.cfg <= 4) && t.cfg != 6) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: unknown k_gemm3 cfg");
                if (t.cfg == 4 && N < 256) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: k_gemm3<256,8,64> needs N >= 256");
                break;
            case 4: {
                if (!gemm_wres_supported(g)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: refused by gemm_wres_supported");
                rgl = t.rgl ? t.rgl : gemm_wres_rgl(g);
                if (rgl < 1 || rgl > gemm_wres_max_rgl(g)) throw Error(PTTS_EINVAL, strfmt("ptts_debug_gemm_rows: rgl %d outside [1, %d]", rgl, gemm_wres_max_rgl(g)));
                break;
            }
            default:
                if (!gemm5_supported(g)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: refused by gemm5_supported");
                if (t.cfg < 0 || t.cfg > 4) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: unknown k_gemm5 cfg");
                if ((t.cfg == 1 || t.cfg == 2) && N % 256) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: a 256-column k_gemm5 form needs N % 256 == 0 (its weight loads are not bounded)");
                break;
        }
        LaunchScope launches;
        launches.run([&] {
            switch (t.kernel) {
                case 0:
                    if (rope) { if (!launch_gemm_rope(g, nullptr)) throw Error(PTTS_EINVAL, "ptts_debug_gemm_rows: no RoPE epilogue for this shape"); }
                    else launch_gemm(g, nullptr);
                    break;
                case 1: launch_gemm(g, nullptr); break;
                case 2: launch_gemm2(g, nullptr); break;
                case 3: { Scoped<int> cfg(g_gemm3_cfg, t.cfg); launch_gemm3(g, nullptr); break; }
                case 4: launch_gemm_wres_as(g, rgl, nullptr); break;
                default: { Scoped<int> cfg(g_gemm5_cfg, t.cfg); launch_gemm5(g, nullptr); break; }
            }
        });
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        put_str(t.launched, t.launched_cap, launches.str());
        if (t.info) { t.info[0] = cus; t.info[1] = rgl; }
        down(t.C, dC, (size_t)t.c_elems * 4);
    });
}

// ---- the fused SEANet blocks (csrc/resblock.hip, csrc/resblock_up.hip) stand-alone ----
// the launch form resblock_plan / resblock_up_plan choose (no GPU: `cus` is an argument)
int ptts_debug_resblock_plan(int32_t C, int32_t final_conv, int32_t w_bf16, int32_t fuse_up, int32_t B, int32_t rows, int32_t form, int32_t grid, int32_t cus, int32_t* out) {
    return guard([&] {
        if (!out || B < 1 || rows < 1 || cus < 1 || form < RES_FORM_AUTO || form > RES_FORM_PERS) throw Error(PTTS_EINVAL, "ptts_debug_resblock_plan: bad arguments");
        const ResPlan p = fuse_up ? resblock_up_plan(B, rows, form, grid, cus) : resblock_plan(C, final_conv, w_bf16, B, rows, form, grid, cus);
        out[0] = p.nw; out[1] = p.pers; out[2] = p.grid; out[3] = p.tiles; out[4] = p.tout;
    });
}

// the loader's packers on a caller's matrix (no GPU)
int ptts_debug_seanet_pack(int32_t kind, const float* rm, int32_t out, int32_t in, uint16_t* hi, uint16_t* lo) {
    return guard([&] {
        if (!rm || !hi || in < 32 || in % 32 || (kind != 2 && (out < 16 || out % 16)) || kind < 0 || kind > 2 || (kind == 2 && !lo))
            throw Error(PTTS_EINVAL, "ptts_debug_seanet_pack: bad arguments");
        if (kind == 0) pack_frag16(rm, (size_t)out, (size_t)in, hi, lo);
        else if (kind == 1) {
            if (out != 256) throw Error(PTTS_EINVAL, "ptts_debug_seanet_pack: the fused transposed convolution has 4 x 64 rows");
            std::vector<float> rg((size_t)out * in);
            regroup_convtr_rows(rm, out, in, out / 4, rg.data());
            pack_frag16(rg.data(), (size_t)out, (size_t)in, hi, lo);
        } else pack_final_frag(rm, (size_t)in, hi, lo);
    });
}

// what the loader itself packed (no GPU): the plan's arena is filled on the host and the item's planes are copied out
int ptts_debug_plan_seanet_frags(ptts_plan* hp, int32_t item, uint16_t* hi, uint16_t* lo, int64_t cap, int64_t* count, int32_t* dims) {
    return guard([&] {
        if (!hp || !count || !dims || item < 0 || item > 7) throw Error(PTTS_EINVAL, "ptts_debug_plan_seanet_frags: bad arguments");
        const Desc& d = hp->p.desc;
        size_t wf = NONE, wl = NONE, n = 0;
        if (item < 7) {
            const Lin& l = item < 3 ? d.rb1[item] : (item < 6 ? d.rb2[item - 3] : d.up[2]);
            wf = l.wf; wl = l.wf_lo; dims[0] = l.out; dims[1] = l.in;
            if (wf != NONE) n = frag16_count((size_t)l.out, (size_t)l.in);
        } else {
            wf = d.final_wf; wl = d.final_wf_lo; dims[0] = 1; dims[1] = d.final_k * d.sea_ch[3];
            if (wf != NONE) n = frag16_count(16, (size_t)dims[1]);
        }
        dims[2] = wl != NONE;
        *count = (int64_t)n;
        if (!n || !hi) return;
        if ((int64_t)n > cap || (wl != NONE && !lo)) throw Error(PTTS_EINVAL, "ptts_debug_plan_seanet_frags: buffers too small");
        std::vector<uint8_t> host(d.total_bytes);
        plan_fill(hp->p, host.data());
        std::memcpy(hi, host.data() + wf, n * 2);
        if (wl != NONE) std::memcpy(lo, host.data() + wl, n * 2);
    });
}

// ONE launch of k_resblock / k_resblock_up on host operands.  The slack rows of u and xin are NaN.  The weights go through the loader's own packers (model.h).
int ptts_debug_resblock(const ptts_resblock_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_resblock: null argument");
        const ptts_resblock_args& t = *pa;
        const bool fin = t.final_conv != 0, up_ = t.fuse_up != 0, bf = t.w_bf16 != 0;
        if (t.B < 1 || t.B > 64 || t.L < 1 || t.L > (1 << 16) || t.t0 < 0 || t.t1 <= t.t0 || t.t1 > t.L || t.pad < 0 || t.pad > 64 || t.slack < 0 || t.slack > 64 ||
            t.form < RES_FORM_AUTO || t.form > RES_FORM_PERS || !t.w1 || !t.w2 || (!up_ && !t.u) || (fin ? (!t.wf || !t.pcm) : !t.uo))
            throw Error(PTTS_EINVAL, "ptts_debug_resblock: bad arguments");
        if (!((t.C == 64 && t.H == 32) || (t.C == 128 && t.H == 64))) throw Error(PTTS_EINVAL, "ptts_debug_resblock: unsupported widths (C / H is 64 / 32 or 128 / 64)");
        if (t.pad < 2) throw Error(PTTS_EINVAL, "ptts_debug_resblock: pad < 2 (the kernel reads two rows of history)");
        if (t.rows) {
            if (!fin) throw Error(PTTS_EINVAL, "ptts_debug_resblock: row destinations need the final convolution");
            if (t.t0 % 4) throw Error(PTTS_EINVAL, "ptts_debug_resblock: t0 % 4 != 0 with row destinations");
            if (!t.row_out || t.row_bytes % 16 || t.row_bytes < (int64_t)t.L * 4) throw Error(PTTS_EINVAL, "ptts_debug_resblock: row_bytes must be a multiple of 16 and hold L f32 samples");
            for (int b = 0; b < t.B; b++) if (t.rows[2 * b] < 0) throw Error(PTTS_EINVAL, "ptts_debug_resblock: negative lim");
        }
        if (up_) {
            if (!bf) throw Error(PTTS_EINVAL, "ptts_debug_resblock: f32 weights with the fused form (its weights live in registers and LDS as bf16)");
            if (t.C != 64 || !fin) throw Error(PTTS_EINVAL, "ptts_debug_resblock: the fused form is the 64-wide block with the final convolution");
            if (!t.xin || !t.wup || t.x_pad < 1 || t.x_pad > 64 || t.x_slack < 0 || t.x_slack > 64 || t.x_L < 1) throw Error(PTTS_EINVAL, "ptts_debug_resblock: bad arguments of the fused form");
            if ((int64_t)t.x_L * 4 != t.L) throw Error(PTTS_EINVAL, "ptts_debug_resblock: x_L * 4 != L");
            if (t.t0 % 4) throw Error(PTTS_EINVAL, "ptts_debug_resblock: t0 % 4 != 0 with the fused form");
            if (t.form == RES_FORM_TILE) throw Error(PTTS_EINVAL, "ptts_debug_resblock: the fused form is persistent only");
        }
        // the launch form: the production choice, or the caller's
        ResPlan plan;
        if (t.form == RES_FORM_AUTO) {
            require_device();
            plan = up_ ? resblock_up_plan(t.B, t.t1 - t.t0, RES_FORM_AUTO, 0, resblock_cus()) : resblock_plan(t.C, fin, bf, t.B, t.t1 - t.t0, RES_FORM_AUTO, 0, resblock_cus());
            if (plan.grid == 0) throw Error(PTTS_EINVAL, "ptts_debug_resblock: the fused form is not taken at this size (resblock_up_supported's threshold); ask for form 2 with a grid");
        } else {
            plan = up_ ? resblock_up_plan(t.B, t.t1 - t.t0, t.form, t.grid, 1) : resblock_plan(t.C, fin, bf, t.B, t.t1 - t.t0, t.form, t.grid, 1);
            if (plan.nw == 0) throw Error(PTTS_EINVAL, "ptts_debug_resblock: no persistent form of this block (bf16 weights; 64-wide with the final convolution, 128-wide without)");
        }
        const int64_t total = (int64_t)t.B * plan.tiles;
        if (plan.pers && (plan.grid < 1 || plan.grid > total))
            throw Error(PTTS_EINVAL, strfmt("ptts_debug_resblock: grid %d outside [1, B * tiles = %lld]: a block's first tile would lie past the last utterance", plan.grid, (long long)total));
        if (!plan.pers && plan.grid != total) throw Error(PTTS_EINVAL, "ptts_debug_resblock: one block per tile");

        // weights: the loader's packers
        const int C = t.C, H = t.H, B = t.B, L = t.L;
        const size_t n1 = frag16_count((size_t)H, (size_t)3 * C), n2 = frag16_count((size_t)C, (size_t)H), nf = frag16_count(16, (size_t)3 * C), nu = frag16_count(256, 256);
        std::vector<uint16_t> w1h(n1), w1l(n1), w2h(n2), w2l(n2), wfh(nf), wfl(nf), wuh(nu);
        pack_frag16(t.w1, (size_t)H, (size_t)3 * C, w1h.data(), bf ? nullptr : w1l.data());
        pack_frag16(t.w2, (size_t)C, (size_t)H, w2h.data(), bf ? nullptr : w2l.data());
        if (fin) pack_final_frag(t.wf, (size_t)3 * C, wfh.data(), wfl.data());
        if (up_) {
            std::vector<float> rg((size_t)256 * 256);
            regroup_convtr_rows(t.wup, 256, 256, 64, rg.data());
            pack_frag16(rg.data(), 256, 256, wuh.data(), nullptr);
        }
        require_device();
        const int64_t urows = (int64_t)t.pad + L + t.slack, u_bs = urows * C, xrows = up_ ? (int64_t)t.x_pad + t.x_L + t.x_slack : 1, x_bs = xrows * 128;
        const size_t u_elems = (size_t)B * u_bs, x_elems = (size_t)B * x_bs, pcm_elems = (size_t)B * L, row_bytes = t.rows ? (size_t)B * t.row_bytes : 0;
        Stage st;
        std::vector<float> img(u_elems, std::nanf("")), xi(up_ ? x_elems : 0, std::nanf(""));   // rows [pad + L] of every utterance as given, NaN in the slack rows behind them
        if (t.u) for (int b = 0; b < B; b++) std::memcpy(img.data() + (size_t)b * u_bs, t.u + (size_t)b * (t.pad + L) * C, (size_t)(t.pad + L) * C * 4);
        if (up_) for (int b = 0; b < B; b++) std::memcpy(xi.data() + (size_t)b * x_bs, t.xin + (size_t)b * (t.x_pad + t.x_L) * 128, (size_t)(t.x_pad + t.x_L) * 128 * 4);
        float *dUo = st.out(u_elems), *dPcm = st.out(pcm_elems);
        uint8_t* dRows = st.out<uint8_t>(row_bytes);
        ResArgs a;
        a.u = st.in(img.data(), u_elems); a.u_bs = u_bs; a.pad = t.pad;
        a.w1 = st.in(w1h.data(), n1); a.w2 = st.in(w2h.data(), n2);
        if (!bf) { a.w1_lo = st.in(w1l.data(), n1); a.w2_lo = st.in(w2l.data(), n2); }
        a.b1 = st.in(t.b1, (size_t)H); a.b2 = st.in(t.b2, (size_t)C);
        a.B = B; a.L = L; a.t0 = t.t0; a.t1 = t.t1; a.C = C; a.H = H; a.k1 = 3; a.k2 = 1; a.w_bf16 = bf; a.final_conv = fin;
        if (fin) {
            a.kf = 3; a.wf_hi = st.in(wfh.data(), nf); a.wf_lo = st.in(wfl.data(), nf);
            a.bf = st.in(t.bf, 1);
            a.pcm = dPcm; a.pcm_bs = L;
            if (t.rows) {
                std::vector<PcmRow> pr((size_t)B);
                for (int b = 0; b < B; b++) pr[b] = PcmRow{dRows + (size_t)b * t.row_bytes, t.rows[2 * b], t.rows[2 * b + 1] != 0};
                a.pcm_rows = st.in(pr.data(), (size_t)B);
            }
        } else a.uo = dUo;
        if (up_) {
            a.fuse_up = 1; a.xin = st.in(xi.data(), x_elems); a.x_bs = x_bs; a.x_pad = t.x_pad; a.x_L = t.x_L; a.CI = 128; a.up_stride = 4; a.wup = st.in(wuh.data(), nu);
            a.bup = st.in(t.bup, 64);
        }
        // refused before any launch: whatever the kernels' own predicates refuse
        if (!(up_ ? resblock_up_shape_supported(a) : resblock_supported(a))) throw Error(PTTS_EINVAL, "ptts_debug_resblock: refused by resblock_supported / resblock_up_shape_supported");
        if (up_) launch_resblock_up_as(a, plan, nullptr);
        else launch_resblock_as(a, plan, nullptr);
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        if (t.launched) { t.launched[0] = plan.nw; t.launched[1] = plan.pers; t.launched[2] = plan.grid; t.launched[3] = plan.tiles; t.launched[4] = plan.tout; }
        if (t.uo) down(t.uo, dUo, u_elems * 4);
        if (t.pcm) down(t.pcm, dPcm, pcm_elems * 4);
        if (t.rows) down(t.row_out, dRows, row_bytes);
    });
}

// ---- the kernels of csrc/ffn_fused.hip stand-alone ----
// the loader's image packers on a caller's matrices (no GPU)
int ptts_debug_mimi_pack(int32_t kind, const float* w1, const float* w2, int32_t n, uint16_t* dst) {
    return guard([&] {
        if (!w1 || !dst || n < 32 || n % 32 || kind < 0 || kind > 1 || (kind == 0 && !w2)) throw Error(PTTS_EINVAL, "ptts_debug_mimi_pack: bad arguments");
        if (kind == 0) pack_ffn_image(w1, w2, n, dst);
        else pack_w1_image(w1, n, dst);
    });
}

// ONE launch of k_mimi_ffn / k_mimi_rowlin on host operands.  Both kernels clamp a block's rows past M to row M - 1 and bound nothing else, so every row of
// both maps and every table position is checked against the caller's buffers here, before anything is uploaded.
int ptts_debug_mimi_fused(const ptts_mimi_fused_args* pa) {
    return guard([&] {
        if (!pa) throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: null argument");
        const ptts_mimi_fused_args& t = *pa;
        if (t.kind < 0 || t.kind > 1) throw Error(PTTS_EINVAL, strfmt("ptts_debug_mimi_fused: unknown kind %d", t.kind));
        const bool ffn = t.kind == 0;
        if (!t.x || !t.ln_w || !t.ln_b || !t.w1 || !t.out || (ffn && !t.w2) || t.M < 1 || t.M > (1 << 20) || t.D < 1 || t.D > 4096 || t.F < 1 || t.F > 8192 ||
            t.x_elems < 1 || t.x_ld < 1 || t.x_rows_per_batch < 0 || t.x_rows_per_batch > INT32_MAX || t.x_batch_stride < 0 || t.x_off < 0 || t.ls_off < 0 || t.ls_off > 64)
            throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: bad arguments");
        if (!ffn && (t.y_elems < 1 || t.y_ld < 1 || t.y_rows_per_batch < 0 || t.y_rows_per_batch > INT32_MAX || t.y_batch_stride < 0 || t.y_off < 0 || t.ls))
            throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: bad arguments for k_mimi_rowlin");
        const bool rope = t.rope_cos || t.rope_sin;
        if (rope && (ffn || !t.rope_cos || !t.rope_sin || t.n_pos < 1 || t.pos0 < 0 || t.rows_per_seg < 0 || t.rope_cols < 0))
            throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: bad RoPE arguments");
        const int M = t.M, D = t.D, F = t.F;
        // the maps against the buffers; rows that are stored to must not overlap (two lanes would store to one element)
        const RowMap xmap{t.x_ld, t.x_rows_per_batch, t.x_batch_stride}, ymap{t.y_ld, t.y_rows_per_batch, t.y_batch_stride};
        check_rows("ptts_debug_mimi_fused", "x", M, t.x_elems, xmap, t.x_off, D, ffn);
        if (!ffn) check_rows("ptts_debug_mimi_fused", "y", M, t.y_elems, ymap, t.y_off, F, true);
        if (rope)
            for (int64_t m = 0; m < M; m++) {
                const int64_t pos = (int64_t)t.pos0 + (t.rows_per_seg ? m % t.rows_per_seg : m);
                if (pos >= t.n_pos) throw Error(PTTS_EINVAL, strfmt("ptts_debug_mimi_fused: row %lld at position %lld, the tables hold %d", (long long)m, (long long)pos, t.n_pos));
            }
        require_device();
        const size_t img_entries = ffn ? ffn_image_count(F) : w1_image_count(F), ntab = rope ? (size_t)t.n_pos * 32 : 0;
        // (allocated here, uploaded behind the predicates: they are what vouches for the widths the uploads and the packers read)
        Stage st;
        Tmp dX((size_t)t.x_elems * 4), dLw((size_t)D * 4), dLb((size_t)D * 4), dLs(((size_t)D + t.ls_off) * 4), dImg(img_entries * 2), dCos(ntab * 4), dSin(ntab * 4);
        float* dY = ffn ? nullptr : st.out((size_t)t.y_elems);
        FfnArgs fa;
        RowLinArgs ra;
        if (ffn) {
            fa.x = dX.as<float>() + t.x_off; fa.xmap = xmap;
            fa.ln_w = dLw.as<float>(); fa.ln_b = dLb.as<float>(); fa.eps = t.eps;
            fa.img = dImg.p;
            if (t.ls) fa.ls = dLs.as<float>() + t.ls_off;
            fa.M = M; fa.D = D; fa.F = F;
            if (!mimi_ffn_supported(fa)) throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: refused by mimi_ffn_supported");
        } else {
            ra.x = dX.as<float>() + t.x_off; ra.xmap = xmap;
            ra.ln_w = dLw.as<float>(); ra.ln_b = dLb.as<float>(); ra.eps = t.eps;
            ra.img = dImg.p;
            ra.y = dY + t.y_off; ra.ymap = ymap;
            if (rope) { ra.rope_cos = dCos.as<float>(); ra.rope_sin = dSin.as<float>(); ra.rope_cols = t.rope_cols; ra.rope_pos0 = t.pos0; ra.rope_rows_per_seg = t.rows_per_seg; }
            ra.M = M; ra.N = F; ra.K = D;
            if (!mimi_rowlin_supported(ra)) throw Error(PTTS_EINVAL, "ptts_debug_mimi_fused: refused by mimi_rowlin_supported");
        }
        // (D == 512 from here on: the packers' width)
        std::vector<uint16_t> img(img_entries);
        if (ffn) pack_ffn_image(t.w1, t.w2, F, img.data());
        else pack_w1_image(t.w1, F, img.data());
        up(dImg.p, img.data(), img_entries * 2);
        up(dX.p, t.x, (size_t)t.x_elems * 4);
        up(dLw.p, t.ln_w, (size_t)D * 4); up(dLb.p, t.ln_b, (size_t)D * 4);
        if (t.ls) up(dLs.as<float>() + t.ls_off, t.ls, (size_t)D * 4);
        if (rope) { up(dCos.p, t.rope_cos, ntab * 4); up(dSin.p, t.rope_sin, ntab * 4); }
        LaunchScope launches;
        launches.run([&] {
            if (ffn) launch_mimi_ffn(fa, nullptr);
            else launch_mimi_rowlin(ra, nullptr);
        });
        PTTS_HIP(hipGetLastError());
        PTTS_HIP(hipDeviceSynchronize());
        put_str(t.launched, t.launched_cap, launches.str());
        if (ffn) down(t.out, dX.p, (size_t)t.x_elems * 4);
        else down(t.out, dY, (size_t)t.y_elems * 4);
    });
}

int ptts_mimi_layer_piece(ptts_model* h, int32_t layer, int32_t which, const float* x, int64_t rows, int32_t pos0, int32_t rows_per_seg, float* out) {
    return guard([&] {
        if (!h || !h->m) throw Error(PTTS_EINVAL, "native-safetensors runtime unavailable");
        Model& m = *h->m;
        const Desc& d = m.d;
        if (!x || !out || rows <= 0 || rows > (1 << 24)) throw Error(PTTS_EINVAL, "ptts-hip: bad rows");
        if (layer < 0 || layer >= d.mimi_layers) throw Error(PTTS_EINVAL, strfmt("ptts-hip: mimi layer %d out of range [0,%d)", layer, d.mimi_layers));
        if (which != PTTS_MIMI_PIECE_QKV && which != PTTS_MIMI_PIECE_FFN) throw Error(PTTS_EINVAL, "ptts-hip: unknown layer piece");
        if (pos0 < 0 || rows_per_seg < 0 || (int64_t)pos0 + (rows_per_seg ? rows_per_seg : rows) > ROPE_SEQ)
            throw Error(PTTS_EINVAL, strfmt("ops: rope cos/sin sequence length too small for pos=%d seq=%lld", pos0, (long long)(rows_per_seg ? rows_per_seg : rows)));
        std::lock_guard<std::mutex> lock(m.mu);
        m.use_device();
        const int C = d.mimi_dim, F = d.mimi_ffn, R = (int)rows;
        const int NO = which == PTTS_MIMI_PIECE_QKV ? 3 * C : C;
        Tmp dx((size_t)R * C * 4), dn((size_t)R * C * 4), dy((size_t)R * std::max(NO, F) * 4);
        PTTS_HIP(hipMemcpyAsync(dx.p, x, (size_t)R * C * 4, hipMemcpyHostToDevice, m.stream));
        if (which == PTTS_MIMI_PIECE_QKV) {
            mimi_layer_qkv(m, layer, dx.as<float>(), RowMap{C, 0, 0}, R, dy.as<float>(), RowMap{3 * C, 0, 0}, pos0, rows_per_seg, dn.as<float>(), m.stream);
            PTTS_HIP(hipMemcpyAsync(out, dy.p, (size_t)R * NO * 4, hipMemcpyDeviceToHost, m.stream));
        } else {
            mimi_layer_ffn(m, layer, dx.as<float>(), RowMap{C, 0, 0}, R, dn.as<float>(), dy.as<float>(), m.stream);
            PTTS_HIP(hipMemcpyAsync(out, dx.p, (size_t)R * NO * 4, hipMemcpyDeviceToHost, m.stream));
        }
        PTTS_HIP(hipStreamSynchronize(m.stream));
    });
}

}  // extern "C"
