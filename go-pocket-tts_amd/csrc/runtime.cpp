// runtime.cpp -- engine, the parts every phase stands on: host <-> device transfers, model open / share / replicate, the timestep embeddings, the
// pinned result pool.  The phases: batch.cpp (batch state, voices, prefill), step.cpp (AR step and its graphs), mimi_decode.cpp (decoder),
// generate.cpp (request staging, delivery, GenerateAudio).
// Reference call path being replaced: internal/tts/runtime_native_safetensors.go:52-238 ->
// internal/native/{model,flow_lm,flow_transformer,flow_net,mimi}.go.
#include "launch_args.h"

#include <chrono>

#include <algorithm>

namespace ptts {

// Small host->device uploads (slot tables, token ids, per-utterance limits): a copy from pageable memory has to be waited for
// (~20 us each, a dozen per call).  Inside generate_chunk they are staged through a page-locked arena instead and queued
// without a wait; the arena is rewound when the call starts (the previous call ended with the stream drained).
static thread_local UploadArena* tl_upload = nullptr;
static void arena_open(UploadArena& a) {   // allocated on first use, rewound; uploads of this thread go through it until the scope ends
    if (!a.base && hipHostMalloc((void**)&a.base, (size_t)1 << 20, hipHostMallocDefault) == hipSuccess) a.cap = (size_t)1 << 20;
    else if (!a.base) (void)hipGetLastError();
    a.off = 0;
    tl_upload = &a;
}
UploadScope::UploadScope(UploadArena& a, hipStream_t s) {
    (void)hipStreamSynchronize(s);   // normally idle already; after a failed call it may still be reading the arena
    arena_open(a);
}
UploadScope::UploadScope(UploadArena& a, hipEvent_t last_use) {   // an arena of its own, reused once the copies queued from it last time are done
    if (last_use) (void)hipEventSynchronize(last_use);
    arena_open(a);
}
UploadScope::~UploadScope() { tl_upload = nullptr; }
void h2d(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (!bytes) return;
    UploadArena* a = tl_upload;
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (a && a->base && a->off + need <= a->cap) {
        char* stage = a->base + a->off;
        a->off += need;
        std::memcpy(stage, src, bytes);
        PTTS_HIP(hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, s));
        return;
    }
    PTTS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    PTTS_HIP(hipStreamSynchronize(s));
}
void d2h(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (!bytes) return;
    PTTS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    PTTS_HIP(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------------------------
// Model
// ------------------------------------------------------------------------------------------------
Model::~Model() {
    if (upload.base) (void)hipHostFree(upload.base);
    for (hipEvent_t e : prof.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : prof.phase) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (stream2) (void)hipStreamDestroy(stream2);

    cached_batch.reset();
    tcomb.clear();
    for (DevBuf& w : ws) w.release();
    if (own_arena && arena) (void)hipFree(arena);
    if (stream) (void)hipStreamDestroy(stream);
}

// an engine without streams or arena yet: the shapes, the options (on `device`), its own noise-seed stream
static std::unique_ptr<Model> model_on(const Desc& d, const ptts_opts& opts, int device) {
    std::unique_ptr<Model> m(new Model());
    m->d = d;
    m->opts = opts;
    m->opts.device = m->device = device;
    m->noise_state = (uint64_t)std::chrono::system_clock::now().time_since_epoch().count() ^ (uint64_t)(uintptr_t)m.get();
    return m;
}
// ... and its two streams on its device: the step chain at the highest priority, the decoder at the lowest
static void open_streams(Model& m) {
    m.use_device();
    int lo = 0, hi = 0;   // numerically lower = higher priority
    PTTS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    PTTS_HIP(hipStreamCreateWithPriority(&m.stream, hipStreamNonBlocking, hi));
    PTTS_HIP(hipStreamCreateWithPriority(&m.stream2, hipStreamNonBlocking, lo));
}

Model* model_open(Plan* plan, void* device_arena, int fill) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw Error(PTTS_ENODEVICE, "ptts-hip: no HIP device available (this library has no CPU fallback)");
    if (plan->opts.device < 0 || plan->opts.device >= ndev)
        throw Error(PTTS_ENODEVICE, strfmt("ptts-hip: device %d out of range (%d visible)", plan->opts.device, ndev));
    std::unique_ptr<Model> m = model_on(plan->desc, plan->opts, plan->opts.device);
    open_streams(*m);
    if (device_arena) {
        m->arena = reinterpret_cast<uint8_t*>(device_arena);
    } else {
        void* p = nullptr;
        PTTS_HIP(hipMalloc(&p, m->d.total_bytes));
        m->arena = reinterpret_cast<uint8_t*>(p);
        m->own_arena = true;
        fill = 1;
    }
    if (fill) {
        std::vector<uint8_t> host(m->d.total_bytes, 0);
        plan_fill(*plan, host.data());
        PTTS_HIP(hipMemcpy(m->arena, host.data(), host.size(), hipMemcpyHostToDevice));
    }
    return m.release();
}

// A second engine over the weights of `base`: its own streams, KV caches and workspaces, the SAME arena (read-only after load).
// Two engines on one GPU let one batch's Mimi decode (throughput work) run beside the next batch's prefill and AR loop
// (latency-bound, most of the chip idle): tools/serve_bench.py, 256 clients: 9.1 k -> 12.2 k x real time.
Model* model_share(Model& base) {
    std::unique_ptr<Model> m = model_on(base.d, base.opts, base.device);
    open_streams(*m);
    m->arena = base.arena;
    m->own_arena = false;
    return m.release();
}

// The model again on ANOTHER GPU of the same process: its own arena, filled from base's over the GPUs' direct link (hipMemcpyPeer: xGMI on an MI355X node) --
// no second file read, no host staging, no collective library.  This is the shape the reference's server has: ONE process holding N workers
// (internal/server/server.go:119-143,398-421; cmd/pockettts/serve.go:15-52); there the workers share one CPU model, here every GPU gets the bytes once at
// start-up and a dispatcher over the N models deals the requests (dispatcher.cpp: one worker thread per model, each on its own device).  `device` may be
// base's own (a second private copy on the same GPU: what a one-GPU box can test).
Model* model_replicate(Model& base, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(PTTS_ENODEVICE, "ptts-hip: no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) throw Error(PTTS_ENODEVICE, strfmt("ptts-hip: device %d out of range (%d visible)", device, ndev));
    std::unique_ptr<Model> m = model_on(base.d, base.opts, device);
    {   // base's arena is complete and idle-readable: nothing of base may be mid-upload (model_open returns after its copy)
        std::lock_guard<std::mutex> lock(base.mu);
        base.use_device();
        PTTS_HIP(hipStreamSynchronize(base.stream));
    }
    open_streams(*m);
    void* p = nullptr;
    PTTS_HIP(hipMalloc(&p, m->d.total_bytes));
    m->arena = reinterpret_cast<uint8_t*>(p);
    m->own_arena = true;
    if (device != base.device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, base.device) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(base.device, 0);   // (speed only: hipMemcpyPeer stages through the host without it)
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
    }
    PTTS_HIP(hipMemcpyPeer(m->arena, device, base.arena, base.device, m->d.total_bytes));
    PTTS_HIP(hipDeviceSynchronize());
    return m.release();
}

// the measurement pass's figures since ptts_profile_enable or the last read (bench.py), and the counters back to zero.  The caller holds m.mu
void profile_read(Model& m, ptts_profile* out) {
    PTTS_HIP(hipStreamSynchronize(m.stream));
    std::memset(out, 0, sizeof *out);
    double ms = 0;
    for (size_t i = 0; i + 1 < m.prof.used; i += 2) {
        float t = 0;
        PTTS_HIP(hipEventElapsedTime(&t, m.prof.ev[i], m.prof.ev[i + 1]));
        ms += t;
    }
    out->launches = m.prof.launches;
    out->total_ms = ms;
    out->algorithmic_bytes = m.prof.bytes;
    out->weight_bytes = m.prof.wbytes;
    if (m.prof.phases) {
        PTTS_HIP(hipStreamSynchronize(m.stream2));
        float t = 0;
        PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[0], m.prof.phase[1])); out->prefill_ms = t;
        PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[1], m.prof.phase[2])); out->ar_loop_ms = t;
        PTTS_HIP(hipEventElapsedTime(&t, m.prof.phase[3], m.prof.phase[4])); out->mimi_ms = t;
    }
    snprintf(out->kernel, sizeof out->kernel, "%s", "k_skinny");
    m.prof.used = 0; m.prof.bytes = 0; m.prof.wbytes = 0; m.prof.launches = 0; m.prof.phases = false;
}

// timestep embedder (flow_net.go:42-83) for one (s, t) pair, then 0.5*(e_s + e_t) (flow_net.go:320-335)
void Model::compute_tcomb(float sv, float tv, float* dst) {
    const int C = d.flow_dim, nf = d.nfreq;
    DevBuf& wsb = work(WORK_TCOMB, (size_t)(2 * nf + 3 * C) * sizeof(float));
    float* feat = wsb.as<float>();
    float* h = feat + 2 * nf;
    float* e[2] = {h + C, h + 2 * C};
    const float tvals[2] = {sv, tv};
    for (int i = 0; i < 2; i++) {
        const auto& te = d.te[i];
        if (te.l1.in != 2 * nf) throw Error(PTTS_EFORMAT, "native: timestep embedder width mismatch");
        launch_timestep_features(tvals[i], at<float>(te.freqs), nf, feat, stream);
        GemmArgs g1 = mk(*this, feat, flat(2 * nf), te.l1, h, flat(C), 1);
        g1.epi = EPI_SILU;
        launch_gemm(g1, stream);
        GemmArgs g2 = mk(*this, h, flat(C), te.l2, e[i], flat(C), 1);
        launch_gemm(g2, stream);
        launch_rmsnorm_alpha(e[i], at<float>(te.alpha), 1e-5f, 1, C, stream);
    }
    launch_avg2(e[0], e[1], dst, C, stream);
}

const float* Model::tcomb_for(int n) {
    auto it = tcomb.find(n);
    if (it != tcomb.end()) return it->second->as<float>();
    std::unique_ptr<DevBuf> buf(new DevBuf());
    buf->ensure((size_t)n * d.flow_dim * sizeof(float));
    for (int i = 0; i < n; i++)  // flow_lm.go:325-329: s = i/n, t = (i+1)/n in float32
        compute_tcomb((float)i / (float)n, (float)(i + 1) / (float)n, buf->as<float>() + (size_t)i * d.flow_dim);
    PTTS_HIP(hipStreamSynchronize(stream));
    const float* p = buf->as<float>();
    tcomb[n] = std::move(buf);
    return p;
}

// ------------------------------------------------------------------------------------------------
// pinned result pool
// ------------------------------------------------------------------------------------------------
namespace {
struct PinnedPool {
    std::mutex mu;
    std::map<void*, size_t> owned;                    // every live pinned block -> its (rounded) size
    std::multimap<size_t, void*> free_blocks;         // size -> block
    size_t free_bytes = 0;
    static constexpr size_t kKeep = (size_t)1 << 30;  // keep at most 1 GiB of idle pinned memory
};
PinnedPool& pool() { static PinnedPool* p = new PinnedPool(); return *p; }   // leaked on purpose: results may outlive static destructors
}  // namespace

void* result_alloc(size_t bytes) {
    const size_t sz = (std::max<size_t>(bytes, 1) + 65535) & ~(size_t)65535;
    PinnedPool& pp = pool();
    {
        std::lock_guard<std::mutex> lock(pp.mu);
        auto it = pp.free_blocks.lower_bound(sz);
        if (it != pp.free_blocks.end() && it->first <= sz * 2) {
            void* p = it->second;
            pp.free_bytes -= it->first;
            pp.free_blocks.erase(it);
            return p;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, sz, hipHostMallocDefault) != hipSuccess || !p) {
        (void)hipGetLastError();
        return malloc(sz);   // still a valid result buffer for the copy path (result_is_pinned() says no: never handed to a kernel)
    }
    std::lock_guard<std::mutex> lock(pp.mu);
    pp.owned[p] = sz;
    return p;
}

bool result_is_pinned(const void* p) {
    PinnedPool& pp = pool();
    std::lock_guard<std::mutex> lock(pp.mu);
    return p && pp.owned.count(const_cast<void*>(p)) != 0;
}

void result_free(void* p) {
    if (!p) return;
    PinnedPool& pp = pool();
    size_t sz = 0;
    {
        std::lock_guard<std::mutex> lock(pp.mu);
        auto it = pp.owned.find(p);
        if (it == pp.owned.end()) { free(p); return; }
        sz = it->second;
        if (pp.free_bytes + sz <= PinnedPool::kKeep) {
            pp.free_blocks.emplace(sz, p);
            pp.free_bytes += sz;
            return;
        }
        pp.owned.erase(it);
    }
    (void)hipHostFree(p);
}

}  // namespace ptts
