// resample.hip -- k_resample: rate and format conversion of delivered audio (kernels.h ResampleRow).
// One launch converts a table of rows.  Workgroup (tile, row) stages the row's taps (tables up to kResampleTapsLds floats) and the
// tile's input window in LDS with 16-byte loads; every lane then produces 4 consecutive outputs, each one f32 fmaf chain over
// ascending input index, and stores them in the row's format.  The order of the sum is fixed per output, so the result does not
// depend on tiles, batching or ranges: a streamed hand-over equals the one-shot conversion bit for bit.
#include <atomic>

#include "device_util.h"

namespace ptts {

namespace {

// ITU-T G.711 as the classic linear2ulaw / linear2alaw code states it, applied to WritePCM16Samples' int16
__device__ __forceinline__ int g711_segment(int v, int first) {   // the first s with v < first << s (8: past the last segment)
    int s = 0;
    while (s < 8 && v >= (first << s)) s++;
    return s;
}
__device__ __forceinline__ uint32_t ulaw_one(int v) {    // bias 0x84, clip 32635, inverted bits
    int mask = 0xFF;
    if (v < 0) { v = -v; mask = 0x7F; }
    if (v > 32635) v = 32635;
    v += 0x84;
    const int seg = g711_segment(v, 0x100);
    const int u = seg >= 8 ? 0x7F : ((seg << 4) | ((v >> (seg + 3)) & 0xF));
    return (uint32_t)((u ^ mask) & 0xFF);
}
__device__ __forceinline__ uint32_t alaw_one(int v) {    // 13-bit input v >> 3, XOR 0x55 (negative) or 0xD5
    v >>= 3;
    int mask = 0xD5;
    if (v < 0) { mask = 0x55; v = -v - 1; }
    const int seg = g711_segment(v, 0x20);
    const int a = seg >= 8 ? 0x7F : ((seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 0xF));
    return (uint32_t)((a ^ mask) & 0xFF);
}

__device__ __forceinline__ float in_or_zero(const float* src, int64_t i, int64_t n) { return (i >= 0 && i < n) ? src[i] : 0.0f; }

__global__ __launch_bounds__(kResampleThreads) void k_resample(const ResampleRow* __restrict__ rows) {
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    const ResampleRow& r = rows[blockIdx.y];
    const int L = r.L, M = r.M, fmt = r.fmt;
    int64_t n_in = r.n_in, o1 = r.o1;
    if (r.nf) {   // streaming: an utterance that has ended is flushed -- its input ends at its last frame, everything past it reads zeros
        const int64_t e = (int64_t)r.nf[0] * r.spf;
        if (r.fin || e < n_in || (r.act[0] == 0 && e <= n_in)) {
            n_in = min(n_in, e);
            o1 = min(r.o_cap, (n_in * L + M - 1) / M);
        }
    }
    const int64_t j0 = r.o0 + (int64_t)blockIdx.x * r.tile;
    if (j0 >= o1) return;
    const int64_t j1 = min(j0 + (int64_t)r.tile, o1);
    const bool ident = r.taps == nullptr;
    const int K = ident ? 1 : r.K;
    const int ntap = ident ? 0 : L * K;
    const bool taps_lds = ntap <= kResampleTapsLds;
    const int tap_floats = taps_lds ? ((ntap + 3) & ~3) : 0;
    float* win = lds + tap_floats;
    // the tile's input window [in0, in1], staged from the 4-aligned a0 (zeros outside [0, n_in))
    const int64_t in0 = ident ? j0 : (j0 * M) / L + r.dlo;
    const int64_t in1 = ident ? j1 - 1 : ((j1 - 1) * M) / L + r.dlo + K - 1;
    const int64_t a0 = in0 - (((in0 % 4) + 4) % 4);
    const int nw = (int)((in1 - a0 + 4) & ~(int64_t)3);
    const bool src16 = ((uintptr_t)r.src & 15) == 0;
    for (int q = threadIdx.x * 4; q < nw; q += kResampleThreads * 4) {
        const int64_t i = a0 + q;
        float4 v;
        if (src16 && i >= 0 && i + 4 <= n_in) v = *reinterpret_cast<const float4*>(r.src + i);
        else v = make_float4(in_or_zero(r.src, i, n_in), in_or_zero(r.src, i + 1, n_in), in_or_zero(r.src, i + 2, n_in), in_or_zero(r.src, i + 3, n_in));
        *reinterpret_cast<float4*>(win + q) = v;
    }
    for (int q = threadIdx.x * 4; q < tap_floats; q += kResampleThreads * 4)
        *reinterpret_cast<float4*>(lds + q) = *reinterpret_cast<const float4*>(r.taps + q);
    __syncthreads();
    const float* taps = taps_lds ? lds : r.taps;
    const int64_t jt = j0 + (int64_t)threadIdx.x * 4;
    if (jt >= j1) return;
    const int nv = (int)min((int64_t)4, j1 - jt);
    float y[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t j = jt + u;
        float acc = 0.0f;
        if (u < nv) {
            if (ident) acc = win[j - a0];
            else {
                const int64_t jm = j * M, base = jm / L;
                const float* h = taps + (int)(jm - base * L) * K;
                const float* x = win + (base + r.dlo - a0);
                for (int k = 0; k < K; k++) acc = fmaf(x[k], h[k], acc);
            }
        }
        y[u] = acc;
    }
    if (fmt == RS_F32) {
        float* d = static_cast<float*>(r.dst) + jt;
        if (nv == 4 && ((uintptr_t)d & 15) == 0) *reinterpret_cast<float4*>(d) = make_float4(y[0], y[1], y[2], y[3]);
        else for (int u = 0; u < nv; u++) d[u] = y[u];
        return;
    }
    int s[4];
#pragma unroll
    for (int u = 0; u < 4; u++) s[u] = pcm16_one(y[u]);
    if (fmt == RS_S16) {
        int16_t* d = static_cast<int16_t*>(r.dst) + jt;
        if (nv == 4 && ((uintptr_t)d & 7) == 0)
            *reinterpret_cast<uint2*>(d) = make_uint2((unsigned)(s[0] & 0xffff) | ((unsigned)s[1] << 16), (unsigned)(s[2] & 0xffff) | ((unsigned)s[3] << 16));
        else for (int u = 0; u < nv; u++) d[u] = (int16_t)s[u];
        return;
    }
    uint32_t b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) b[u] = fmt == RS_ULAW ? ulaw_one(s[u]) : alaw_one(s[u]);
    uint8_t* d = static_cast<uint8_t*>(r.dst) + jt;
    if (nv == 4 && ((uintptr_t)d & 3) == 0) *reinterpret_cast<uint32_t*>(d) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    else for (int u = 0; u < nv; u++) d[u] = (uint8_t)b[u];
}

}  // namespace

std::atomic<int64_t> g_resample_launches{0};

void launch_resample(const ResampleRow* rows_dev, int n, int max_tiles, size_t lds_bytes, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_resample");
    g_resample_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_resample, dim3((unsigned)max_tiles, (unsigned)n), dim3(kResampleThreads), lds_bytes, stream, rows_dev);
}

}  // namespace ptts
