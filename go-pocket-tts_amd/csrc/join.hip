// join.hip -- a text's parts copied into one row of 24 kHz audio on the device, with a gap of zeros or a crossfade at the seams (kernels.h
// JoinRow; join.cpp is the host statement and gives the bits).
//
//   k_join   one workgroup per kJoinTile output samples of a part's span, which is its gap zeros and then its own samples up to where its
//            successor's seam begins: [off - gap, off + n).  The spans of a table's rows tile the joined row, so every output sample, zeros
//            included, is written once, by one lane; nothing is cleared beforehand and nothing is atomic.  Lanes walk the DESTINATION in
//            16-byte groups on the destination's own 16-byte grid (a part lands on any sample offset: a 37.5 ms gap is 900 samples): a group
//            inside the span is one float4 store, a group the span's edge cuts is up to three scalar stores.  The source is read as a float4
//            where it happens to be aligned with the destination, else as four consecutive floats; a wave's loads cover one contiguous 1 KiB
//            either way.  In a seam (the part's first k samples) lane j's sample is
//                a[j] * ((float)(k - 1 - j) / (float)k) + b[j] * ((float)j / (float)k)
//            with a = prev, the predecessor's last k samples: dsp_fade_out of that tail plus dsp_fade_in of this head, two IEEE divisions, two
//            products and one sum, each rounded once (__fdiv_rn, __fmul_rn, __fadd_rn: no contraction), as store_tile (dsp.hip) fades.
//            prev may lie in the joined row itself, at the seam's own place (ptts_generate_joined: the predecessor came with an earlier group,
//            whose launch stored its tail unfaded): the lane that reads a[j] there is the lane that then writes the sample.
// Every other sample is moved as its 32 bits: NaN and infinity pass.  Nothing outside a row's span is read or written.
#include "device_util.h"

namespace ptts {

namespace {

__global__ __launch_bounds__(kJoinThreads) void k_join(const JoinRow* __restrict__ rows) {
    const JoinRow r = rows[blockIdx.y];
    const int64_t begin = r.off - r.gap, end = r.off + r.n;
    if (begin >= end) return;
    // the destination's 16-byte grid: group 0 starts at or up to three samples in front of the span
    const int64_t first = begin - (int64_t)(((uintptr_t)(r.dst + begin) >> 2) & 3);
    const int64_t p = first + ((int64_t)blockIdx.x * kJoinThreads + threadIdx.x) * 4;
    if (p >= end) return;
    const int64_t j0 = p - r.off;   // the part's sample that lands on p
    float v[4];
    if (j0 >= r.k && p + 4 <= end && (((uintptr_t)(r.src + j0)) & 15) == 0) {   // behind the seam, whole, and aligned like the destination
        const float4 w = *reinterpret_cast<const float4*>(r.src + j0);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
        const float kf = (float)r.k;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t q = p + u, j = j0 + u;
            float s = 0.0f;                                  // the gap, and the places outside the span that are never stored
            if (q >= r.off && q < end) {
                s = r.src[j];
                if (j < r.k) {
                    const float wa = __fdiv_rn((float)(r.k - 1 - (int32_t)j), kf), wb = __fdiv_rn((float)(int32_t)j, kf);
                    s = __fadd_rn(__fmul_rn(r.prev[j], wa), __fmul_rn(s, wb));
                }
            }
            v[u] = s;
        }
    }
    if (p >= begin && p + 4 <= end) {
        *reinterpret_cast<float4*>(r.dst + p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (p + u >= begin && p + u < end) r.dst[p + u] = v[u];
    }
}

}  // namespace

void launch_join(const JoinRow* rows_dev, int n, int max_tiles, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_join");
    hipLaunchKernelGGL(k_join, dim3((unsigned)max_tiles, (unsigned)n), dim3(kJoinThreads), 0, stream, rows_dev);
}

}  // namespace ptts
