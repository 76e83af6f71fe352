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
//   k_join_gain   the same lanes and stores for a table in which a part has a volume (kernels.h JoinGainRow; include/ptts.h ptts_part_opts): the
//            part's samples, and its predecessor's tail in a seam, are multiplied by their gains first -- an immediate f32, or the word a loudness
//            row's k_loud_gate left on the device (a measured gain of 1 multiplies nothing) -- one __fmul_rn each, never contracted with the seam's
//            products.  A separate instantiation: k_join's code does not know the gains.  A tail that lies in the joined row is already scaled.
// Every other sample is moved as its 32 bits: NaN and infinity pass.  Nothing outside a row's span is read or written.
#include "device_util.h"

namespace ptts {

namespace {

// One lane's group of four output samples of row r.  GAIN: the part's samples are multiplied by gb where sb is set, the predecessor's tail by ga where
// sa is set, one __fmul_rn each in front of the seam arithmetic; without GAIN the four arguments are not read and the code is k_join's own
template <bool GAIN>
__device__ __forceinline__ void join_group(const JoinRow& r, bool sb, float gb, bool sa, float ga) {
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
        if (GAIN && sb) {
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = __fmul_rn(v[u], gb);
        }
    } else {
        const float kf = (float)r.k;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t q = p + u, j = j0 + u;
            float s = 0.0f;                                  // the gap, and the places outside the span that are never stored
            if (q >= r.off && q < end) {
                s = r.src[j];
                if (GAIN && sb) s = __fmul_rn(s, gb);
                if (j < r.k) {
                    const float wa = __fdiv_rn((float)(r.k - 1 - (int32_t)j), kf), wb = __fdiv_rn((float)(int32_t)j, kf);
                    float a = r.prev[j];
                    if (GAIN && sa) a = __fmul_rn(a, ga);
                    s = __fadd_rn(__fmul_rn(a, wa), __fmul_rn(s, wb));
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

__global__ __launch_bounds__(kJoinThreads) void k_join(const JoinRow* __restrict__ rows) {
    const JoinRow r = rows[blockIdx.y];
    join_group<false>(r, false, 1.0f, false, 1.0f);
}

// the gain form: a fixed gain multiplies every sample, a measured one (the word k_loud_gate left) where it is not 1, as loud_normalize applies it
__global__ __launch_bounds__(kJoinThreads) void k_join_gain(const JoinGainRow* __restrict__ rows) {
    const JoinGainRow g = rows[blockIdx.y];
    if (g.r.off - g.r.gap >= g.r.off + g.r.n) return;   // (nothing to write: no word is read)
    float gb = g.g, ga = g.g_prev;
    bool sb = (g.flags & JOIN_GAIN_IMM) != 0, sa = (g.flags & JOIN_PREV_IMM) != 0;
    if (g.flags & JOIN_GAIN_WORD) { gb = *g.gw; sb = gb != 1.0f; }
    if ((g.flags & JOIN_PREV_WORD) && g.r.k > 0) { ga = *g.gw_prev; sa = ga != 1.0f; }
    join_group<true>(g.r, sb, gb, sa, ga);
}

}  // namespace

void launch_join(const JoinRow* rows_dev, int n, int max_tiles, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_join");
    hipLaunchKernelGGL(k_join, dim3((unsigned)max_tiles, (unsigned)n), dim3(kJoinThreads), 0, stream, rows_dev);
}

void launch_join_gain(const JoinGainRow* rows_dev, int n, int max_tiles, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;
    note_launch("k_join_gain");
    hipLaunchKernelGGL(k_join_gain, dim3((unsigned)max_tiles, (unsigned)n), dim3(kJoinThreads), 0, stream, rows_dev);
}

}  // namespace ptts
