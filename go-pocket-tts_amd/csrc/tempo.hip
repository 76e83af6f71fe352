// tempo.hip -- the speaking rate of the parts of a joined text on ragged rows of 24 kHz audio, from one buffer into another, behind the trim and
// in front of k_join (kernels.h TempoRow; tempo.h has the rule, tempo.cpp is the host statement and gives the bits).
//
//   k_tempo_plan    one workgroup of 256 threads per row, the hops in order (p_k needs p_(k-1): the walk is serial, the rows are parallel).  Per
//                   hop the workgroup fills LDS with the quantised template (the Hs samples at c_k) and the quantised window (the 2 D + Hs
//                   samples from a_k - D), quantising on the fill and biased to unsigned 16 bits; a read outside the row is the bias, a
//                   quantised zero.  Thread t sums |window - template| for the lags 2 t and 2 t + 1 of the 481, packs each sum with its lag into
//                   the key (tempo_key: least S, then least |d|, then the negative d), and the least key comes from shuffles within a wave and
//                   one LDS step across the four; every thread then knows p_k = a_k + d*, and thread 0 stores it.  The trip count F is the
//                   same for every thread, the barriers are __syncthreads alone: no spin, no flag, no hand-off between workgroups.
//   k_tempo_store   on the grid of the DSP stages (dsp_tile.h: tiles of 1920 = 4 hops, one wave a workgroup): output sample m of hop k is the
//                   input's x[p_k + j] as its 32 bits where the hop continues its predecessor (k == 0 or p_k == p_(k-1) + Hs), else the blend
//                   of the predecessor's continuation and the new segment: two divisions (__fdiv_rn), two products, one sum, each rounded once
//                   (contraction is switched off around them).  A row with n_out == 0 writes nothing.
// Nothing is atomic and nothing is cleared beforehand; every output sample and every position is written once, by one thread; nothing outside
// [0, n) is read, and nothing at or beyond n_out (samples) or F (positions) is written.  Sample indices are 64-bit.
#include "device_util.h"
#include "dsp_tile.h"
#include "tempo.h"

namespace ptts {

namespace {

constexpr int kTempoThreads = 256;
constexpr uint32_t kTempoBias = 32767;   // quantised values -32767 .. 32767 as 0 .. 65534
constexpr int kTempoWindowPadded = kTempoWindow + 8;   // the last odd lag's funnel shift reads one word behind the window
static_assert(kTempoLags <= 2 * kTempoThreads && kTempoHop % 8 == 0 && kDspTile % kTempoHop == 0, "two lags a thread; the template is read eight at a time; a tile is whole hops");

// the pair that starts at the upper half of lo and ends at the lower half of hi
__device__ __forceinline__ uint32_t odd(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }
// |a.lo - b.lo| + |a.hi - b.hi| + acc on unsigned 16-bit halves
__device__ __forceinline__ uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u16(a, b, acc); }

__device__ __forceinline__ uint16_t quant_at(const float* __restrict__ x, int64_t n, int64_t i) {
    return (uint16_t)((uint32_t)(i >= 0 && i < n ? tempo_quant(x[i]) : 0) + kTempoBias);
}

__global__ __launch_bounds__(kTempoThreads) void k_tempo_plan(const TempoRow* __restrict__ rows, const TempoScan* __restrict__ designs) {
    __shared__ __attribute__((aligned(16))) uint16_t tmpl[kTempoHop];
    __shared__ __attribute__((aligned(16))) uint16_t win[kTempoWindowPadded];
    __shared__ unsigned long long least[kTempoThreads / WAVE];
    const TempoRow r = rows[blockIdx.x];
    const int32_t speed = designs[r.design].speed;
    const int64_t n = r.n, F = tempo_hops(r.n_out);
    if (F <= 0) return;
    const int t = threadIdx.x;
    if (t == 0) r.p[0] = 0;
    // The thread's two lags are NEIGHBOURS, 2 t and 2 t + 1 as window offsets: both read the same aligned 32-bit words of the window, the odd
    // one through a funnel shift by 16 bits, so no LDS read is misaligned and lane l reads the word next to lane l - 1's.  Threads behind the
    // last lag compute in bounds (as thread kTempoLags / 2) and are not counted
    const int pair = min(t, kTempoLags / 2);
    const int lag0 = 2 * pair, lag1 = lag0 + 1;
    const bool one = 2 * t < kTempoLags, two = 2 * t + 1 < kTempoLags;
    const uint32_t* const w = reinterpret_cast<const uint32_t*>(win) + pair;
    int64_t prev = 0;
    for (int64_t k = 1; k < F; k++) {
        const int64_t a = tempo_target(k, speed), c = prev + kTempoHop;
        for (int i = t; i < kTempoHop; i += kTempoThreads) tmpl[i] = quant_at(r.src, n, c + i);
        for (int i = t; i < kTempoWindowPadded; i += kTempoThreads) win[i] = quant_at(r.src, n, i < kTempoWindow ? a - kTempoRadius + i : (int64_t)-1);
        __syncthreads();
        uint32_t S0 = 0, S1 = 0;
        uint32_t w0 = w[0];
#pragma unroll 2
        for (int j = 0; j < kTempoHop; j += 8) {
            // eight values at a time as four pairs: the template's are the same for every lane (a broadcast read); one v_sad_u16 adds the
            // absolute differences of both halves of a pair
            const uint4 tv = *reinterpret_cast<const uint4*>(tmpl + j);
            const uint32_t w1 = w[j / 2 + 1], w2 = w[j / 2 + 2], w3 = w[j / 2 + 3], w4 = w[j / 2 + 4];
            S0 = sad2(w0, tv.x, S0); S0 = sad2(w1, tv.y, S0); S0 = sad2(w2, tv.z, S0); S0 = sad2(w3, tv.w, S0);
            S1 = sad2(odd(w1, w0), tv.x, S1); S1 = sad2(odd(w2, w1), tv.y, S1); S1 = sad2(odd(w3, w2), tv.z, S1); S1 = sad2(odd(w4, w3), tv.w, S1);
            w0 = w4;
        }
        unsigned long long key = one ? (unsigned long long)tempo_key((int32_t)S0, lag0 - kTempoRadius) : ~0ull;
        if (two) key = min(key, (unsigned long long)tempo_key((int32_t)S1, lag1 - kTempoRadius));
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, WAVE));
        if ((t & (WAVE - 1)) == 0) least[t / WAVE] = key;
        __syncthreads();   // behind it nobody reads tmpl or win any more: the next hop may fill them
        key = least[0];
#pragma unroll
        for (int w = 1; w < kTempoThreads / WAVE; w++) key = min(key, least[w]);
        prev = a + tempo_key_lag(key);
        if (t == 0) r.p[k] = (int32_t)prev;
        // (least[] is written again behind the next hop's first barrier, which every thread reaches only after this read)
    }
}

__device__ __forceinline__ uint32_t bits_at(const float* __restrict__ x, int64_t n, int64_t i) {
    return i >= 0 && i < n ? reinterpret_cast<const uint32_t*>(x)[i] : 0u;
}

__global__ __launch_bounds__(kDspLanes) void k_tempo_store(const TempoRow* __restrict__ rows) {
    const TempoRow r = rows[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * kDspTile;
    if (base >= r.n_out) return;
    const int cnt = (int)min((int64_t)kDspTile, r.n_out - base);
    const int64_t k0 = base / kTempoHop;
    uint32_t* const dst = reinterpret_cast<uint32_t*>(r.dst);
    for (int q = threadIdx.x; q < cnt; q += kDspLanes) {
        const int h = q / kTempoHop, j = q - h * kTempoHop;
        const int64_t k = k0 + h, p = r.p[k];
        uint32_t v = bits_at(r.src, r.n, p + j);
        if (k > 0) {
            const int64_t c = (int64_t)r.p[k - 1] + kTempoHop;
            if (c != p) {
#pragma clang fp contract(off)
                // Plain operators under the pragma, as store_tile (dsp.hip) fades: __fmul_rn and __fadd_rn are inline functions whose
                // operations keep the contraction their header was compiled with, and the second product was fused into the sum
                const float xa = __uint_as_float(bits_at(r.src, r.n, c + j)), xb = __uint_as_float(v);
                const float pa = xa * tempo_w_out(j), pb = xb * tempo_w_in(j);
                v = __float_as_uint(pa + pb);
            }
        }
        dst[base + q] = v;
    }
}

}  // namespace

void launch_tempo(const TempoRow* rows_dev, int n, int max_tiles, const TempoScan* designs_dev, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;   // empty rows only: no position, no sample
    note_launch("k_tempo_plan");
    hipLaunchKernelGGL(k_tempo_plan, dim3((unsigned)n), dim3(kTempoThreads), 0, stream, rows_dev, designs_dev);
    note_launch("k_tempo_store");
    hipLaunchKernelGGL(k_tempo_store, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev);
}

}  // namespace ptts
