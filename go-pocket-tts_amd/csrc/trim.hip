// trim.hip -- silence control of the parts of a joined text on ragged rows of 24 kHz audio, from one buffer into another, in front of k_join
// (kernels.h TrimRow, TrimTile; trim.h has the rule, trim.cpp is the host statement and gives the bits).  Three
// launches on the grid of the DSP stages: one wave per workgroup, lane l owns run l of its tile.
//
//   k_trim_mark    every tile: the loud samples of its runs as a bit mask per lane (one float comparison per sample against t), the tile's
//                  first and last loud index, and the cuts whose two loud ends both lie in the tile -- each counted by the lane of its later
//                  end, which knows the last loud index in front of its run from an exclusive prefix maximum over the wave.
//   k_trim_carry   one workgroup per row, 64 tiles at a time, lane j on tile c0 + j: "the last loud index in front of tile f" is the
//                  exclusive prefix maximum of the tiles' last loud indices, carried from one group of 64 to the next; "the first loud index
//                  behind tile f" the exclusive suffix minimum of their first ones, carried backward.  The two ends of the sweeps are L.first
//                  and L.last: the row's lo and hi.  A tile then keeps its samples inside [lo, hi) less what its inner cuts lose less the
//                  overlap of the tile with the cuts that cross its edges (trim_cut_in: between prev and first, between last and next, or,
//                  in a tile without a loud sample, between prev and next); the exclusive prefix of that is where the tile's output begins.
//                  A cut that crosses tiles is counted where its later end lies.  Lane 0 writes the row's ptts_trim_info.
//   k_trim_store   every tile: the masks again; a lane's quiet samples are decided from the two loud indices around them (trim_keep), which
//                  come from the lane's own mask, from its neighbours' (prefix maximum, suffix minimum) or from the carried pair; an exclusive
//                  prefix sum of the runs' kept counts gives each lane its place in the tile's output, which is gathered in LDS and stored
//                  in one piece at the tile's offset.
// Nothing is atomic and nothing is cleared beforehand; every output sample is written once, by one lane; nothing at or beyond n is read, and
// nothing at or beyond n_out is written.  Index arithmetic that involves a tile's base is 64-bit; an index itself fits 31 bits (a row has
// fewer than 2^31 samples).  No transcendental function: t comes designed from the host.
#include "device_util.h"
#include "dsp_tile.h"

namespace ptts {

namespace {

static_assert(kDspLanes == WAVE && kDspRun < 32, "a run's loud samples are one 32-bit mask, a tile's runs one wave");

struct OpMax { __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; } };
struct OpMin { __device__ int32_t operator()(int32_t a, int32_t b) const { return a < b ? a : b; } };
struct OpAdd { __device__ int32_t operator()(int32_t a, int32_t b) const { return a + b; } };

// the inclusive scan of v over lanes 0 .. l (every lane of the wave calls it)
template <class Op>
__device__ __forceinline__ int32_t scan_up(int32_t v, Op op) {
    const int l = threadIdx.x;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int32_t o = __shfl_up(v, d, WAVE);
        if (l >= d) v = op(v, o);
    }
    return v;
}
// ... and over lanes l .. 63
template <class Op>
__device__ __forceinline__ int32_t scan_down(int32_t v, Op op) {
    const int l = threadIdx.x;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int32_t o = __shfl_down(v, d, WAVE);
        if (l + d < WAVE) v = op(v, o);
    }
    return v;
}
// an inclusive scan made exclusive: the lane in front's value (behind's), `none` for the first (last) lane
__device__ __forceinline__ int32_t before(int32_t incl, int32_t none) {
    const int32_t o = __shfl_up(incl, 1, WAVE);
    return threadIdx.x == 0 ? none : o;
}
__device__ __forceinline__ int32_t behind(int32_t incl, int32_t none) {
    const int32_t o = __shfl_down(incl, 1, WAVE);
    return threadIdx.x == WAVE - 1 ? none : o;
}

// the loud samples of the lane's run (c of them) as a mask: bit i is sample l * kDspRun + i of the tile
__device__ __forceinline__ uint32_t loud_mask(const float* tile, int c, float t) {
    const float* run = tile + threadIdx.x * kDspRun;
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < kDspRun; i++)
        if (i < c && trim_loud(run[i], t)) m |= 1u << i;
    return m;
}
__device__ __forceinline__ int32_t mask_first(uint32_t m, int32_t b0) { return m ? b0 + (__ffs((int)m) - 1) : kTrimNoneBehind; }
__device__ __forceinline__ int32_t mask_last(uint32_t m, int32_t b0) { return m ? b0 + (31 - __clz((int)m)) : kTrimNone; }

__global__ __launch_bounds__(kDspLanes) void k_trim_mark(const TrimRow* __restrict__ rows, const TrimScan* __restrict__ designs) {
    __shared__ float tile[kDspTile];
    const TrimRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const TrimScan d = designs[r.design];
    tile_load(r.src + base, cnt, tile);
    __syncthreads();
    const int l = threadIdx.x;
    const int32_t b0 = (int32_t)base + l * kDspRun;   // the row index of the run's first sample
    const uint32_t mask = loud_mask(tile, run_count(cnt), d.t);
    const int32_t first = mask_first(mask, b0), last = mask_last(mask, b0);
    const int32_t last_upto = scan_up(last, OpMax());
    int64_t u = before(last_upto, kTrimNone);   // the last loud index of the tile in front of the run
    int32_t removed = 0, cuts = 0;
    for (uint32_t m = mask; m; m &= m - 1) {
        const int64_t v = b0 + (__ffs((int)m) - 1);
        int64_t a, b;
        trim_cut(u, v, d.M, &a, &b);
        if (b > a) { removed += (int32_t)(b - a); cuts++; }
        u = v;
    }
    removed = wave_sum(removed);
    cuts = wave_sum(cuts);
    const int32_t tile_last = __shfl(last_upto, WAVE - 1, WAVE), tile_first = __shfl(scan_down(first, OpMin()), 0, WAVE);
    if (l == 0) {
        TrimTile& t = r.tiles[blockIdx.x];
        t.first = tile_first; t.last = tile_last; t.removed = removed; t.cuts = cuts;
    }
}

__global__ __launch_bounds__(kDspLanes) void k_trim_carry(const TrimRow* __restrict__ rows, const TrimScan* __restrict__ designs) {
    const TrimRow& r = rows[blockIdx.x];
    const TrimScan d = designs[r.design];
    const int64_t n = r.n > 0 ? r.n : 0, F = scan_tiles(n);
    const int l = threadIdx.x;
    TrimTile* const tiles = r.tiles;
    // A tile is lane (f mod 64)'s in every sweep: the lane that stored prev and next is the lane that reads them
    int32_t carry = kTrimNone;
    for (int64_t c0 = 0; c0 < F; c0 += WAVE) {
        const int64_t f = c0 + l;
        const int32_t upto = scan_up(f < F ? tiles[f].last : kTrimNone, OpMax());
        const int32_t prev = max(carry, before(upto, kTrimNone));
        if (f < F) tiles[f].prev = prev;
        carry = max(carry, __shfl(upto, WAVE - 1, WAVE));
    }
    const int64_t L_last = carry;
    carry = kTrimNoneBehind;
    for (int64_t c0 = F > 0 ? (F - 1) / WAVE * WAVE : -1; c0 >= 0; c0 -= WAVE) {
        const int64_t f = c0 + l;
        const int32_t from = scan_down(f < F ? tiles[f].first : kTrimNoneBehind, OpMin());
        const int32_t next = min(carry, behind(from, kTrimNoneBehind));
        if (f < F) tiles[f].next = next;
        carry = min(carry, __shfl(from, 0, WAVE));
    }
    const int64_t L_first = carry;
    const bool speech = L_last >= 0;
    const int64_t lo = speech && d.edges ? max((int64_t)0, L_first - d.H) : 0;
    const int64_t hi = speech && d.edges ? min(n, L_last + 1 + d.H) : n;
    int64_t total = 0, cuts = 0;
    for (int64_t c0 = 0; c0 < F; c0 += WAVE) {
        const int64_t f = c0 + l;
        int32_t kept = 0, cut = 0;
        if (f < F) {
            const TrimTile t = tiles[f];
            const int64_t A = f * kDspTile, B = min(n, A + kDspTile);
            if (!speech) {
                kept = (int32_t)(B - A);
            } else {
                const int64_t in = max((int64_t)0, min(B, hi) - max(A, lo));
                int64_t gone;
                if (t.last != kTrimNone) {
                    gone = t.removed + trim_cut_in(t.prev, t.first, d.M, A, B) + trim_cut_in(t.last, t.next, d.M, A, B);
                    int64_t a, b;
                    trim_cut(t.prev, t.first, d.M, &a, &b);
                    cut = t.cuts + (b > a ? 1 : 0);
                } else {
                    gone = trim_cut_in(t.prev, t.next, d.M, A, B);
                }
                kept = (int32_t)(in - gone);
            }
        }
        const int32_t upto = scan_up(kept, OpAdd());
        const int32_t in_front = before(upto, 0);
        if (f < F) tiles[f].off = (int32_t)(total + in_front);
        total += __shfl(upto, WAVE - 1, WAVE);
        cuts += wave_sum(cut);
    }
    if (l == 0) {
        ptts_trim_info& o = *r.info;
        o.lo = lo; o.hi = hi; o.n_out = total; o.cuts = cuts; o.speech = speech ? 1 : 0; o.reserved = 0;
    }
}

__global__ __launch_bounds__(kDspLanes) void k_trim_store(const TrimRow* __restrict__ rows, const TrimScan* __restrict__ designs) {
    __shared__ float tile[kDspTile];
    __shared__ float kept[kDspTile];
    const TrimRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    const TrimScan d = designs[r.design];
    const ptts_trim_info o = *r.info;
    const TrimTile t = r.tiles[blockIdx.x];
    tile_load(r.src + base, cnt, tile);
    __syncthreads();
    const int l = threadIdx.x, c = run_count(cnt);
    const int32_t b0 = (int32_t)base + l * kDspRun;
    const uint32_t mask = loud_mask(tile, c, d.t);
    // the loud indices around the run: the tile's other runs', else the carried pair
    const int32_t u0 = max(t.prev, before(scan_up(mask_last(mask, b0), OpMax()), kTrimNone));
    const int32_t v1 = min(t.next, behind(scan_down(mask_first(mask, b0), OpMin()), kTrimNoneBehind));
    uint32_t keep = 0;
    if (!o.speech) {
        keep = (1u << c) - 1u;
    } else {
        int64_t u = u0;
#pragma unroll
        for (int i = 0; i < kDspRun; i++) {
            if (i >= c) continue;
            if (mask >> i & 1u) {   // a loud sample lies inside [lo, hi) and in no cut
                keep |= 1u << i;
                u = b0 + i;
            } else {
                const uint32_t above = mask & ~((2u << i) - 1u);
                const int64_t v = above ? (int64_t)b0 + (__ffs((int)above) - 1) : (int64_t)v1;
                if (trim_keep((int64_t)b0 + i, u, v, d.M, o.lo, o.hi)) keep |= 1u << i;
            }
        }
    }
    const int32_t upto = scan_up(__popc(keep), OpAdd());
    int at = before(upto, 0);
    const int all = __shfl(upto, WAVE - 1, WAVE);
    const float* run = tile + l * kDspRun;
    for (uint32_t m = keep; m; m &= m - 1) kept[at++] = run[__ffs((int)m) - 1];
    __syncthreads();
    // (what the carry counted is what the lanes kept; the bound holds whatever either did)
    const int64_t room = o.n_out - (int64_t)t.off;
    const int out = (int)max((int64_t)0, min((int64_t)all, min(room, n - (int64_t)t.off)));
    if (t.off >= 0) tile_store(r.dst + t.off, out, kept);
}

}  // namespace

void launch_trim(const TrimRow* rows_dev, int n, int max_tiles, const TrimScan* designs_dev, hipStream_t stream) {
    if (n <= 0) return;
    const dim3 tiles((unsigned)max(max_tiles, 1), (unsigned)n), lanes(kDspLanes);
    if (max_tiles > 0) {
        note_launch("k_trim_mark");
        hipLaunchKernelGGL(k_trim_mark, tiles, lanes, 0, stream, rows_dev, designs_dev);
    }
    note_launch("k_trim_carry");
    hipLaunchKernelGGL(k_trim_carry, dim3((unsigned)n), lanes, 0, stream, rows_dev, designs_dev);
    if (max_tiles > 0) {
        note_launch("k_trim_store");
        hipLaunchKernelGGL(k_trim_store, tiles, lanes, 0, stream, rows_dev, designs_dev);
    }
}

}  // namespace ptts
