// loudness.hip -- integrated loudness (ITU-R BS.1770-4, mono, 24 kHz) of ragged rows of decoded audio on the device, and the gain that takes a
// row to its target (kernels.h DspRow, DSP_LOUD; loudness_block.h).  The rows' RAW samples are read, nothing is written
// to them: k_dsp_apply (dsp.hip) applies the gain.
//
//   k_loud_summary  one workgroup per full tile that another tile follows; lane l runs run l of the K-weighting cascade from zero state, lane 0
//                   folds the 64 four-state end states in run order into E_f.
//   k_loud_carry    one workgroup per row; S_0 = 0, S_(f+1) = A^1920 S_f + E_f in tile order.
//   k_loud_energy   every tile: the runs' entering states (t_0 = S_f, t_(l+1) = A^30 t_l + e_l in run order), each run's sum of squared outputs
//                   in sample order, and the tile's four sub-block energies (16 run sums each, in run order) as doubles.
//   k_loud_gate     one workgroup per row: block energies (20 sub-blocks in order, over 9600; lanes take a block each), the absolute and the
//                   relative gate and the means in block order by lane 0, M and the f32 gain min((float)sqrt(T / M), 1 / peak).
// One wave per workgroup and at most 12.5 KB of LDS, as dsp.hip's kernels: a CU holds a dozen workgroups, the passes are reads of the rows at HBM
// rate.  Tiles lie on the row's own grid, every sum has one order: a row's M and gain are a function of the row alone, and they are the bits of
// the host instantiation (loudness.cpp).  Nothing at or beyond n is read.
#include "device_util.h"
#include "loudness_block.h"

namespace ptts {

namespace {

// samples [base, base + cnt) of the row into tile[0, cnt); 16-byte loads where the row's alignment allows
__device__ __forceinline__ void load_raw(const DspRow& r, int64_t base, int cnt, float* tile) {
    const float* src = r.x + base;
    const bool vec = ((uintptr_t)src & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(tile + q) = *reinterpret_cast<const float4*>(src + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) tile[q + u] = src[q + u];
    }
}

__device__ __forceinline__ int64_t row_tiles(const DspRow& r) { return (r.n + kDspTile - 1) / kDspTile; }
__device__ __forceinline__ double* row_states(const DspRow& r, int64_t f) { return r.loud + 2 + f * 8; }          // E_f (4), S_f (4)
__device__ __forceinline__ double* row_subs(const DspRow& r) { return r.loud + 2 + row_tiles(r) * 8; }            // [4 F]

__global__ __launch_bounds__(kDspLanes) void k_loud_summary(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes][4];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_LOUD) || base + kDspTile >= r.n) return;   // only a full tile that another one follows hands a state on
    load_raw(r, base, kDspTile, tile);
    __syncthreads();
    const int l = threadIdx.x;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    (void)loud_run(sc, tile + l * kDspRun, kDspRun, z);
    for (int i = 0; i < 4; i++) e[l][i] = z[i];
    __syncthreads();
    if (l == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < kDspLanes; j++) loud_advance(sc.a_run, s, e[j]);
        double* st = row_states(r, blockIdx.x);
        for (int i = 0; i < 4; i++) st[i] = s[i];
    }
}

__global__ __launch_bounds__(kDspLanes) void k_loud_carry(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ double ein[kDspLanes][4], sout[kDspLanes][4];
    const DspRow& r = rows[blockIdx.x];
    if (!(r.flags & DSP_LOUD) || r.n <= 0) return;
    const int64_t F = row_tiles(r);
    const int l = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};   // lane 0's: the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < F - 1) for (int i = 0; i < 4; i++) ein[l][i] = row_states(r, f)[i];
        __syncthreads();
        if (l == 0) {
            const int m = (int)min((int64_t)kDspLanes, F - c0);
            for (int j = 0; j < m; j++) {
                for (int i = 0; i < 4; i++) sout[j][i] = s[i];
                if (c0 + j < F - 1) loud_advance(sc.a_tile, s, ein[j]);
            }
        }
        __syncthreads();
        if (f < F) for (int i = 0; i < 4; i++) row_states(r, f)[4 + i] = sout[l][i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kDspLanes) void k_loud_energy(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ float4 tile4[kDspTile / 4];
    __shared__ double e[kDspLanes][4], t[kDspLanes][4], q[kDspLanes];
    float* tile = reinterpret_cast<float*>(tile4);
    const DspRow& r = rows[blockIdx.y];
    const int64_t n = r.n, base = (int64_t)blockIdx.x * kDspTile;
    if (!(r.flags & DSP_LOUD) || base >= n) return;
    const int cnt = (int)min((int64_t)kDspTile, n - base);
    load_raw(r, base, cnt, tile);
    __syncthreads();
    const int l = threadIdx.x;
    const int c = max(0, min(kDspRun, cnt - l * kDspRun));
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    (void)loud_run(sc, tile + l * kDspRun, c, z);
    for (int i = 0; i < 4; i++) e[l][i] = z[i];
    __syncthreads();
    if (l == 0) {   // (behind a run that is not full no run follows: its t is not read)
        const double* st = row_states(r, blockIdx.x) + 4;
        double s[4] = {st[0], st[1], st[2], st[3]};
        for (int j = 0; j < kDspLanes; j++) {
            for (int i = 0; i < 4; i++) t[j][i] = s[i];
            loud_advance(sc.a_run, s, e[j]);
        }
    }
    __syncthreads();
    for (int i = 0; i < 4; i++) z[i] = t[l][i];
    q[l] = loud_run(sc, tile + l * kDspRun, c, z);
    __syncthreads();
    // (a sub-block the row ends in holds the sum over the samples that are there; no whole 400 ms block contains it, so the gate never reads it)
    if (l < kLoudSubsPerTile) row_subs(r)[(int64_t)blockIdx.x * kLoudSubsPerTile + l] = loud_sub_energy(q + l * kLoudRunsPerSub);
}

__global__ __launch_bounds__(kDspLanes) void k_loud_gate(const DspRow* __restrict__ rows, const LoudScan sc) {
    __shared__ double z[kDspLanes];
    __shared__ double rel_s;
    const DspRow& r = rows[blockIdx.x];
    if (!(r.flags & DSP_LOUD)) return;
    const int64_t nb = loud_blocks(r.n);
    const double* sub = row_subs(r);
    const int l = threadIdx.x;
    LoudAcc first{0.0, 0}, second{0.0, 0};   // lane 0's
    for (int pass = 0; pass < 2; pass++) {
        const double rel = pass ? rel_s : sc.abs_gate;
        for (int64_t c0 = 0; c0 < nb; c0 += kDspLanes) {
            if (c0 + l < nb) z[l] = loud_block_energy(sub, c0 + l);
            __syncthreads();
            if (l == 0) {
                const int m = (int)min((int64_t)kDspLanes, nb - c0);
                for (int j = 0; j < m; j++) loud_gate_add(pass ? second : first, z[j], sc.abs_gate, rel);
            }
            __syncthreads();
        }
        if (pass == 0) {
            if (l == 0) rel_s = first.cnt ? loud_rel_gate(first) : 0.0;
            __syncthreads();
        }
    }
    if (l == 0) {
        const double M = (first.cnt && second.cnt) ? loud_div(second.sum, (double)second.cnt) : 0.0;
        r.loud[0] = M;
        *reinterpret_cast<float*>(r.loud + 1) = loud_gain(M, r.target, __uint_as_float(*r.peak));
    }
}

}  // namespace

void launch_loudness(const DspRow* rows_dev, int n, int max_tiles, const LoudScan& scan, hipStream_t stream) {
    if (n <= 0) return;
    if (max_tiles > 1) {
        note_launch("k_loud_summary");
        hipLaunchKernelGGL(k_loud_summary, dim3((unsigned)(max_tiles - 1), (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
    }
    if (max_tiles > 0) {
        note_launch("k_loud_carry");
        hipLaunchKernelGGL(k_loud_carry, dim3((unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
        note_launch("k_loud_energy");
        hipLaunchKernelGGL(k_loud_energy, dim3((unsigned)max_tiles, (unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
    }
    note_launch("k_loud_gate");
    hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)n), dim3(kDspLanes), 0, stream, rows_dev, scan);
}

}  // namespace ptts
