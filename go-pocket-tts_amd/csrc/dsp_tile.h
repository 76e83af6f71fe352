// dsp_tile.h -- what the post-processing kernels share on the device (dsp.hip, compressor.hip, limiter.hip; scan_block.h has the grid and the
// host-and-device arithmetic): one wave per workgroup, workgroup blockIdx.x on tile blockIdx.x of its row, lane l on
// run l of the tile.  Device code only.
#pragma once
#include "compressor.h"
#include "scan_block.h"

namespace ptts {

// only a full tile that another one follows hands a state on (n: the row's samples)
__device__ __forceinline__ bool tile_hands_on(int64_t n) { return (int64_t)(blockIdx.x + 1) * kDspTile < n; }
// samples of the lane's run in a tile of cnt
__device__ __forceinline__ int run_count(int cnt) { return max(0, min(kDspRun, cnt - (int)threadIdx.x * kDspRun)); }

// src[0, cnt) -- a tile's samples in the row -- into tile[0, cnt) (LDS) and back; 16-byte accesses where the row's alignment allows
__device__ __forceinline__ void tile_load(const float* src, int cnt, float* tile) {
    const bool vec = ((uintptr_t)src & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(tile + q) = *reinterpret_cast<const float4*>(src + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) tile[q + u] = src[q + u];
    }
}
__device__ __forceinline__ void tile_store(float* dst, int cnt, const float* tile) {
    const bool vec = ((uintptr_t)dst & 15) == 0;
    for (int q = threadIdx.x * 4; q < cnt; q += kDspLanes * 4) {
        if (vec && q + 4 <= cnt) *reinterpret_cast<float4*>(dst + q) = *reinterpret_cast<const float4*>(tile + q);
        else for (int u = 0; u < 4 && q + u < cnt; u++) dst[q + u] = tile[q + u];
    }
}

// The (max, times) fold (compressor.h cmp_fold_p) over a tile's runs from state S: e[l] is run l's end state from zero (LDS, [kDspLanes],
// complete), rho_run the release's power kDspRun.  Every lane evaluates it alike (a broadcast read) and returns the state entering its own run;
// *behind receives the state behind the last run
__device__ __forceinline__ double fold_enter_max(double rho_run, const double* e, double S, double* behind) {
    const int l = threadIdx.x;
    double t = S, mine = S;
    for (int j = 0; j < kDspLanes; j++) {
        if (j == l) mine = t;
        t = cmp_fold_p(rho_run, t, e[j]);
    }
    *behind = t;
    return mine;
}

// A row of F >= 1 tiles with one state: S_f of every tile from the E_f (scan_E<1>, scan_S<1>), 64 tiles at a time, by every lane alike (lane 0
// stores); the state is carried from one group of 64 to the next.  Max: S_(f+1) = max(a_tile S_f, E_f), else a_tile S_f + E_f
// (scan_advance<1>).  ein: LDS, [kDspLanes]
template <bool Max>
__device__ __forceinline__ void carry_one(double a_tile, int64_t F, double* states, double* ein) {
    const int l = threadIdx.x;
    double s[1] = {0.0};   // the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < F - 1) ein[l] = scan_E<1>(states, f)[0];
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            if (l == 0) scan_S<1>(states, c0 + j)[0] = s[0];
            if (c0 + j < F - 1) {
                if (Max) s[0] = cmp_fold_p(a_tile, s[0], ein[j]);
                else scan_advance<1>(&a_tile, s, ein + j);
            }
        }
        __syncthreads();
    }
}

}  // namespace ptts
