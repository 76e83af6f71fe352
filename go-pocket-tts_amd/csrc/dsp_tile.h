// dsp_tile.h -- what the post-processing kernels share on the device (dsp.hip, compressor.hip, deesser.hip, limiter.hip; scan_block.h has the grid and the
// host-and-device arithmetic): one wave per workgroup, workgroup blockIdx.x on tile blockIdx.x of its row, lane l on
// run l of the tile.  Device code only.
#pragma once
#include "compressor.h"
#include "scan_block.h"

namespace ptts {

// A launch covers a window of a row: tiles [t0, ceil(n / kDspTile)) of the row's own grid, n the samples up to the window's end; workgroup
// blockIdx.x is on tile t0 + blockIdx.x and on entry blockIdx.x of the window's per-tile states.  The row is open when more samples will follow
// behind n (n is then a multiple of kDspTile).  The one-shot chain is the window t0 = 0 of a closed row.
// only a full tile that another one follows hands a state on: in a closed row every tile but the last, in an open one the last as well
__device__ __forceinline__ bool tile_hands_on(int64_t t0, int64_t n, bool open) { return (t0 + blockIdx.x + 1) * kDspTile < n + (open ? 1 : 0); }
// of a window's F tiles, those that hand a state on (the first ones)
__device__ __forceinline__ int64_t win_hands(int64_t F, bool open) { return open ? F : F - 1; }
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

// The linear fold with one state (scan_advance<1>, t <- alpha^30 t + e_l) over a tile's runs from state S, shaped like fold_enter_max: the
// attack smoothing's, in compressor.hip and deesser.hip
__device__ __forceinline__ double fold_enter_sum(double alpha_run, const double* e, double S, double* behind) {
    const int l = threadIdx.x;
    double t[1] = {S}, mine = S;
    for (int j = 0; j < kDspLanes; j++) {
        if (j == l) mine = t[0];
        scan_advance<1>(&alpha_run, t, e + j);
    }
    *behind = t[0];
    return mine;
}

// A window of F >= 1 tiles with one state: S_f of every tile from the E_f (scan_E<1>, scan_S<1>), 64 tiles at a time, by every lane alike (lane 0
// stores); the state is carried from one group of 64 to the next.  Max: S_(f+1) = max(a_tile S_f, E_f), else a_tile S_f + E_f
// (scan_advance<1>).  ein: LDS, [kDspLanes].  carry (null: the row starts here from state 0 and ends here): the state the window in front left;
// an open window leaves the state behind its last tile there
template <bool Max>
__device__ __forceinline__ void carry_one(double a_tile, int64_t F, double* states, double* ein, double* carry, bool open) {
    const int l = threadIdx.x;
    const int64_t hands = win_hands(F, open);
    double s[1] = {carry ? *carry : 0.0};   // the state entering tile c0 + j
    for (int64_t c0 = 0; c0 < F; c0 += kDspLanes) {
        const int64_t f = c0 + l;
        if (f < hands) ein[l] = scan_E<1>(states, f)[0];
        __syncthreads();
        const int m = (int)min((int64_t)kDspLanes, F - c0);
        for (int j = 0; j < m; j++) {
            if (l == 0) scan_S<1>(states, c0 + j)[0] = s[0];
            if (c0 + j < hands) {
                if (Max) s[0] = cmp_fold_p(a_tile, s[0], ein[j]);
                else scan_advance<1>(&a_tile, s, ein + j);
            }
        }
        __syncthreads();
    }
    if (open && l == 0) *carry = s[0];
}

}  // namespace ptts
