// gemm_tile.h -- the steps the many-row GEMM generations share (k_gemm in kernels.hip, k_gemm2, k_gemm3, k_gemm5, k_gemm_wres): tile order,
// fragment swizzle, the activation step, the scalar epilogue, and the host's operand conditions.  Why each generation exists, and what it
// does differently, is written in its own file.  Everything here is forced inline and was admitted only in a form that leaves every
// kernel's instructions as they were (profiles/mfma_refactor.txt, which also says why the pipelined fragment sweep of k_gemm5 and
// k_gemm_wres is still written out in both).
#pragma once

#include "kernels.h"
#include "device_util.h"
#include "mfma_util.h"

namespace ptts {

// ---- XCD-aware tile order ----
// Blocks are dealt round-robin to the 8 XCDs (each with a private L2), so block id b runs on XCD b % 8.  All column tiles of one row panel
// of A are given ids with the same b % 8 and consecutive b / 8: the panel is fetched from HBM once into that XCD's L2 instead of once per
// column tile.  (Speed only.)  The grid is padded to whole rounds of 8: a block whose panel is past the last one returns at once, and
// the column tile is asked for behind that check, where the kernels always had its division.
struct XcdTile {
    int pan, j;
    __device__ __forceinline__ int coltile(int ncol) const { return j % ncol; }
};
__device__ __forceinline__ XcdTile xcd_tile(int bid, int ncol) {
    const int xcd = bid & 7, j = bid >> 3;
    return {(j / ncol) * 8 + xcd, j};
}
static inline unsigned xcd_grid(int npan, int ncol) { return (unsigned)(((npan + 7) / 8) * 8 * ncol); }

// ---- fragment swizzle of a [column][32 k] bf16 weight image in LDS ----
// A weight column's 32 k (64 bytes = four 16-byte chunks) are stored with chunk c at c ^ frag_swz(column).  A ds_read_b128 is served
// in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: each group holds every fragment column once,
// columns 4..11 with the neighbouring k group; with this XOR its 16 lanes hit 16 different 16-byte bank slots (the plain layout was a
// 2-way conflict on every fragment read).
__device__ __forceinline__ int frag_swz(int col) { return ((col >> 3) & 1) * 3; }

// ---- activation step: 32 k of the wave's 32 rows, straight from memory into MFMA operands ----
// lane (r16 = lane & 15, g = lane >> 4) holds k 8 g .. 8 g + 7 of row r16 of each of the wave's two 16-row tiles: two float4 per tile.
// row[t]: the lane's row of tile t, at its k group.
__device__ __forceinline__ void a_step_load(const float* const (&row)[2], int ko, float4 (&dst)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
        dst[t][0] = *reinterpret_cast<const float4*>(row[t] + ko);
        dst[t][1] = *reinterpret_cast<const float4*>(row[t] + ko + 4);
    }
}
// The split of a step is mfma_util.h's split8 per tile, behind the ELU of the kernels that have one as a prologue.
__device__ __forceinline__ void elu_fast4(float4& v) { v.x = elu_fast(v.x); v.y = elu_fast(v.y); v.z = elu_fast(v.z); v.w = elu_fast(v.w); }

// ---- scalar epilogue of a 32 x 32 accumulator tile (k_gemm, k_gemm2) ----
// lane holds C[row = acc32_row(reg, lane)][col = lane & 31] of the tile
__device__ __forceinline__ int acc32_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
// the per-column operands of output column n
struct EpiCol {
    float bias, addv, scl;
};
__device__ __forceinline__ EpiCol epi_col(const GemmArgs& a, int n) {
    return {a.bias ? a.bias[n] : 0.0f, a.addvec ? a.addvec[n] : 0.0f, a.scale ? a.scale[n] : 1.0f};
}
// C[row()][n], at offset co, from v = its sum + bias (row: asked for by the gated form only)
template <class Row>
__device__ __forceinline__ float epi_scalar(const GemmArgs& a, const EpiCol& c, float v, int n, int64_t co, Row&& row) {
    switch (a.epi) {
        case EPI_NONE: break;
        case EPI_GELU: v = gelu1(v); break;
        case EPI_SILU: v = silu1(c.addv + v); break;
        case EPI_ELU: v = elu1(v); break;
        case EPI_RESADD: v = a.R[co] + v; break;
        case EPI_SCALE_RESADD: v = a.R[co] + c.scl * v; break;
        case EPI_GATE_RESADD: v = a.R[co] + a.gate[(int64_t)row() * a.ldg + n] * v; break;
        case EPI_AXPY: v = a.R[co] + a.alpha * v; break;
        case EPI_RESADD_ELU: v = elu1(a.R[co] + v); break;
    }
    return v;
}

// ---- host: what the 16-byte accesses of these kernels ask of the operands ----
// A and W always (kalign: 8 bf16 / 4 f32 per 16-byte weight piece); C where the kernel stores float4.
static inline bool gemm_c_aligned(const GemmArgs& a) { return aligned16(a.C) && a.cmap.ld % 4 == 0 && a.cmap.batch_stride % 4 == 0; }
static inline bool gemm_operands_aligned(const GemmArgs& a, int kalign, bool need_c16) {
    return aligned16(a.A) && a.amap.ld % 4 == 0 && a.amap.batch_stride % 4 == 0 && a.ldw % kalign == 0 && aligned16(a.W) &&
           (!need_c16 || gemm_c_aligned(a));
}

}  // namespace ptts
