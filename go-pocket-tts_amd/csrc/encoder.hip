// encoder.hip -- the two pieces of the Mimi encoder (runtime encoder.cpp) that no decoder kernel covers.  PARITY UNPINNED: the reference has no
// native encoder (mimi.go:14,791-794); the chain is inferred from the decoder.
//   k_enc_head        the 1-channel input convolution (K = 7 taps: no product worth a matrix core), PCM -> channels-last rows
//   k_enc_ds_partial  the downsample convolution at the frame rate: a few rows (12.5 per second of audio) against a 16384-deep weight, so
//   k_enc_ds_reduce   split-K -- every block sums its own k slice into a plane, and one pass adds the planes in slice order (deterministic)
// Both compute in f32 on the vector ALUs with f32 accumulation (bf16 weights are widened exactly), which is at least as accurate as the decoder's
// bf16 hi/lo split products.  No MFMA is issued here.
#include <algorithm>

#include "kernels.h"
#include "device_util.h"

namespace ptts {

namespace {

__device__ __forceinline__ float wload(const void* w, int64_t i, int bf16) {
    if (bf16) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(w)[i] << 16);
    return reinterpret_cast<const float*>(w)[i];
}

// out[t][c] = b[c] + sum_x w[c][x] * pcm[t + x]   (pcm: k - 1 zero history samples in front of sample 0)
__global__ void k_enc_head(const float* __restrict__ pcm, const void* __restrict__ w, int w_bf16, const float* __restrict__ b, int64_t L, int C, int k,
                           float* __restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L * C) return;
    const int64_t t = i / C;
    const int c = (int)(i % C);
    float acc = b ? b[c] : 0.0f;
    for (int x = 0; x < k; x++) acc = fmaf(wload(w, (int64_t)c * k + x, w_bf16), pcm[t + x], acc);
    out[t * ldo + c] = acc;
}

constexpr int DS_ROWS = 32, DS_COLS = 64, DS_KC = 64;

// partial[z][m][n] = sum over k in [z kslice, min(K, (z+1) kslice)) of A[m * lda + k] * W[n * K + k]; a block owns 32 rows x 64 columns.
// A chunk is staged transposed (As[k][row]: a thread's 8 rows are two broadcast b128 reads), W as Ws[col][k] with one word of padding
// (the 64 lanes of a wave read 64 different banks).
__global__ void __launch_bounds__(256) k_enc_ds_partial(const float* __restrict__ A, int64_t lda, const void* __restrict__ W, int w_bf16,
                                                        int M, int N, int K, int kslice, float* __restrict__ partial) {
    __shared__ float As[DS_KC][DS_ROWS];
    __shared__ float Ws[DS_COLS][DS_KC + 1];
    const int tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
    const int n0 = blockIdx.x * DS_COLS, m0 = blockIdx.y * DS_ROWS, z = blockIdx.z;
    const int k_lo = z * kslice, k_hi = min(K, k_lo + kslice);
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0.0f;
    for (int k0 = k_lo; k0 < k_hi; k0 += DS_KC) {
#pragma unroll
        for (int i = 0; i < DS_ROWS * DS_KC / 256; i++) {
            const int e = tid + 256 * i, r = e / DS_KC, kk = e % DS_KC;
            As[kk][r] = (m0 + r < M && k0 + kk < k_hi) ? A[(int64_t)(m0 + r) * lda + k0 + kk] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < DS_COLS * DS_KC / 256; i++) {
            const int e = tid + 256 * i, c = e / DS_KC, kk = e % DS_KC;
            Ws[c][kk] = (n0 + c < N && k0 + kk < k_hi) ? wload(W, (int64_t)(n0 + c) * K + k0 + kk, w_bf16) : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < DS_KC; kk++) {
            const float wv = Ws[lane][kk];
            const float4 a0 = *reinterpret_cast<const float4*>(&As[kk][rg * 8]);
            const float4 a1 = *reinterpret_cast<const float4*>(&As[kk][rg * 8 + 4]);
            acc[0] = fmaf(a0.x, wv, acc[0]); acc[1] = fmaf(a0.y, wv, acc[1]);
            acc[2] = fmaf(a0.z, wv, acc[2]); acc[3] = fmaf(a0.w, wv, acc[3]);
            acc[4] = fmaf(a1.x, wv, acc[4]); acc[5] = fmaf(a1.y, wv, acc[5]);
            acc[6] = fmaf(a1.z, wv, acc[6]); acc[7] = fmaf(a1.w, wv, acc[7]);
        }
        __syncthreads();
    }
    const int n = n0 + lane;
    if (n >= N) return;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int m = m0 + rg * 8 + i;
        if (m < M) partial[((int64_t)z * M + m) * N + n] = acc[i];
    }
}

// out[m][n] = bias[n] + partial[0][m][n] + partial[1][m][n] + ...   (planes added in slice order)
__global__ void k_enc_ds_reduce(const float* __restrict__ partial, int splits, int M, int N, const float* __restrict__ bias, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t mn = (int64_t)M * N;
    if (i >= mn) return;
    float s = partial[i];
    for (int z = 1; z < splits; z++) s += partial[(int64_t)z * mn + i];
    out[i] = bias ? s + bias[i % N] : s;
}

}  // namespace

void launch_enc_head(const float* pcm, const void* w, int w_bf16, const float* b, int64_t L, int C, int k, float* out, int64_t ldo, hipStream_t stream) {
    if (L <= 0) return;
    note_launch("k_enc_head");
    const int64_t n = L * C;
    hipLaunchKernelGGL(k_enc_head, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pcm, w, w_bf16, b, L, C, k, out, ldo);
}

int enc_ds_splits(int M, int N, int K) {
    const int tiles = ((N + DS_COLS - 1) / DS_COLS) * ((M + DS_ROWS - 1) / DS_ROWS);
    if (tiles <= 0) return 1;
    const int chunks = (K + DS_KC - 1) / DS_KC;
    const int want = std::max(1, std::min(chunks, (1024 + tiles - 1) / tiles));   // ~4 blocks per CU
    const int per = (chunks + want - 1) / want;
    return (chunks + per - 1) / per;
}

void launch_enc_downsample(const float* A, int64_t lda, const void* W, int w_bf16, const float* bias, int M, int N, int K, float* partial, float* out,
                           hipStream_t stream) {
    if (M <= 0) return;
    const int splits = enc_ds_splits(M, N, K);
    const int chunks = (K + DS_KC - 1) / DS_KC, kslice = ((chunks + splits - 1) / splits) * DS_KC;
    note_launch("k_enc_ds_partial");
    dim3 grid((unsigned)((N + DS_COLS - 1) / DS_COLS), (unsigned)((M + DS_ROWS - 1) / DS_ROWS), (unsigned)splits);
    hipLaunchKernelGGL(k_enc_ds_partial, grid, dim3(256), 0, stream, A, lda, W, w_bf16, M, N, K, kslice, partial);
    note_launch("k_enc_ds_reduce");
    const int64_t mn = (int64_t)M * N;
    hipLaunchKernelGGL(k_enc_ds_reduce, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, stream, partial, splits, M, N, bias, out);
}

}  // namespace ptts
