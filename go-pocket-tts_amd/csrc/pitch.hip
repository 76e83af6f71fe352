// pitch.hip -- the resampling step of the pitch of the parts of a joined text on ragged rows of 24 kHz audio, from one buffer into another, behind
// the trim and in front of the tempo (kernels.h PitchRow; pitch.h has the rule, pitch.cpp is the host statement and gives the bits; DESIGN.md
// section 8, N3).
//
//   k_pitch_resample   workgroup (x, y) of 512 threads on tile x (kPitchTile outputs) of row y; a row's pitch (p, D, g) is its design, so one launch
//                      serves rows of different pitches.  The workgroup stages in LDS: the prototype table as {h, hd} pairs (one 8-byte read a tap;
//                      entry q lies at q + q / 32, see below), the tile's input window (at most 2 x tile + 106 floats, zeros outside the row) and
//                      the row's D values of (float)r / (float)D (__fdiv_rn: the bits of the host's division; a tap looks its fraction up).
//                      Thread t then computes outputs t and t + 512 of the tile, each over its inputs in ascending order.  a * R moves by the
//                      constant 1000 R from tap to tap, so its quotient and remainder by D are carried with a subtraction and a compare from one
//                      unsigned 32-bit division per output, as the floor pair (qf, rf) of the SIGNED (c - 1000 i) R: behind the centre, where
//                      that is negative, |.|'s pair is (-qf, 0) or (-qf - 1, D - rf).
//                      LDS banking: an 8-byte entry takes two of the 64 banks and a half wave reads conflict-free when its 32 entries differ
//                      mod 32.  Neighbouring outputs' entries at one tap lie a multiple of 128 apart at p = 500 and of 256 wherever two lanes
//                      share an input: one bank for all.  The image skips one entry in 32, so entries k * 32 apart land k bank pairs apart.
// Nothing is atomic and nothing is cleared beforehand; every output sample is written once, by one thread; nothing outside [0, n) is read and
// nothing at or beyond n_out is written.  Sample indices are 64-bit.  The two fused multiply-adds of a tap are written as such and the gain is
// one product; contraction is switched off around them.
#include "device_util.h"
#include "kernels.h"
#include "pitch.h"

namespace ptts {

namespace {

static_assert(kPitchWindow >= 2 * kPitchTile + 106, "a tile's inputs at p = 2000: 2 (tile - 1) + 160 D / 3000 + 1, rounded up");
static_assert(kPitchTile % kPitchThreads == 0, "every thread has the same number of outputs in a full tile");

__global__ __launch_bounds__(kPitchThreads) void k_pitch_resample(const PitchRow* __restrict__ rows, const PitchScan* __restrict__ designs,
                                                                  const float2* __restrict__ image) {
    __shared__ __attribute__((aligned(16))) float2 tab[kPitchImage];
    __shared__ float win[kPitchWindow];
    __shared__ float fracs[2000];
    const PitchRow r = rows[blockIdx.y];
    const int64_t j0 = (int64_t)blockIdx.x * kPitchTile;
    if (j0 >= r.n_out) return;   // (the same for the whole workgroup)
    const PitchScan d = designs[r.design];
    const int D = d.D;
    const int t = threadIdx.x;
    const int cnt = (int)min((int64_t)kPitchTile, r.n_out - j0);
    const int64_t w0 = pitch_first(j0 * d.p, D);
    const int wlen = (int)min((int64_t)kPitchWindow, pitch_last((j0 + cnt - 1) * d.p, D) - w0 + 1);
    for (int i = t; i < kPitchImage; i += kPitchThreads) tab[i] = image[i];
    for (int i = t; i < wlen; i += kPitchThreads) {
        const int64_t at = w0 + i;
        win[i] = at >= 0 && at < r.n ? r.src[at] : 0.0f;
    }
    const float fD = (float)D;
    for (int i = t; i < D; i += kPitchThreads) fracs[i] = __fdiv_rn((float)i, fD);
    __syncthreads();
    const int dq = 1000 * kPitchR / D, dr = 1000 * kPitchR % D;
    for (int k = t; k < cnt; k += kPitchThreads) {
#pragma clang fp contract(off)
        const int64_t c = (j0 + k) * d.p;
        const int64_t i0 = pitch_first(c, D);
        const int taps = (int)(pitch_last(c, D) - i0) + 1;
        const float* const w = win + (int)(i0 - w0);
        const uint32_t u = (uint32_t)(c - 1000 * i0) * (uint32_t)kPitchR;   // (positive: the support's first input lies in front of c)
        int qf = (int)(u / (uint32_t)D), rf = (int)(u - (uint32_t)qf * (uint32_t)D);
        float acc = 0.0f;
        // (unrolled: the LDS reads of four taps are in flight together; only acc runs through them in order)
#pragma unroll 4
        for (int i = 0; i < taps; i++) {
            int q = qf, rr = rf;
            if (qf < 0) {
                q = rf ? -qf - 1 : -qf;
                rr = rf ? D - rf : 0;
            }
            const float2 e = tab[pitch_image_at(q)];
            const float coef = __builtin_fmaf(e.y, fracs[rr], e.x);
            acc = __builtin_fmaf(w[i], coef, acc);
            qf -= dq;
            rf -= dr;
            if (rf < 0) { rf += D; qf -= 1; }
        }
        r.dst[j0 + k] = acc * d.g;
    }
}

}  // namespace

void launch_pitch(const PitchRow* rows_dev, int n, int max_tiles, const PitchScan* designs_dev, const float* image_dev, hipStream_t stream) {
    if (n <= 0 || max_tiles <= 0) return;   // empty rows only: no sample
    note_launch("k_pitch_resample");
    hipLaunchKernelGGL(k_pitch_resample, dim3((unsigned)max_tiles, (unsigned)n), dim3(kPitchThreads), 0, stream, rows_dev, designs_dev,
                       reinterpret_cast<const float2*>(image_dev));
}

}  // namespace ptts
