/*
 * ptts_debug.h -- test and measurement hooks of the MI355X PocketTTS path.  NOT part of the drop-in ABI (include/ptts.h) and NOT exported by
 * libptts_hip.so: these entry points are compiled from csrc/capi_hooks.cpp into libptts_hooks.so, a small library that depends on libptts_hip.so and is
 * loaded beside it by tests/, tools/ and bench.py's measurement passes.  A host of the reference links libptts_hip.so alone and can
 * neither inject faults nor run micro-benchmarks through it.  The reference's own seam has nothing of the kind: internal/tts/runtime.go:42-45.
 */
#ifndef PTTS_DEBUG_H
#define PTTS_DEBUG_H

#include "ptts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pieces of one Mimi decoder-transformer layer on host rows, through the kernels the decoder itself launches for them (staged parity checks of
 * mimiTransformerLayer, mimi.go:245-441).  which = PTTS_MIMI_PIECE_QKV: norm1 -> in_proj -> RoPE of q and k at positions pos0 + (row % rows_per_seg)
 * (rows_per_seg 0: pos0 + row): x [rows, mimi_dim] -> out [rows, 3 mimi_dim] (q | k | v).  which = PTTS_MIMI_PIECE_FFN: x + layer_scale_2 *
 * linear2(gelu(linear1(norm2(x)))): x [rows, mimi_dim] -> out [rows, mimi_dim]. */
#define PTTS_MIMI_PIECE_QKV 0
#define PTTS_MIMI_PIECE_FFN 1
int  ptts_mimi_layer_piece(ptts_model* m, int32_t layer, int32_t which, const float* x, int64_t rows, int32_t pos0, int32_t rows_per_seg, float* out);

/* The same with one more observation point: transformer_out (optional) receives the decoder transformer's output, i.e. the
 * [n_utt, frames * steps_per_latent, mimi_dim] rows that MimiModel.DecodeFromLatent hands to the SEANet decoder after its
 * mimiTransformerLayer loop (mimi.go:733-748) -- the staged check of a17 (window attention, RoPE, layer_scale). */
int  ptts_decode_stages(ptts_model* m, const float* latents, int32_t n_utt, int32_t frames,
                        float* pcm, float* mimi_latent, float* transformer_out);

/* Staged observation of the Mimi encoder (ptts_mimi_encode; PARITY UNPINNED) on one clip: stages[i] (host, any may be NULL) receives, channels-last,
 *   0 head conv [L0, f]          1 elu(residual block 1) [L0, f]   2 down conv 1 [L1, 2f]   3 elu(residual block 2) [L1, 2f]
 *   4 down conv 2 [L2, 4f]        5 elu(residual block 3) [L2, 4f]  6 down conv 3 [L3, 8f]  7 tail conv [L3, 512]
 *   8 transformer output [L3, 512]  9 latent [frames, 512]
 * with L3 = 16 frames, L2 = 6 L3, L1 = 5 L2, L0 = 4 L1 at full size (the strides are the checkpoint's).  The residual stages are given after the ELU
 * that every reader applies (the sum itself is never stored).  shapes [10][2] receives every stage's (rows, channels); with stages NULL that is all
 * the call does. */
int  ptts_debug_encode_stages(ptts_model* m, const float* pcm, int64_t n_samples, float* const* stages, int64_t* shapes);

/* Kernel micro-benchmarks (tools/microbench.py; device-resident synthetic operands, HIP-event timing; not part of the
 * drop-in path).  ptts_debug_gemm also returns max |C_variant - C_other| between the two many-row GEMM kernels. */
int ptts_debug_time_skinny(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t splitk, int32_t fuse_ln, int32_t iters, float* avg_us);
int ptts_debug_skinny_stamps(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t splitk, int32_t fuse_ln, uint64_t* out /* [max_blocks][8] */,
                             int32_t max_blocks, int32_t* n_blocks);
int ptts_debug_step_stamps(ptts_batch* b, int32_t lsd_steps, uint64_t* out /* [cap_blocks][8] */, int64_t cap_blocks, int32_t* desc /* [cap_desc][8] */,
                           int32_t cap_desc, int32_t* n_desc);
int ptts_debug_gemm(int32_t M, int32_t N, int32_t K, int32_t w_bf16, int32_t variant, int32_t epi, int32_t iters, float* avg_us,
                    float* maxdiff);

/* The AR step's linears at 128+ rows (csrc/tall.hip) stand-alone on host operands: ONE launch of k_rowprep, ONE of k_tall, or the two chained.
 *   op PTTS_TALL_ROWPREP  launch_rowprep: x' = x + (((p_0 + p_1) + ...) + pbias) -> x_out; LayerNorm(x') (biased variance, affine ln_w / ln_b [K], eps) -> y_out
 *                         and its bf16 split yh / yl.  The row width D is K.
 *      PTTS_TALL_TALL     launch_tall_as: out = epi(x W^T + bias); x is split into its bf16 hi / lo planes [rows][lda] on the host the way the kernels split
 *      PTTS_TALL_BOTH     the first, then the second on yh / yl (lda must equal ldy)
 *   Every per-row buffer holds `rows` >= M rows; the launch is told of M.  Rows behind M and columns behind a width are there to be found unchanged.
 *   k_rowprep: x [rows][ldx]; planes [psplit][pstride] (a plane's rows dense [M][K]; pstride >= rows K; NULL with psplit 0: no pending sum, x_out is not
 *   written); pbias [K] or NULL; x_out, y_out [rows][K] f32 (want_x_out / want_y_out 0: the kernel is passed a null pointer); yh, yl [rows][ldy] bf16 bits.
 *   k_tall: W [N][K] f32 row-major, rounded to bf16 and packed by the loader's packer; bias [N] or NULL; R [rows][ldr] or NULL; epi 0 none, 1 GELU, 4 residual
 *   add (kernels.h Epi); form 0: tall_rows(M) picks as in production, 32 / 64: that block height.  The result leaves
 *     splitk > 1: as the planes out [splitk][zstride] (a plane's rows dense [M][N]; zstride >= rows N).  k_skinny's convention: with R, plane 0 =
 *                 R + (sums_0 + bias) and the others raw sums; without R every plane holds raw sums and a bias is refused (it would be dropped: it is the
 *                 consumer's through PendingSum::bias);
 *     ch != NULL: as bf16 bits ch / cl [rows][ldp] (the hi / lo planes the next product reads);
 *     otherwise:  as out [rows][ldc] f32.
 * Every result (out, ch, cl, x_out, y_out, yh, yl; any may be NULL where the form does not need it) is filled with 0xff bytes before the launch and returned whole.
 * form_out: the block height launched (0 for ROWPREP); grid [3]: the last launch's grid as the launcher's own functions give it (tall_grid / rowprep_blocks);
 * launched (launched_cap bytes): the census of the call ("kernel=count;"), empty after a refusal.
 * PTTS_EINVAL with a message, before anything is uploaded or launched -- no call can take an access outside these buffers:
 *   an unknown op; a form other than 0, 32, 64; M < 1, rows < M or rows > 1024; N or K outside [1, 8192]; a leading dimension below its width (ldx, ldy, lda < K;
 *   ldc, ldr, ldp < N); pstride < rows K; zstride < rows N; psplit outside [0, 16] or not matching planes; pbias without planes; splitk outside [1, 16];
 *   a null operand or result of the form; BOTH with lda != ldy; whatever rowprep_supported / tall_supported refuse. */
#define PTTS_TALL_ROWPREP 1
#define PTTS_TALL_TALL 2
#define PTTS_TALL_BOTH 3
typedef struct ptts_tall_args {
    int32_t op, M, rows, N, K, epi, splitk, form, psplit, want_x_out, want_y_out;
    float eps;
    int64_t ldx, ldy, lda, ldc, ldr, ldp, pstride, zstride, launched_cap;
    const float *x, *planes, *pbias, *ln_w, *ln_b, *W, *bias, *R;
    float *out, *x_out, *y_out;
    uint16_t *ch, *cl, *yh, *yl;
    int32_t *form_out, *grid;
    char* launched;
} ptts_tall_args;
int ptts_debug_tall(const ptts_tall_args* a);

/* The step linear (csrc/skinny.hip: k_skinny, the kernel every AR step spends its time in) stand-alone on host operands.  C = epi(prologue(x) W^T + bias):
 *   x [M][lda] (lda >= K), W [N][K] f32 row-major; wfmt 0: f32 weights, 1: rounded to bf16, 2: per-row int8 (w_eff [N][K] receives W^ = q s, w_scale [N] the
 *   row scales); the tiled copy the kernel streams is made by the packers the model loader uses.
 *   Epilogue: epi 0..8 (kernels.h Epi) with bias [N], addvec [N, or N - 1 with tail], R [M][ldc] (r_in_c: R is uploaded INTO C and the kernel runs with
 *   R == C), scale [N], gate [M][ldg], alpha; tail: the last column goes as acc + bias to tail_out [M] instead of C.
 *   splitk > 1: C receives the planes [splitk][zrows or M][N] (plane 0 = R + (sums + bias) when R is given, raw sums otherwise); zrows > 0 launches with
 *   GemmArgs::zstride = zrows N (the planes of a row chunk of a taller operand).  Otherwise C is [M][ldc].
 *   Fused prologue (splitk 1, lda == K): planes [psplit][M][K] (+ pbias [K]) are added to the rows in order -> x_out [M][K]; ln: LayerNorm (eps) with the
 *   optional affine ln_w / ln_b [K] and the optional modulation y (1 + mscale[m]) + shift[m] (rows [M][ldmod]) -> y_out [M][K]; pgate != 0 asks for the
 *   gated pending sum the kernel does not have (refused).
 *   path 0: launch_skinny; 1: launch_gemm (the <= 64-row hand-over and the 64-row chunks up to 256 rows; no split, no prologue).
 * C, tail_out, x_out and y_out are filled with 0xff bytes before the launch and returned whole (padding columns included).  launches [2] receives the
 * census of the call: k_skinny launches, all noted launches.  PTTS_EINVAL, before anything is launched, for whatever skinny_supported /
 * skinny_fuse_supported (or launch_gemm's hand-over condition) refuse. */
typedef struct ptts_step_linear_args {
    int32_t M, N, K, lda, ldc, wfmt, epi, splitk, tail, path, ldg, ln, ldmod, psplit, r_in_c, zrows, pgate, reserved;
    float alpha, eps;
    const float *x, *W, *bias, *addvec, *R, *scale, *gate, *ln_w, *ln_b, *shift, *mscale, *planes, *pbias;
    float *C, *tail_out, *x_out, *y_out, *w_eff, *w_scale;
    int32_t* launches;
} ptts_step_linear_args;
int ptts_debug_step_linear(const ptts_step_linear_args* a);

/* The code that opens and closes an AR step, stand-alone on host operands: ONE launcher call, built as step.cpp / batch.cpp build it.
 *   op PTTS_STEP_EDGE_BEGIN      launch_step_begin without the two 32-deep linears (k_step_begin)
 *      PTTS_STEP_EDGE_BEGIN_LIN  launch_step_begin with them: the launcher picks k_step_begin_mm (step_open_mfma_ok, even strides) or k_step_begin
 *      PTTS_STEP_EDGE_FINISH     launch_step_finish on `frame` (k_step_finish)
 *      PTTS_STEP_EDGE_FIN        launch_skinny with SkinnyFuse::fin: the flow net's final layer with the bookkeeping in its epilogue
 *      PTTS_STEP_EDGE_FIN_CHAIN  ... and SkinnyFuse::chain: the launch opens the next step as well
 *   Every per-row buffer and every state array holds `rows` >= B rows; the launch is told of B.  Rows behind B are there to be found unchanged.
 *   State, read and written back in place: kv_len, active, step, countdown, n_frames, eos_step, max_steps, frames_after_eos, broke [rows], eos_threshold
 *   [rows], n_active [1] (kernels.h StepState).
 *   latents [rows][lat_stride] (lat_stride >= S ldim; S frames per row), read and written back in place; noise [rows][noise_stride] or NULL (zeros);
 *   bos [ldim]; eos_logit [rows]; frame [rows][ldim] (FINISH).
 *   The 32-deep linears: w_in [d_in][ldim], w_pj [d_pj][ldim] row-major, f32 or -- lin_bf16 -- bf16 bits; b_in [d_in], b_pj [d_pj] or NULL.
 *   FIN / FIN_CHAIN: fx_in [rows][K]; W [N][K] f32 with bias [N] or NULL, packed by the loader's packers as wfmt says (0 f32, 1 bf16, 2 int8: w_eff [N][K]
 *   and w_scale [N] receive W^ and the row scales); shift, mscale [rows][ldmod]; LayerNorm without affine at eps; epilogue epi with alpha;
 *   cur [rows][N] is the residual AND the output (R == C, as step_flow passes it), read and written back in place.  N == ldim.
 *   FIN_CHAIN builds the StepFinish + StepChain record in device memory as the batch set-up does: the next step's x0 and fx are the OTHER copies (Batch::cur2,
 *   fx2), here the results x0 and fx -- a chained launch's blocks read cur and fx_in while one of them writes the next opening, so the two never alias.
 * Results, filled with 0xff bytes before the launch and returned whole: in32 [rows][ldim], x0 [rows][ldim], x [rows][d_in], fx [rows][d_pj] (NULL or unused
 * when the op has no linears).  launched (launched_cap bytes): the census of the call ("kernel=count;").
 * PTTS_EINVAL with a message, before anything is launched -- no call can take an access outside these buffers:
 *   an unknown op; ldim > 64 or ldim % 4 != 0; B outside [1, 256] or rows < B; S < 1; lat_stride < S ldim (noise_stride likewise with noise);
 *   a row below B without 0 <= step <= max_steps <= S, or active with step == max_steps; a null operand of the op;
 *   with linears: d_in or d_pj outside [1, 4096];  FIN / FIN_CHAIN: N != ldim, ldmod < K, wfmt outside 0..2, whatever skinny_fuse_supported refuses;
 *   FIN_CHAIN: whatever step_open_mfma_ok refuses, an odd lat_stride, lin_bf16 != (wfmt != 0) (the chained form takes the linears' type from the step
 *   kernel's weight type). */
#define PTTS_STEP_EDGE_BEGIN 0
#define PTTS_STEP_EDGE_BEGIN_LIN 1
#define PTTS_STEP_EDGE_FINISH 2
#define PTTS_STEP_EDGE_FIN 3
#define PTTS_STEP_EDGE_FIN_CHAIN 4
typedef struct ptts_step_edge_args {
    int32_t op, B, rows, S, ldim, d_in, d_pj, lin_bf16, N, K, wfmt, epi, ldmod, reserved;
    float alpha, eps;
    int64_t lat_stride, noise_stride, launched_cap;
    int32_t *kv_len, *active, *step, *countdown, *n_frames, *eos_step, *max_steps, *frames_after_eos, *broke, *n_active;
    float* eos_threshold;
    float* latents;
    const float *noise, *bos, *eos_logit, *frame;
    const void *w_in, *w_pj;
    const float *b_in, *b_pj;
    const float *fx_in, *W, *bias, *shift, *mscale;
    float* cur;
    float *in32, *x0, *x, *fx, *w_eff, *w_scale;
    char* launched;
} ptts_step_edge_args;
int ptts_debug_step_edge(const ptts_step_edge_args* a);

/* The step attention (csrc/attn_step.hip: k_attn_step, and k_attention behind it for caches beyond one burst) stand-alone: ONE launch_attention call with
 * AttnArgs filled as the AR step fills them (step.cpp step_core: fused_step, context -1, d_model = heads * 64, max_keys = cap), on host operands.
 *   qkv [rows][qkv_ld] (q | k | v, d_model each), cos_t / sin_t [cap][32], seg_len / active / pre_len / voice_of_row [rows];
 *   pre_k / pre_v [n_pre <= 4]: prefix buffers [layers][heads][pre_rows[i]][64] in the cache format (bf16 bits or f32); voice_of_row[r] names the buffer
 *   row r's prefix pointers are set to (-1: null pointers); the pre_k / pre_v / pre_len device arrays are always passed, as the step passes them;
 *   k, v [rows][heads][cap][64]: the rows' own caches of `layer` as raw bytes in the cache format, uploaded, and returned whole after the launch;
 *   out [rows][out_ld]: filled with 0xff bytes before the launch and returned whole.
 * kernel (kernel_cap bytes) receives the name launch_attention picked; info [4]: the load rounds the launch issues (attn_step_launch_rounds; 0 when another
 * kernel ran), all noted launches, k_attn_step launches, k_attention launches.
 * PTTS_EINVAL with a message, before anything is uploaded or launched, unless (these keep every access inside the buffers above):
 *   0 <= seg_len[r] < cap; pre_len[r] <= seg_len[r]; pre_len[r] is 0 or exactly pre_rows[voice_of_row[r]]; -1 <= voice_of_row[r] < n_pre;
 *   keys_now == 0 or seg_len[r] + 1 <= keys_now for every active row; qkv_ld >= 3 * heads * 64; out_ld >= heads * 64; 0 <= layer < layers;
 *   1 <= rows <= 1024, 1 <= heads <= 64, 1 <= cap <= 4096, 1 <= layers <= 64, pre_rows[i] >= 1. */
typedef struct ptts_attn_step_args {
    int32_t kv_bf16, heads, rows, layers, layer, cap, keys_now, n_pre;
    int64_t qkv_ld, out_ld, kernel_cap;
    const float *qkv, *cos_t, *sin_t;
    const int32_t *seg_len, *active, *pre_len, *voice_of_row;
    const void* pre_k[4];
    const void* pre_v[4];
    int32_t pre_rows[4];
    void *k, *v;
    float* out;
    char* kernel;
    int32_t* info;
} ptts_attn_step_args;
int ptts_debug_attn_step(const ptts_attn_step_args* a);
/* attn_step_rounds / attn_step_keys_per_round of csrc/attn_step.hip (no GPU): the load rounds for a launch bounded by `keys`, the keys one round covers. */
int ptts_debug_attn_step_rounds(int32_t keys, int32_t kv_bf16, int32_t* keys_per_round);

/* The window attention (csrc/attn_window.hip: k_attn_window, k_attn_window_lds) stand-alone: ONE launch on host operands, AttnArgs filled as the callers do.
 * Dense (ragged 0; mimi_decode.cpp mimi_range, encoder.cpp): qkv [segs][T1][ld] f32 holds q | k | v at columns 0, D, 2 D (D = heads * 64).  The chunk (t0, CT) is
 *   launched: q = qkv + t0 ld with q_rows_per_batch CT and q_batch_stride T1 ld; k / v = qkv + D / 2 D with k_seg_stride T1 ld, k_head_stride 64,
 *   k_row_stride ld; rows_per_seg CT, pos_base t0, context (> 0), rows = segs CT.
 * Ragged (ragged 1; batch.cpp's prompt prefill): qkv is the packed query rows [rows][ld]; k, v are caches [segs][heads][cap][64] as raw bytes (f32, or bf16
 *   bits with kv_bf16); rag_off [segs + 1] (rag_off[0] = 0, rag_off[segs] = rows), rag_pos0 [segs]; row_seg / row_pos are derived and passed as the prefill
 *   passes them; rows_per_seg = the longest segment; context: -1 as in production, or a window.
 * out [rows][out_ld] is filled with 0xff bytes before the launch and returned whole.
 * form 0: through launch_attention (the dispatch is under test); 1: k_attn_window<false, false>, or the ragged instance of the cache format; 2:
 * k_attn_window_lds<4> (dense only).  kernel (kernel_cap bytes) receives the name launch_attention picked (form 0) or the instance's; launched (launched_cap
 * bytes) the census of the call ("kernel=count;").
 * PTTS_EINVAL with a message, before anything is uploaded or launched, for whatever could take an access outside these buffers: ld < 3 D (ragged: < D) or
 * out_ld < D; ld or out_ld not a multiple of 4 (the kernels' 16-byte accesses: attn_window_supported); t0 < 0, CT < 1, t0 + CT > T1; a dense context < 1 or a
 * dense bf16 cache; rag_off not starting at 0, not non-decreasing or not ending at rows; rag_pos0[s] < 0 or rag_pos0[s] + n_s > cap; an unknown form or form 2
 * on ragged operands; sizes outside 1 <= rows <= 4096, heads <= 16, segs <= 16, cap / T1 <= 4096. */
typedef struct ptts_attn_window_args {
    int32_t form, ragged, kv_bf16, heads, segs, context, T1, t0, CT, cap, rows, reserved;
    int64_t ld, out_ld, kernel_cap, launched_cap;
    const float* qkv;
    const void *k, *v;
    const int32_t *rag_off, *rag_pos0;
    float* out;
    char *kernel, *launched;
} ptts_attn_window_args;
int ptts_debug_attn_window(const ptts_attn_window_args* a);

/* The many-row GEMMs (csrc/kernels.hip k_gemm, gemm2.hip, gemm3.hip, gemm_wres.hip, gemm5.hip) stand-alone: ONE launch of a named kernel on host operands.
 * C = epi(rope(aop(A) W^T + bias)) with kernels.h' RowMaps on A and C:
 *   A: a buffer of a_elems floats; row m starts at a_off + (m / a_rows_per_batch) a_batch_stride + (m % a_rows_per_batch) a_ld (a_rows_per_batch 0: a_off + m a_ld)
 *   and is K wide -- a_ld < K makes the rows overlap (a convolution's windows), a_off leaves history rows in front.
 *   W [N][ldw] f32 (ldw >= K); w_bf16: rounded to bf16 (nearest even) by the hook.  aop 0 / 1 (ELU on A), epi 0..8 (kernels.h Epi), alpha.
 *   C: a buffer of c_elems floats addressed the same way (c_off, c_ld, c_rows_per_batch, c_batch_stride), filled with 0xff bytes before the launch and
 *   returned whole.  R (c_elems floats, addressed like C) is the residual; r_in_c: R is uploaded INTO C and the kernel runs with R == C.
 *   bias [N], addvec [N], scale [N], gate [M][ldg]: each optional (a missing scale is 1).
 *   RoPE (interleaved pairs) on the first rope_cols columns: rope_cos / rope_sin [n_pos][rope_hd / 2]; row m sits at rope_row_pos[m] when given, else at
 *   rope_pos0 + (rope_rows_per_seg ? m % rope_rows_per_seg : m).
 *   Split-K: kslice > 0: plane z (k in [z kslice, (z + 1) kslice)) goes, as raw sums, to C + z zstride.  win_taps / win_c: GemmArgs' (k_gemm5's k order).
 *   kernel 0: what launch_gemm (launch_gemm_rope with tables) dispatches; 1 k_gemm (the shape must be one launch_gemm leaves to it); 2 k_gemm2; 3 k_gemm3 with
 *   cfg 0 (production) / 1 <.,4,64> / 2 <.,4,128> / 3 <.,8,64> / 6 <.,8,128> / 4 <256,8,64>; 4 k_gemm_wres with rgl row groups per XCD (0: production);
 *   5 k_gemm5 with cfg 0 (production) / 1 <256,8> / 2 <256,4> / 3 <128,8> / 4 <128,4>.
 * launched (launched_cap bytes) receives the census of the call ("kernel=count;"), info [2] the device's compute units and the rgl used (0: another kernel).
 * PTTS_EINVAL with a message, before anything is launched, for: what the chosen kernel's *_supported refuses; an unknown kernel or cfg, a 256-column form
 * with N not a multiple of 256 (k_gemm5 does not bound its weight loads), rgl outside [1, CUs / 8 (/ column tiles)]; RoPE, split-K on a kernel that has none;
 * what would be ignored: an rgl on another kernel than k_gemm_wres, a cfg on another than k_gemm3 / k_gemm5, a zstride without kslice;
 * a map whose rows (the K-wide reads, the N-wide stores and residual reads of every plane) leave a_elems / c_elems; a map of C whose rows, segments or planes
 * overlap (c_ld < N, c_batch_stride below a segment's extent, zstride below a plane's: two blocks would store to one element); a position outside [0, n_pos). */
typedef struct ptts_gemm_rows_args {
    int32_t M, N, K, ldw, w_bf16, aop, epi, kernel, cfg, rgl, r_in_c, ldg, rope_cols, rope_hd, rope_pos0, rope_rows_per_seg, n_pos, kslice, win_taps, win_c;
    float alpha;
    int32_t reserved;
    int64_t a_elems, a_ld, a_rows_per_batch, a_batch_stride, a_off, c_elems, c_ld, c_rows_per_batch, c_batch_stride, c_off, zstride, launched_cap;
    const float *A, *W, *bias, *addvec, *scale, *gate, *R, *rope_cos, *rope_sin;
    const int32_t* rope_row_pos;
    float* C;
    char* launched;
    int32_t* info;
} ptts_gemm_rows_args;
int ptts_debug_gemm_rows(const ptts_gemm_rows_args* a);

/* The fused SEANet blocks (csrc/resblock.hip: k_resblock; csrc/resblock_up.hip: k_resblock_up) stand-alone: ONE launch on host operands.
 *   u [B][pad + L][C]: `pad` history rows (zeros by the kernels' contract) and L rows per utterance; on the device every utterance gets `slack` more rows
 *   (u_bs = (pad + L + slack) C), filled with NaN.  Rows [t0, t1) are produced: uo [B][pad + L + slack][C] = elu(u + block(u)) (final_conv 0), or
 *   pcm [B][L] (final_conv 1), or -- rows [B][2] = {lim, s16} given -- utterance b's samples [0, min(lim, L, t1)) in its own 16-byte-aligned destination of
 *   row_bytes bytes (f32, or int16 by WritePCM16Samples' rule), returned in row_out [B][row_bytes]; pcm then stays untouched.
 *   Weights, f32 row-major in the checkpoint's GEMM layouts: w1 [H][3 C] (conv k3: [tap][c]), w2 [C][H] (conv k1), wf [3 C] (final conv), b1 [H], b2 [C],
 *   bf [1] (each optional); w_bf16: rounded to bf16, else hi + lo planes.  They are packed by the loader's own packers (csrc/model.h).
 *   fuse_up: u is not read; the block's input is the transposed convolution 128 -> 64, stride 4, of xin [B][x_pad + x_L][128] (x_slack NaN rows behind each
 *   utterance on the device) with wup [4 * 64][2 * 128] (row (phase r, channel): x[t-1] . W[.., r + 4] | x[t] . W[.., r]) and bup [64] (optional).
 *   form 0: the production choice (resblock_plan / resblock_up_plan, today's thresholds); 1: one tile per block; 2: `grid` persistent blocks.
 * uo, pcm and row_out are filled with 0xff bytes before the launch and returned whole.  launched [5] receives waves per block, persistent, grid, tiles
 * per utterance, new rows per tile.  PTTS_EINVAL with a message, before anything is launched, for: whatever resblock_supported / resblock_up_supported
 * refuse apart from the size threshold, a form the block does not have, and a persistent grid outside [1, B * tiles]. */
typedef struct ptts_resblock_args {
    int32_t B, L, t0, t1, C, H, pad, slack, w_bf16, final_conv, form, grid, fuse_up, x_pad, x_L, x_slack;
    const float *u, *w1, *w2, *wf, *b1, *b2, *bf, *xin, *wup, *bup;
    const int32_t* rows;
    float *uo, *pcm;
    uint8_t* row_out;
    int64_t row_bytes;
    int32_t* launched;
} ptts_resblock_args;
int ptts_debug_resblock(const ptts_resblock_args* a);
/* The launch form alone, for `cus` compute units (no GPU): out [5] as `launched` above; grid 0: the form does not exist / the fused kernel is not taken. */
int ptts_debug_resblock_plan(int32_t C, int32_t final_conv, int32_t w_bf16, int32_t fuse_up, int32_t B, int32_t rows, int32_t form, int32_t grid, int32_t cus,
                             int32_t* out);
/* The blocks' weight packers on a caller's matrix (no GPU).  kind 0: rm [out][in] -> fragment-ordered bf16 hi (and lo when given) planes of
 * out * in entries; 1: the fused transposed convolution's [256][in] operand (rows regrouped first); 2: the final convolution rm [in] as a one-column
 * matrix, hi and lo planes of 16 * in entries. */
int ptts_debug_seanet_pack(int32_t kind, const float* rm, int32_t out, int32_t in, uint16_t* hi, uint16_t* lo);
/* ... and what the model loader packed for a plan (no GPU): item 0-2 the blocks' conv k3, 3-5 their conv k1, 6 the last transposed convolution, 7 the
 * final convolution.  count receives the entries per plane (0: the loader made no such copy), dims {out, in, has lo plane}; hi / lo (cap entries each)
 * may be NULL to ask for the sizes only. */
int ptts_debug_plan_seanet_frags(ptts_plan* p, int32_t item, uint16_t* hi, uint16_t* lo, int64_t cap, int64_t* count, int32_t* dims);

/* name of the kernel the calling thread's last attention launch used ("k_attn_step", "k_attn_window", "k_attn_window<ragged>",
 * "k_attention"): lets a parity test assert that it exercised the kernel it means to */
const char* ptts_debug_last_attention_kernel(void);

/* Launch census of the calling thread: writes "kernel=count;..." of the launches noted since the previous call (truncated to
 * cap - 1 characters, returns the full length), clears it, and switches counting on (1) or off (0) from here on.  Calls that
 * run their launches on the calling thread (every entry point except the dispatcher's) are covered. */
int64_t ptts_debug_launch_counts(int32_t on, char* out, int64_t cap);
/* k_resample launches of the whole process since the last reset, on every thread (the launch census above sees the calling thread only, and the
 * continuous engine converts on the dispatcher's worker threads); reset != 0: returns the count and sets it to 0 */
int64_t ptts_debug_resample_launches(int32_t reset);

/* The DC block of ptts_dsp_apply in the blocked form the device kernels run (csrc/scan_block.h: runs of 30 samples from zero state, their end
 * states folded in run order, the frame tiles' states carried in frame order), evaluated on the host by the host instantiation of the very
 * functions the kernels call: n samples at 24 kHz, in -> out (in == out allowed).  No GPU. */
int ptts_debug_dsp_blocked_host(const float* in, int64_t n, float* out);

/* The causal chain over rows of host samples in windows, by the launches a streamed joined call runs (ptts_generate_joined_streamed): window j
 * covers [cuts[j-1], cuts[j]) of every row that reaches it (cuts: ascending multiples of 1920 above 0; behind the last cut one more window to each
 * row's end); a row is open in a window when it has samples behind the window's end.  State is carried between windows on the device.  out[i]:
 * n[i] floats (out[i] == in[i] allowed): the bits of ptts_dsp_rows on the same rows and options.  PTTS_EINVAL for a stage that is not causal
 * (normalize, the true-peak ceiling, the limiter: as the streamed call words it), a cut off the grid, and a cut c < n[i] with c > n[i] - Fo,
 * Fo = (int64)(fade_out_ms / 1000 * 24000) (it would deliver part of row i's fade out), naming row and cut. */
int ptts_debug_dsp_windows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, const ptts_dsp_opts* opts,
                           const int64_t* cuts, int32_t n_cuts, float* const* out);

/* Loudness (ptts_loudness; csrc/scan_block.h): the energies of the rows' whole 480-sample sub-blocks -- out[i] receives n[i] / 480 doubles, the
 * sums of squares of the K-weighted samples -- as the device kernels of a request's `loudness` compute them (m != NULL), or by the host
 * instantiation of the functions those kernels call (m == NULL, no GPU).  Twenty of them in order, over 9600, are one 400 ms block. */
int ptts_debug_loudness_energies(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, double* const* out);
/* The K-weighting sections as ptts_loudness derives them for a sample rate: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2.  No GPU. */
int ptts_debug_kweighting(int32_t sample_rate, double out[10]);

/* Test hook for the bounded hand-offs of k_flow_cluster (csrc/flow_cluster.hip): the model's NEXT plain-launched AR step runs the flow net's residual
 * blocks with one workgroup withholding what it should publish for block `block` (1-based; 0 clears).  Its peers' sweeps give up after their bound, the
 * launch runs to its end, and the call that contained the step fails with PTTS_ENODEVICE ("hand-off timed out"); the exchange state is cleared, the next
 * call is clean.  Nothing in the product sets it. */
int ptts_debug_flow_cluster_inject(ptts_model* m, int32_t block);

/* k_flow_cluster (csrc/flow_cluster.hip) stand-alone on host operands: a sequence of launches, FlowClusterArgs filled as step.cpp step_flow fills them.
 *   fx [rows][512]; ada [rows][ldmod]: block r's shift | scale | gate at columns 3 r 512; ln_w, ln_b, b0, b2 [depth][512]; eps [depth];
 *   w0, w2 [depth][512][512] f32 row-major, rounded to bf16 and tiled by the loader's pack_step_tiled.
 *   launch_rows [n_launch]: the launches run one after another on ONE granule buffer and ONE set of tag words -- both zeroed as the batch set-up zeroes them,
 *   then all 22 tiles' tag words set to tag_base0.  Launch i runs on its own device copy of fx's first launch_rows[i] rows (0xff bytes behind them);
 *   in_place 1: fx_out == fx_in (production); 0: a separate output, and fx_back [n_launch][rows][512] receives the input copies after the launches.
 *   On the device fx, the outputs and ada carry 3 slack rows of 0xff bytes behind `rows`.
 *   out [n_launch][rows][512]: filled with 0xff bytes before the launches and returned whole; state [23]: the 22 tag words and the fault word after the
 *   sequence; launched (launched_cap bytes): the census of the call ("kernel=count;").
 * If a launch leaves the fault word set, nothing more is launched and -- out, state and the census delivered -- the call fails with PTTS_ENODEVICE ("hand-off
 * timed out"); nothing is retried.  The hook has no way to set FlowClusterArgs::inject or ::stamps.
 * PTTS_EINVAL with a message, before a device is asked for: rows outside [1, 264]; depth outside [1, 8]; ldmod % 4 != 0, ldmod < 3 depth 512 or ldmod > 65536;
 * n_launch outside [1, 8]; a launch_rows entry outside [1, rows]; an odd tag_base0 (a launch's base is even: h tags are odd, x tags even); in_place not 0 / 1; a
 * null operand (fx_back only with in_place 0; launched may be null).  With a device: a grid that is not resident at once (flow_cluster_fits) and whatever
 * flow_cluster_supported refuses. */
typedef struct ptts_flow_cluster_args {
    int32_t rows, depth, n_launch, in_place;
    uint32_t tag_base0;
    int32_t reserved;
    int64_t ldmod, launched_cap;
    const float *fx, *ada, *ln_w, *ln_b, *b0, *b2, *eps, *w0, *w2;
    const int32_t* launch_rows;
    float *out, *fx_back;
    uint32_t* state;
    char* launched;
} ptts_flow_cluster_args;
int ptts_debug_flow_cluster(const ptts_flow_cluster_args* a);

/* The two kernels of csrc/ffn_fused.hip stand-alone: ONE launch on host operands.
 *   kind 0, k_mimi_ffn: x += ls * linear2(gelu(linear1(LayerNorm(x)))) in place; kind 1, k_mimi_rowlin: y = rope(LayerNorm(x) W1^T).
 *   x: a buffer of x_elems floats; row m starts at x_off + (m / x_rows_per_batch) x_batch_stride + (m % x_rows_per_batch) x_ld (x_rows_per_batch 0:
 *   x_off + m x_ld) and is D wide.  ln_w, ln_b [D], eps.  w1 [F][D] (kind 1: [N][D], N in the field F), w2 [D][F] (kind 0 only): f32 row-major, rounded to
 *   bf16 and laid out by the loader's packers (csrc/model.h pack_ffn_image / pack_w1_image).  ls [D] or NULL (kind 0); on the device it starts ls_off
 *   elements into its allocation (0: aligned as the loader aligns it).
 *   kind 1: y, a buffer of y_elems floats addressed like x (y_off, y_ld, ...), N wide rows; rope_cos / rope_sin [n_pos][32] or both NULL; the first
 *   rope_cols columns are rotated (interleaved pairs, 64-wide heads) at position pos0 + (rows_per_seg ? m % rows_per_seg : m).
 * kind 0 returns the whole x buffer after the launch in `out` (x_elems floats); kind 1 fills y with 0xff bytes before the launch and returns it whole in
 * `out` (y_elems floats).  launched (launched_cap bytes) receives the census of the call ("kernel=count;").
 * PTTS_EINVAL with a message, before anything is uploaded or launched, for: a row of either map that leaves its buffer; rows of x (kind 0) or of y that
 * overlap; a position outside [0, n_pos) (the kernels clamp rows, they do not bound table reads); one table without the other; and whatever
 * mimi_ffn_supported / mimi_rowlin_supported refuse (D != 512, F % 32, N % 64, ld / batch_stride / off % 4, a misaligned ls, rope_cols % 64 or > N). */
typedef struct ptts_mimi_fused_args {
    int32_t kind, M, D, F, n_pos, rope_cols, pos0, rows_per_seg, ls_off, reserved;
    float eps, reserved_f;
    int64_t x_elems, x_ld, x_rows_per_batch, x_batch_stride, x_off, y_elems, y_ld, y_rows_per_batch, y_batch_stride, y_off, launched_cap;
    const float *x, *ln_w, *ln_b, *w1, *w2, *ls, *rope_cos, *rope_sin;
    float* out;
    char* launched;
} ptts_mimi_fused_args;
int ptts_debug_mimi_fused(const ptts_mimi_fused_args* a);
/* The packers of those kernels' weight images on a caller's matrices (no GPU).  kind 0: w1 [n][512], w2 [512][n] -> n / 32 chunks of 64 KB (k_mimi_ffn);
 * kind 1: w1 [n][512] -> n / 32 images of 32 KB (k_mimi_rowlin; w2 unused).  dst: n * 1024 (kind 0) or n * 512 (kind 1) uint16.  n % 32 == 0. */
int ptts_debug_mimi_pack(int32_t kind, const float* w1, const float* w2, int32_t n, uint16_t* dst);

/* The check every entry point runs on a ptts_dsp_opts, without a model: out (cap bytes, terminated) receives its message, empty when the options are
 * fine; returns the message's length.  No GPU. */
int64_t ptts_debug_dsp_opts_error(const ptts_dsp_opts* opts, char* out, int64_t cap);
/* The true-peak meter's taps (ptts_true_peak; csrc/true_peak.h): out [8][54] receives h[p][k] as f32, *L the phases (8), *K the taps per phase
 * (54), *dlo the input offset of tap 0 (-26).  Any pointer may be NULL.  No GPU. */
int ptts_debug_true_peak_taps(float* out /* [8][54] */, int32_t* L, int32_t* K, int32_t* dlo);
/* ... and its oversampled signal on the host: y [8 n] receives y[8 i + p] of ptts_true_peak's definition for samples [n].  No GPU. */
int ptts_debug_true_peak_oversample(const float* samples, int64_t n, float* y /* [8 n] */);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_DEBUG_H */
