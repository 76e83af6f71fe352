// kernels.h -- launchers of the hand-written gfx950 kernels (kernels.hip).
// All pointers are device pointers; every launcher enqueues on `stream` and returns.
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "deesser.h"
#include "limiter.h"
#include "pitch.h"
#include "tempo.h"
#include "trim.h"

namespace ptts {

// Rows of a 2-D operand may live in per-utterance segments (channels-last sequences with
// zero "history" rows in front of each utterance): row r is at
//   base + (r / rows_per_batch) * batch_stride + (r % rows_per_batch) * ld      (elements)
// rows_per_batch == 0 means one flat segment (base + r * ld).
struct RowMap {
    int64_t ld = 0;
    int64_t rows_per_batch = 0;
    int64_t batch_stride = 0;
};

enum AOp : int { AOP_NONE = 0, AOP_ELU = 1 };
enum Epi : int {
    EPI_NONE = 0,        // C = acc + bias
    EPI_GELU,            // C = gelu_erf(acc + bias)                     tensor_util.go:84-94
    EPI_SILU,            // C = silu(addvec + (acc + bias))              tensor_util.go:73-82
    EPI_ELU,             // C = elu(acc + bias)                          tensor_util.go:119-128
    EPI_RESADD,          // C = R + (acc + bias)
    EPI_SCALE_RESADD,    // C = R + scale[n] * (acc + bias)              mimi.go:275-285,351-358
    EPI_GATE_RESADD,     // C = R + gate[m, n] * (acc + bias)            flow_net.go:166-171
    EPI_AXPY,            // C = R + alpha * (acc + bias)                 flow_lm.go:346-349
    EPI_RESADD_ELU,      // C = elu(R + (acc + bias))   SEANet residual sum whose every reader applies ELU first (mimi.go:146-164,752-783)
};

struct GemmArgs {
    // C[M, N] = epi( aop(A)[M, K] * W[N, K]^T )
    const float* A = nullptr; RowMap amap;
    const void*  W = nullptr; int w_bf16 = 0; int64_t ldw = 0;
    const void*  Wt = nullptr;       // fragment-ordered copy of W for the AR-step kernel (model.cpp add_tiled), optional
    int wt_i8 = 0; const float* wscale = nullptr;   // Wt holds per-row-scaled int8 (PTTS_WEIGHTS_INT8); wscale: [N] row scales
    const float* bias = nullptr;     // [N] or null
    const float* addvec = nullptr;   // [N] or null (EPI_SILU only)
    float*       C = nullptr; RowMap cmap;
    const float* R = nullptr;        // residual, addressed like C
    const float* scale = nullptr;    // [N]
    const float* gate = nullptr; int64_t ldg = 0;
    float alpha = 1.0f;
    // k_gemm3 only: interleaved-pair RoPE (rope.go:81-105) applied to the first rope_cols output columns before they are
    // stored (q and k of a qkv projection); row m sits at position rope_pos0 + m % rope_rows_per_seg (0: m)
    const float* rope_cos = nullptr; const float* rope_sin = nullptr; int rope_cols = 0, rope_hd = 64, rope_pos0 = 0, rope_rows_per_seg = 0;
    const int32_t* rope_row_pos = nullptr;   // if set: the position of row m is rope_row_pos[m] (ragged prompt rows)
    // k_gemm3 only: split-K.  kslice > 0: ceil(K / kslice) blocks share an output tile, block z multiplies k in
    // [z kslice, (z+1) kslice) and stores its raw sums at C + z * zstride (no bias, no epilogue: the consumer adds the planes)
    int kslice = 0; int64_t zstride = 0;
    // k_gemm5 only: A's rows are the overlapping windows of a causal convolution (K = win_taps x win_c, row stride win_c): walk k channel-block-major
    // (speed only: the taps' reads of one input line then follow each other; gemm5.hip)
    int win_taps = 0, win_c = 0;
    float* tail = nullptr;           // k_skinny only: the LAST column goes, as acc + bias without the epilogue, to tail[m] instead of C
    int M = 0, N = 0, K = 0;
    int aop = AOP_NONE, epi = EPI_NONE;
};
constexpr int kStepMaxRows = 256;       // rows (utterances) one AR step takes: the step kernels' grids grow by row tiles, the flow-net cluster by 12-row tiles
constexpr int kSkinnyChunkRows = 256;   // up to this many rows a GEMM on a step matrix runs as 64-row chunks of the step kernel (launch_gemm)
void launch_gemm(const GemmArgs& a, hipStream_t stream);
bool launch_gemm_rope(const GemmArgs& a, hipStream_t stream);   // a product with the RoPE epilogue (GemmArgs::rope_cos) on k_gemm3; false: the shape is not taken (the caller rotates in a second launch)
bool gemm_wres_supported(const GemmArgs& a);   // gemm_wres.hip: K, N <= 256 with the whole weight matrix resident in LDS
void launch_gemm_wres(const GemmArgs& a, hipStream_t stream);   // = launch_gemm_wres_as(a, gemm_wres_rgl(a))
// its launch form: 8 * rgl (* column tiles) blocks, rgl row groups per XCD, every wave walking the 32-row panels (group, wave) + j * 64 rgl.  gemm_wres_rgl is
// the only place that chooses for production; another rgl in [1, gemm_wres_max_rgl] is for the kernel's test hook
int gemm_wres_max_rgl(const GemmArgs& a);   // CUs / 8 (256 x 256), CUs / 8 / column tiles (128 x 512)
int gemm_wres_rgl(const GemmArgs& a);
void launch_gemm_wres_as(const GemmArgs& a, int rgl, hipStream_t stream);
// The generations below share their tile steps (XCD tile order, fragment swizzle, activation step, scalar epilogue, operand alignment) through gemm_tile.h,
// and with every other matrix-core kernel the bf16 hi + lo operand split, the fragment union and the LDS-DMA instruction through mfma_util.h.
bool gemm2_supported(const GemmArgs& a);
void launch_gemm2(const GemmArgs& a, hipStream_t stream);
bool gemm3_supported(const GemmArgs& a);   // direct-to-register activations, 256-row blocks (gemm3.hip)
void launch_gemm3(const GemmArgs& a, hipStream_t stream);
extern thread_local int g_gemm3_cfg;
bool gemm5_supported(const GemmArgs& a);   // gemm3's data movement without its conditional loads, swizzled weight image, batched epilogue (gemm5.hip)
void launch_gemm5(const GemmArgs& a, hipStream_t stream);
extern thread_local int g_gemm5_cfg;

// Weight-streaming linear for the AR step (M <= kStepMaxRows rows): C[M,N] = epi(prologue(A)[M,K] * W[N,K]^T).
// splitk > 1: raw partial sums go to partial[z][M][N] (no bias / epilogue); a consumer adds them up in a fixed order.
// The optional prologue (SkinnyFuse; needs K == row width <= 1024, splitk == 1) folds the preceding residual update
// and LayerNorm into the activation staging.
struct StepFinish;   // defined with StepState below
// A deferred "rows += sum of split-K planes + bias": `splitk` planes of raw sums, pstride elements apart, added in plane order by the prologue of the rows'
// next consumer (k_skinny, k_rowprep, k_layernorm_reg).  It sits inside those kernels' by-value arguments: a static_assert behind each pins where it lies.
struct PendingSum { const float* partial = nullptr; int splitk = 0; int64_t pstride = 0; const float* bias = nullptr; };
struct SkinnyFuse {
    // x[row] += pgate[row] * (sum_z pend.partial[z][row] + pend.bias)   (partial: [splitk][M][K])
    PendingSum pend;
    const float* pgate = nullptr; int64_t ldpg = 0;
    float* x_out = nullptr;          // the updated rows, written once (dense [M, K]); must not alias A
    int ln = 0;                      // 1: LayerNorm the rows before the product
    const float* ln_w = nullptr; const float* ln_b = nullptr; float eps = 1e-5f;
    const float* shift = nullptr; const float* scale = nullptr; int64_t ldmod = 0;   // adaLN modulation
    float* y_out = nullptr;          // the normalised rows, written once (dense [M, K])
    // last launch of an AR step (the Euler update that produces the frame): the step's bookkeeping (k_step_finish) rides in the
    // epilogue -- the frame is appended to the utterance's latents and the slot's counters advance.  One column block only
    // (N <= 64), so every reader of the counters in this launch has read them before the one lane per row that writes them.
    const StepFinish* fin = nullptr; // device memory
    // with fin: the block also OPENS THE NEXT STEP (fin->ch): x = input_linear(frame, NaN -> bos), fx = input_proj(next noise row), x0 = that row --
    // k_step_begin's work without its launch.  The frame then goes to the utterance's latents only (C is not written: it holds x0).
    int chain = 0;
    const float* chain_noise = nullptr; int64_t chain_noise_stride = 0;   // [B][max_steps][ldim] or null (zeros)
};
static_assert(sizeof(SkinnyFuse) == 152 && offsetof(SkinnyFuse, pgate) == 32, "k_skinny takes it by value: the layout stays");
bool skinny_supported(const GemmArgs& a, int splitk);
bool skinny_fuse_supported(const GemmArgs& a, const SkinnyFuse& f);
void launch_skinny(const GemmArgs& a, const SkinnyFuse& fu, int splitk, float* partial, hipStream_t stream);
extern thread_local unsigned long long* g_skinny_stamps;
// in-situ stamps of a whole AR step (ptts_debug_step_stamps): while set, every stampable launch of the step linear writes its
// blocks' 8 ticks at base + 8 * used and notes its shape
struct SkinnyStampLog {
    unsigned long long* base = nullptr; size_t cap_blocks = 0, used_blocks = 0;
    struct Desc { int32_t M, N, K, pro, nj, cg, blocks, splitk; };
    std::vector<Desc> desc;
};
extern thread_local SkinnyStampLog* g_skinny_stamp_log;
extern thread_local hipEvent_t g_skinny_ev[2];   // when set, launch_skinny times the dispatch with them (hipExtLaunchKernel)

// The AR step's big linears at 128+ rows (tall.hip): row preparation once per row, then a 64 x 64-tile product whose operands both stream through LDS.
struct PrepArgs {   // x' = x + pend (the planes in order, then the bias) -> x_out; LayerNorm(x') -> bf16 hi / lo planes [M][ldy] (and f32 rows to y_out)
    const float* x = nullptr; int64_t ldx = 0;
    PendingSum pend;                 // planes [splitk][M][D]
    float* x_out = nullptr;          // dense [M][D]; written only with pend.partial
    const float* ln_w = nullptr; const float* ln_b = nullptr; float eps = 1e-5f;
    uint16_t* yh = nullptr; uint16_t* yl = nullptr; int64_t ldy = 0;
    float* y_out = nullptr;
    int M = 0, D = 0;
};
static_assert(sizeof(PrepArgs) == 120 && offsetof(PrepArgs, x_out) == 48, "k_rowprep takes it by value: the layout stays");
bool rowprep_supported(const PrepArgs& a);
void launch_rowprep(const PrepArgs& a, hipStream_t stream);
int rowprep_blocks(int M);           // its grid: one wave per row, four rows per block
// splitk > 1 keeps k_skinny's convention: with R, plane 0 = R + (sums_0 + bias) and the other planes raw sums; without R every plane holds raw sums and a bias
// is the consumer's business (PendingSum::bias) -- tall_supported refuses splitk > 1 with a bias and no R, which the kernel would drop in silence.
struct TallArgs {   // C[M,N] = epi(A[M,K] * W[N,K]^T + bias), A = ah + al (bf16 planes), W the fragment-ordered bf16 copy (Linear::wt)
    const uint16_t* ah = nullptr; const uint16_t* al = nullptr; int64_t lda = 0;
    const void* Wt = nullptr; const float* bias = nullptr;
    const float* R = nullptr; int64_t ldr = 0;                     // EPI_RESADD; with splitk > 1: added (with the bias) into plane 0
    float* C = nullptr; int64_t ldc = 0;                           // f32 result, or
    uint16_t* ch = nullptr; uint16_t* cl = nullptr; int64_t ldp = 0;   // the result as bf16 hi / lo planes (the next product's A)
    float* partial = nullptr; int64_t zstride = 0; int splitk = 1; // splitk > 1: planes [splitk][M][N]
    int M = 0, N = 0, K = 0, epi = EPI_NONE;
};
constexpr int kTallMinRows = 128;   // from this many rows the step's in_proj / linear1 / linear2 run on k_tall (below, k_skinny's one-block-per-CU shape wins)
bool tall_supported(const TallArgs& a);
void launch_tall(const TallArgs& a, hipStream_t stream);   // = launch_tall_as(a, tall_rows(a.M))
// its launch form: blocks of 32 or 64 rows x 64 columns x a K slice (tall_grid).  tall_rows is the only place that chooses for production (32 up to 128 rows, 64
// above); launch_tall_as with the other form is for the kernel's test hook, any other `rows` is PTTS_EINVAL
int tall_rows(int M);
void tall_grid(const TallArgs& a, int rows, int grid[3]);
void launch_tall_as(const TallArgs& a, int rows, hipStream_t stream);

struct LnArgs {
    const float* x = nullptr; RowMap xmap;
    const float* w = nullptr; const float* b = nullptr;  // null -> no affine (flow_net.go:228)
    float eps = 1e-5f;
    // optional adaLN modulation y = y * (1 + scale[row]) + shift[row]   (tensor_util.go:175-193)
    const float* shift = nullptr; const float* scale = nullptr; int64_t ldmod = 0;
    float* y = nullptr; int64_t ldy = 0;   // y == null: reduction prologue only
    int rows = 0, d = 0;
    // optional fused split-K reduction + residual update, applied before the normalisation (flat rows, d % 4 == 0):
    //   x[row] += pgate[row] * pscale * (sum_z pend.partial[z][row] + pend.bias)       (x is updated in place)
    PendingSum pend;
    const float* pgate = nullptr; int64_t ldpg = 0;
    const float* pscale = nullptr;
};
static_assert(sizeof(LnArgs) == 160 && offsetof(LnArgs, pgate) == 136, "k_layernorm takes it by value: the layout stays");
void launch_layernorm(const LnArgs& a, hipStream_t stream);
// Bessel-variance "RMS" norm of the timestep embedder (tensor_util.go:273-326), in place
void launch_rmsnorm_alpha(float* x, const float* alpha, float eps, int rows, int d, hipStream_t stream);

// rows of `table` selected by ids (conditioner.go:47, shape_ops.go Gather)
void launch_embed_gather(const float* table, const int64_t* ids, int n, int d, float* out, hipStream_t stream);
// out[r, i] = isnan(in[r, i]) ? bos[i] : in[r, i]   (tensor_util.go:242-271); in_idx (optional) picks the source row
void launch_replace_nan(const float* in, const float* bos, int rows, int d, float* out, hipStream_t stream);
// elementwise helpers
void launch_silu(float* x, int64_t n, hipStream_t stream);
void launch_copy_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int d, hipStream_t stream);
// out[r, c] = sin/cos timestep features: [cos(t*f) | sin(t*f)]  (flow_net.go:52-65)
void launch_timestep_features(float t, const float* freqs, int nf, float* out, hipStream_t stream);
// y[i] = 0.5 * (a[i] + b[i])   (flow_net.go:330-335)
void launch_avg2(const float* a, const float* b, float* y, int n, hipStream_t stream);

// interleaved-pair RoPE (rope.go:81-105) on rows of a [rows, ld] buffer: for each row r and head h the
// vector at x + r*ld + col0 + h*hd is rotated with the table row pos[r]
// position of row r: pos ? pos[r] : pos_base + (rows_per_seg ? r % rows_per_seg : r)
void launch_rope_rows(float* x, RowMap xmap, int col0, int heads, int hd, const int32_t* pos, int pos_base, int rows_per_seg,
                      int rows, const float* cos_t, const float* sin_t, hipStream_t stream);

// KV cache layout: [slot][head][capacity][hd]; append K/V rows taken from a qkv buffer [rows, 3*D]
void launch_kv_append(const float* qkv, int64_t ld, int d_model, int heads, int hd, const int32_t* row_slot,
                      const int32_t* row_pos, int rows, void* kcache, void* vcache, int kv_bf16, int64_t cap,
                      hipStream_t stream);

struct AttnArgs {
    // one query per (row, head)
    const float* q = nullptr; int64_t q_ld = 0; int q_col0 = 0;   // q vector at q + rowaddr(row) + q_col0 + h*hd
    int64_t q_rows_per_batch = 0, q_batch_stride = 0;             // RowMap of the q rows (0: flat, row*q_ld)
    int pos_base = 0;                                             // added to the implicit position (row % rows_per_seg)
    // keys/values: key j of (row, head) at kbase + seg(row)*k_seg_stride + h*k_head_stride + j*k_row_stride
    const void* k = nullptr; const void* v = nullptr; int kv_bf16 = 0;
    int64_t k_seg_stride = 0, k_head_stride = 0, k_row_stride = 0;
    const int32_t* row_seg = nullptr;   // null: seg = row / rows_per_seg
    int rows_per_seg = 0;
    const int32_t* row_pos = nullptr;   // query position; null: pos = row % rows_per_seg
    const int32_t* seg_len = nullptr;   // if set (AR step): pos = seg_len[seg], rope+append fused
    int context = -1;                   // keys j with pos-context < j <= pos   (attention.go:473-484)
    float* out = nullptr; int64_t out_ld = 0;  // out + rowaddr(row) + h*hd
    int64_t o_rows_per_batch = 0, o_batch_stride = 0;
    int rows = 0, heads = 0, hd = 64;
    int max_keys = 0;                   // upper bound on keys per query (sizes the LDS score buffer)
    int keys_now = 0;                   // fused step: host-side upper bound on (cache length + 1) over the rows of THIS launch; 0: unknown
    // fused RoPE + KV append for the AR step (flow_transformer.go:340-347): q,k,v read from a qkv row
    int fused_step = 0; const float* qkv = nullptr; int64_t qkv_ld = 0; int d_model = 0;
    const float* cos_t = nullptr; const float* sin_t = nullptr; int64_t cap = 0;
    const int32_t* active = nullptr;    // per segment; inactive rows write zeros and append nothing
    // fused step only: keys j < pre_len[seg] are read from a shared prefix (a device voice, [layer][head][pre_len][hd] in the
    // cache dtype) instead of the segment's own cache rows
    const void* const* pre_k = nullptr; const void* const* pre_v = nullptr; const int32_t* pre_len = nullptr; int layer = 0;
    // ragged segments (prompt prefill on the matrix cores, attn_window.hip): rows of segment s are the packed rows
    // [rag_off[s], rag_off[s+1]) at positions rag_pos0[s] + i; rows_per_seg is then the longest segment
    const int32_t* rag_off = nullptr; const int32_t* rag_pos0 = nullptr; int rag_segs = 0;
};
extern thread_local const char* g_last_attn_kernel;
// Launch census for parity tests (ptts_debug_launch_counts): while switched on for the calling thread, every launcher notes the
// kernel it picked, so a test can assert that the path it means to check is the one that ran.  Off: one thread-local load.
extern thread_local std::map<std::string, int64_t>* g_launch_census;
inline void note_launch(const char* kernel) { if (g_launch_census) (*g_launch_census)[kernel]++; }
void launch_attention(const AttnArgs& a, hipStream_t stream);   // picks k_attn_step for the fused AR step when the cache fits one burst
bool attn_step_supported(const AttnArgs& a);
void launch_attn_step(const AttnArgs& a, hipStream_t stream);
int attn_step_keys_per_round(bool kv_bf16);       // keys one load round of the block covers (32 bf16 / 16 f32)
int attn_step_rounds(int keys, bool kv_bf16);     // rounds launch_attn_step issues for a launch bounded by `keys` (1..16)
int attn_step_launch_rounds(const AttnArgs& a);   // ... for this launch: bounded by keys_now when the host knows it, by max_keys otherwise
bool attn_window_supported(const AttnArgs& a);   // Mimi sliding-window attention on the f32 matrix cores
void launch_attn_window(const AttnArgs& a, hipStream_t stream);   // = launch_attn_window_as(a, attn_window_form(a))
// The kernel forms of attn_window.hip.  WAVE: k_attn_window, every wave fetches its own key tiles (the only form for ragged segments and bf16 caches);
// LDS: k_attn_window_lds<4>, the key tiles of 128 queries shared through LDS (dense f32 only, 32-bit element offsets inside a segment).
enum { AW_FORM_WAVE = 1, AW_FORM_LDS = 2 };
int attn_window_form(const AttnArgs& a);           // the production choice for a launch attn_window_supported takes
bool attn_window_form_supported(const AttnArgs& a, int form);
void launch_attn_window_as(const AttnArgs& a, int form, hipStream_t stream);   // (test hook: a form the operands do not allow is PTTS_EINVAL)

// latent [B, T, L] -> x[b, 1+t, :] = Wp * latent + bp  (model.go:252-319), row 0 of each utterance zeroed
void launch_projector(const float* latent, int64_t lat_bstride, const float* wp, const float* bp, int b, int t, int f0, int f1,
                      int ldim, int c, float* out, hipStream_t stream);   // frames [f0, f1) -> rows 1+f of out [B][1+t][c]
// depthwise ConvTranspose1d k=2*stride, right-trimmed (convtranspose1d.go:154-202): in [B, 1+T, C] (row 0 = zeros) ->
// out rows [B][pad + T*stride][C]; w0[r][c] multiplies x[t-1], w1[r][c] multiplies x[t]
void launch_upsample_depthwise(const float* in, const float* w0, const float* w1, const float* bias, int b, int t, int f0, int f1,
                               int c, int stride, float* out, int out_pad_rows, hipStream_t stream);   // frames [f0, f1)
// voice model-state ingestion (flow_transformer.go:568-631): raw [2,1,T,H,D] f32 -> first `offset` rows of a slot's K and V cache
void launch_voice_scatter(const float* raw, int t, int heads, int hd, int offset, int slot, void* kcache, void* vcache,
                          int kv_bf16, int64_t cap, hipStream_t stream);
// copies a compact device voice (K, V as [H][offset][hd] in the cache dtype) into the first `offset` rows of several slots
void launch_voice_apply(const void* vk, const void* vv, int offset, int heads, int hd, const int32_t* slots, int n_slots,
                        void* kcache, void* vcache, int elem_bytes, int64_t cap, hipStream_t stream);
// the reverse of launch_voice_apply for many voices at once (voice_build): voice i receives the first dst[i].offset rows of slot dst[i].slot of
// every layer and head of a batch cache [L][B][H][cap][hd], as [L][H][offset][hd] in the cache dtype; one launch for all voices and layers.
// hd * elem_bytes must be a multiple of 16, all buffers 16-byte aligned; max_offset bounds dst[i].offset (sizes the grid)
struct VoiceDst { void* k; void* v; int32_t offset; int32_t slot; };
void launch_voice_extract(const void* kcache, const void* vcache, int B, int64_t cap, int heads, int hd, int elem_bytes, int n_layers,
                          const VoiceDst* dst_dev, int n_voices, int max_offset, hipStream_t stream);
// the inverse of launch_voice_scatter: a compact voice (K, V as [L][H][offset][hd] in the cache dtype) -> per layer the reference's
// [2, 1, offset, H, hd] f32 cache, layer after layer in out; bf16 widened exactly.  hd % 8 == 0, buffers 16-byte aligned
void launch_voice_export(const void* vk, const void* vv, int offset, int heads, int hd, int n_layers, int kv_bf16, float* out, hipStream_t stream);
// final causal conv Cin -> 1, kernel k, ELU on the input (mimi.go:781-783): in [B][pad+T][C] channels-last
void launch_conv_final(const float* in, int in_pad_rows, const float* w /*[k*C]*/, const float* bias, int b, int t, int t0, int t1,
                       int c, int k, int elu_in /* 0: the producer already applied ELU */, float* out /*[B][T]*/, hipStream_t stream);   // samples [t0, t1) of every utterance
void launch_zero_rows(float* base, int64_t batch_stride, int b, int64_t n, hipStream_t stream);
// PCM egress: out[i] = int16(clamp(in[i], -1, 1) * 32767), product in f64, truncation, NaN -> 0 (audio/wav_stream.go:43-54); n % 8 == 0 or any n
void launch_pcm16(const float* in, int16_t* out, int64_t n, hipStream_t stream);
// the same on samples [off, off + n) of each of `rows` rows (row_stride samples apart; off, n, row_stride % 8 == 0)
void launch_pcm16_rows(const float* in, int16_t* out, int rows, int64_t row_stride, int64_t off, int64_t n, hipStream_t stream);

// Rate and format conversion of delivered audio (resample.hip, k_resample): one launch converts a table of rows, each with its own rate
// pair, taps and output format.  Output j of a row sits at input position j*M/L: y[j] = sum over ascending k of x[base + dlo + k] * h[p][k]
// (base = floor(j*M/L), p = j*M mod L), one f32 fmaf chain from 0; inputs outside [0, n_in) read as zero.  taps == nullptr: the identity
// (L = M = 1, y[j] = x[j]).  The result is stored as f32, as WritePCM16Samples' int16, or as G.711 mu-law / A-law of that int16.
enum ResampleFmt : int32_t { RS_F32 = 0, RS_S16 = 1, RS_ULAW = 2, RS_ALAW = 3 };   // = PTTS_PCM_*
constexpr int kResampleThreads = 256;
constexpr int kResampleMaxTile = 4 * kResampleThreads;   // outputs per workgroup (4 consecutive per lane)
constexpr int kResampleWindow = 6144;                    // floats of input window a workgroup stages in LDS (at most)
constexpr int kResampleTapsLds = 10240;                  // tap tables up to this many floats are staged in LDS; larger ones are read through the caches
struct ResampleRow {
    const float* src;      // input samples (device)
    void* dst;             // output j goes to element j of dst (device or page-locked host memory), in the row's format
    const float* taps;     // phase-major [L][K] (device, 16-byte aligned, padded to a multiple of 4 floats), nullptr: identity
    // streaming hand-overs: the utterance's active flag and frame count as the host snapshot them (device; nullptr: n_in and o1 as given).
    // If the utterance has ended inside the input (fin, *nf * spf < n_in, or !*act with *nf * spf <= n_in -- the flag is snapshot before the
    // count, so an inactive utterance comes with its final count), its input ends at *nf * spf and every output up to
    // ceil(n_in * L / M) -- at most o_cap -- is written
    const int32_t* nf; const int32_t* act;
    int64_t n_in, o0, o1, o_cap;   // outputs [o0, o1) are written (o_cap >= o1 bounds the grid)
    int32_t L, M, K, dlo;
    int32_t fmt, tile, spf, fin;   // tile: outputs per workgroup (multiple of 4, <= kResampleMaxTile)
};
// rows_dev: device copy of the n rows; lds_bytes / max_tiles: the largest dynamic LDS and tile count any row needs (resample.cpp sizes them)
void launch_resample(const ResampleRow* rows_dev, int n, int max_tiles, size_t lds_bytes, hipStream_t stream);
// k_resample launches of the whole process, every thread (the dispatcher's workers included): ptts_debug_resample_launches
extern std::atomic<int64_t> g_resample_launches;

// Post-processing of decoded 24 kHz audio in place (dsp.hip): ptts_dsp_apply's chain -- peak normalise, DC block,
// fade in, fade out -- on a table of ragged rows.  k_dsp_peak (normalise rows: max |x| as the uint32 image, atomicMax), k_dsp_summary +
// k_dsp_carry (DC rows: the zero-state end state of every full tile, then the state entering each tile in tile order; scan_block.h) and
// k_dsp_apply (gain, the recurrence of every run from its entering state, the fade gains, one store).  Tiles are kDspTile samples on the
// row's own grid, so a row's bits do not depend on the rows beside it.
// Loudness rows (DSP_LOUD): k_dsp_peak as for normalise, then k_loud_summary + k_loud_carry (the K-weighting cascade's four states per tile,
// as the DC block's two), k_loud_energy (each tile's four sub-block energies) and k_loud_gate (block energies, both gates, the mean square M
// and the row's f32 gain with the 1 / peak ceiling) on the samples as they come (raw, or as the compressor in front left them); k_dsp_summary and k_dsp_apply then take the row's gain from that word
// where normalise's gain sits.  Tables without such a row launch the kernels they launched before it existed.
// Equaliser rows (DSP_EQ): k_eq_summary + k_eq_carry + k_eq_apply behind k_dsp_apply, on what it stored (gain and DC block applied, rounded
// to f32): the row's own cascade of 1 .. 4 sections (scan_block.h EqScan, 2 .. 8 states per tile), then the fades, which k_dsp_apply leaves to
// k_eq_apply for such a row.  A table's distinct equalisers (at most kDspMaxEq) travel behind its rows; a row names its own by index (how rows
// are cut into tables, here and for the compressor and the limiter below: row_tables.h).
// True-peak rows (DSP_TP; true_peak.hip, true_peak.h): k_tp_peak + k_tp_scale behind the table's last kernel, on what the chain stored: the row's
// true peak (eight-fold oversampled, atomicMax on its own zeroed word) and, where it exceeds the row's ceiling, one gain over the whole row.  A
// row with the ceiling as its only switch passes through k_dsp_apply untouched.  Tables without such a row launch what they launched before.
// Limiter rows have no flag here: their kernels run on a table of their own (LimRow below) between this table's last kernel and k_tp_peak; a
// row with the limiter as its only switch passes through k_dsp_apply untouched, like one with the ceiling alone.
// Windows (a streamed joined call, ptts_debug_dsp_windows): a launch of the causal stages -- the compressor, the DC block, the equaliser, the
// fades -- may cover tiles [t0, ceil(n / kDspTile)) of a row only, n the samples up to the window's end, with the per-tile states of the window
// alone in scratch.  DSP_OPEN (CmpRow::open): more samples follow behind n, which is then a multiple of kDspTile; the window's last tile hands a
// state on like the others, the state behind it is left in `carry` and no fade out is applied (the window that closes the row applies it, with
// the row's final n).  The next window starts from `carry`.  The fold S_(f+1) = A^1920 S_f + E_f is the same sequence of operations wherever
// the row is cut, so the windows give the bits of the one-shot chain, which is the window t0 = 0, carry null, of a closed row.  The carried
// states of one row: kCarryDoubles doubles, zero in front of the row's first window.
enum DspFlags : int32_t { DSP_NORMALIZE = 1, DSP_DC = 2, DSP_LOUD = 4, DSP_EQ = 8, DSP_TP = 16, DSP_OPEN = 32 };
constexpr int kCarryDc = 0, kCarryEq = 2, kCarryCmpP = 10, kCarryCmpS = 11, kCarryDoubles = 12;   // DspScan::N, then 2 kEqMaxSections, then the compressor's two
constexpr int kDspMaxEq = 16;
constexpr size_t kDspEqBytes = 1192;
static_assert(sizeof(EqScan) == kDspEqBytes, "the DSP ring's tail (runtime.h) is sized by it");
struct DspRow {
    float* x;              // the row's samples (device), rewritten in place
    int64_t n;             // samples; nothing at or beyond n is touched
    int64_t fade_in, fade_out;   // samples of each fade (0: none, <= n)
    uint32_t* peak;        // normalise and loudness rows: one word, zero before k_dsp_peak
    double* tiles;         // DC rows: the DC block's per-tile states (scan_block.h scan_E / scan_S)
    int32_t flags, eq;     // eq: equaliser rows: the index of the row's equaliser among the table's
    double* loud;          // loudness rows: M, the gain, the K-weighting's per-tile states, the sub-block energies (scan_block.h loud_states / loud_subs)
    double target;         // 10^((target LUFS + 0.691) / 10)
    double* eq_tiles;      // equaliser rows: the cascade's per-tile states, 2 S doubles each for E_f and S_f
    uint32_t* tp;          // true-peak rows: one word, zero before k_tp_peak, then the row's true peak as its uint32 image
    float ceiling;         // true-peak rows: the linear ceiling c = (float)pow(10, dBTP / 20)
    int64_t t0;            // the window's first tile (0: the row from its start); tiles, eq_tiles hold the window's tiles, entry 0 is tile t0's
    double* carry;         // the row's carried states, [kCarryDoubles] (null: a one-shot row, started from zero state and closed)
};
static_assert(sizeof(DspRow) == 112, "a turn of the DSP ring holds 256 of them");
// which flags occur in a table's rows, and the systems' coefficients (loud: needed with any_loud); apply false: the measuring launches only,
// the samples stay as they are
// any_eq: eqs is the device copy of the table's equalisers
struct DspLaunch {
    bool any_norm, any_dc, any_loud, apply; const DspScan* scan; const LoudScan* loud; bool any_eq = false; const EqScan* eqs = nullptr;
    bool any_open = false;   // a row is open: the summaries cover every tile of the longest window
    bool gain_only = false;  // the loudness rows' gain with its 1 / peak ceiling and nothing else: k_dsp_peak and k_loud_*, no sample is rewritten (level_launch)
};
// rows_dev: device copy of the n rows; max_tiles: the most tiles a row's window has (a one-shot row: ceil(n / kDspTile))
void launch_dsp(const DspRow* rows_dev, int n, int max_tiles, const DspLaunch& p, hipStream_t stream);
// the last two of a table with a true-peak row (true_peak.hip; dsp_launch calls them behind launch_dsp's kernels and the limiter's tables, the
// first alone for a measurement): the true peak of every DSP_TP row into its word; the gain c / TP over the rows whose word exceeds c
struct TpTaps;
void launch_tp_peak(const DspRow* rows_dev, int n, int max_tiles, const TpTaps& taps, hipStream_t stream);
void launch_tp_scale(const DspRow* rows_dev, int n, int max_tiles, hipStream_t stream);

// A request's compressor (compressor.hip, compressor.h): the first stage of the post-processing, on a table of its
// own in front of launch_dsp's.  k_cmp_summary_p + k_cmp_carry_p (the peak detector's state entering each tile: a scan in the (max, times)
// semiring), k_cmp_summary_s + k_cmp_carry_s (the same for the attack smoothing, a linear scan with one state whose runs recompute the detector
// from its entering state) and k_cmp_apply (both states entering every run, the gain curve, one store), in place.  A table's distinct designs
// (at most kCmpMaxDesigns) travel behind its rows; a row names its own by index.
constexpr int kCmpMaxDesigns = 16;
constexpr size_t kCmpScanBytes = 128;
static_assert(sizeof(CmpScan) == kCmpScanBytes, "the compressor ring's tail (runtime.h) is sized by it");
struct CmpRow {
    float* x;              // the row's samples (device), rewritten in place
    int64_t n;             // samples; nothing at or beyond n is touched
    double* p_tiles;       // the detector's per-tile states, [ceil(n / kDspTile)][2]: E_f, S_f (scan_block.h scan_E<1> / scan_S<1>)
    double* s_tiles;       // the smoothing's, likewise
    int32_t design, open;  // the index of the row's design among the table's; open: as DSP_OPEN
    int64_t t0;            // the window's first tile, as DspRow::t0: p_tiles and s_tiles hold the window's tiles
    double* carry;         // as DspRow::carry (kCarryCmpP, kCarryCmpS are this stage's)
};
static_assert(sizeof(CmpRow) == 56, "a turn of the compressor ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the most tiles a row's window has; designs_dev: the table's designs; any_open: a row is open
void launch_compressor(const CmpRow* rows_dev, int n, int max_tiles, const CmpScan* designs_dev, hipStream_t stream, bool any_open = false);

// A request's de-esser (deesser.hip, deesser.h): directly behind the compressor's tables and in front of launch_dsp's,
// on a table of its own.  A scan of three levels, each needing the one in front at every tile's start: k_de_summary_b + k_de_carry_b (the side
// chain's two biquad states entering each tile: the equaliser's linear scan for one section), k_de_summary_p + k_de_carry_p (the detector's, the
// compressor's (max, times) scan on the band, which every tile makes again from the section's entering state), k_de_summary_s + k_de_carry_s
// (the smoothing's, likewise) and k_de_apply (all three again, the curve held at the floor, the band's gain, one store), in place.  The band is
// never stored beside the row.  A table's distinct designs (at most kDeMaxDesigns) travel behind its rows; a row names its own by index.  No
// windows: the stage is refused where a row is handed over window after window (dsp_spec.h dsp_window_refusal).
constexpr int kDeMaxDesigns = 16;
constexpr size_t kDeScanBytes = 256;
static_assert(sizeof(DeScan) == kDeScanBytes, "the de-esser ring's tail (runtime.h) is sized by it");
struct DeRow {
    float* x;              // the row's samples (device), rewritten in place
    int64_t n;             // samples; nothing at or beyond n is touched
    double* b_tiles;       // the section's per-tile states, [ceil(n / kDspTile)][4]: E_f, S_f, two each (scan_block.h scan_E<2> / scan_S<2>)
    double* p_tiles;       // the detector's, [ceil(n / kDspTile)][2] (scan_E<1> / scan_S<1>)
    double* s_tiles;       // the smoothing's, likewise
    int32_t design, pad;   // the index of the row's design among the table's
};
static_assert(sizeof(DeRow) == 48, "a turn of the de-esser ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil(n / kDspTile) of a row; designs_dev: the table's designs
void launch_deesser(const DeRow* rows_dev, int n, int max_tiles, const DeScan* designs_dev, hipStream_t stream);

// A request's look-ahead peak limiter (limiter.hip, limiter.h): behind the fades and in front of the true-peak
// ceiling, on a table of its own behind the DSP table's last kernel and in front of k_tp_peak.  k_lim_summary + k_lim_carry (the release's state
// entering each tile, the compressor's (max, times) scan over the look-ahead hold), k_lim_gain (the state entering every run, then the
// required gain r of every sample as an f32 into scratch) and k_lim_apply (the box mean of r in its fixed order, one product, one store), in
// place.  No kernel reads a sample that another workgroup of the same launch writes: the first three read x and write scratch only,
// k_lim_apply reads x in its own tile only.  A table's distinct designs (at most kLimMaxDesigns) travel behind its rows.
constexpr int kLimMaxDesigns = 16;
constexpr size_t kLimScanBytes = 64;
static_assert(sizeof(LimScan) == kLimScanBytes, "the limiter ring's tail (runtime.h) is sized by it");
struct LimRow {
    float* x;              // the row's samples (device), rewritten in place
    int64_t n;             // samples; nothing at or beyond n is touched
    double* p_tiles;       // the release's per-tile states, [ceil(n / kDspTile)][2]: E_f, S_f (scan_block.h scan_E<1> / scan_S<1>)
    float* r;              // the required gain, [n]
    int32_t design, pad;   // the index of the row's design among the table's
};
static_assert(sizeof(LimRow) == 40, "a turn of the limiter ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil(n / kDspTile) of a row; designs_dev: the table's designs
void launch_limiter(const LimRow* rows_dev, int n, int max_tiles, const LimScan* designs_dev, hipStream_t stream);

// A text's parts joined into one row (join.hip, k_join; join.h has the rule, join.cpp the host statement): a table of
// parts, each copied to its offset in the joined row behind its gap of zeros, its first k samples crossfaded with its predecessor's last k.  A
// row writes [off - gap, off + n): n stops where the successor's seam begins, so the rows' spans tile the joined row and every sample is
// written once.  prev travels with the row, so a seam is computed by one row even when the predecessor sits in the previous table.
constexpr int kJoinThreads = 256;
constexpr int kJoinTile = 4 * kJoinThreads;   // output samples per workgroup (4 consecutive per lane)
struct JoinRow {
    const float* src;      // the part's samples (device)
    const float* prev;     // seam rows (k > 0): the predecessor's last k samples (device); may be dst + off itself, see join.hip
    float* dst;            // the joined row (device)
    int64_t off;           // where the part's first sample goes in dst
    int64_t n;             // the part's samples this row writes: its length minus the seam behind it
    int32_t k;             // samples of the seam in front of the part (0: none; <= n)
    int32_t gap;           // zeros in front of the part, dst[off - gap, off) (0 with k > 0)
};
static_assert(sizeof(JoinRow) == 48, "a turn of the join ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil((gap + n + 3) / kJoinTile) of a row (three more: the destination's 16-byte grid)
void launch_join(const JoinRow* rows_dev, int n, int max_tiles, hipStream_t stream);
// The gain form (join.hip, k_join_gain; include/ptts.h ptts_part_opts): a row of a table in which some part has a volume.  The part's gain and
// the gain of its predecessor's tail (seam rows whose prev is the predecessor's own buffer; a tail in the joined row is already scaled) are each
// none, an immediate f32 that multiplies every sample, or a device word holding one -- a loudness row's gain as k_loud_gate left it (kernels.h
// DspRow::loud + 1), which multiplies where it is not 1.  A table without a gain goes to k_join
enum JoinGainFlags : int32_t { JOIN_GAIN_IMM = 1, JOIN_GAIN_WORD = 2, JOIN_PREV_IMM = 4, JOIN_PREV_WORD = 8 };
struct JoinGainRow {
    JoinRow r;
    const float* gw;       // JOIN_GAIN_WORD: the part's gain (device)
    const float* gw_prev;  // JOIN_PREV_WORD: the predecessor's
    float g, g_prev;       // JOIN_GAIN_IMM, JOIN_PREV_IMM
    int32_t flags, pad;
};
static_assert(sizeof(JoinGainRow) == 80, "a turn of the gain join's ring holds 256 of them");
void launch_join_gain(const JoinGainRow* rows_dev, int n, int max_tiles, hipStream_t stream);

// Silence control of the parts of a joined text (trim.hip, trim.h has the rule, trim.cpp the host statement): in front
// of k_join, from one buffer into another.  k_trim_mark (every tile: its first and last loud index, what its inner pauses lose), k_trim_carry
// (one workgroup per row: the loud index in front of and behind every tile, the row's ptts_trim_info, the exclusive prefix of what the tiles
// keep) and k_trim_store (every tile: what it keeps, at its offset).  A table's distinct designs (at most kTrimMaxDesigns) travel behind its rows.
constexpr int kTrimMaxDesigns = 16;
constexpr size_t kTrimScanBytes = 32;
static_assert(sizeof(TrimScan) == kTrimScanBytes, "the trim ring's tail (runtime.h) is sized by it");
struct TrimTile {
    int32_t first, last;     // k_trim_mark: the tile's first and last loud index in the row (kTrimNoneBehind, kTrimNone: no loud sample in the tile)
    int32_t removed, cuts;   // ... and the samples and the count of the cuts both of whose loud ends lie in the tile
    int32_t prev, next;      // k_trim_carry: the last loud index in front of the tile and the first one behind it (kTrimNone, kTrimNoneBehind)
    int32_t off, pad;        // ... and the output samples in front of the tile's
};
static_assert(sizeof(TrimTile) == 32, "trim_scratch_bytes counts on it");
struct TrimRow {
    const float* src;        // the row's samples (device)
    float* dst;              // where what stays goes (device), [n]: another buffer than src
    int64_t n;               // samples, below 2^31; nothing at or beyond n is touched
    TrimTile* tiles;         // [ceil(n / kDspTile)]
    ptts_trim_info* info;    // the row's record (device): k_trim_carry writes it, k_trim_store reads it
    int32_t design, pad;     // the index of the row's design among the table's
};
static_assert(sizeof(TrimRow) == 48, "a turn of the trim ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil(n / kDspTile) of a row (0: empty rows only, which still get their record);
// designs_dev: the table's designs
void launch_trim(const TrimRow* rows_dev, int n, int max_tiles, const TrimScan* designs_dev, hipStream_t stream);

// The speaking rate of the parts of a joined text (tempo.hip, tempo.h has the rule, tempo.cpp the host statement): behind
// the trim and in front of k_join, from one buffer into another.  k_tempo_plan (one workgroup per row: the hops' read positions, in order) and
// k_tempo_store (every tile of the OUTPUT: the copy or the blend).  A table's distinct designs (at most kTempoMaxDesigns) travel behind its rows.
constexpr int kTempoMaxDesigns = 16;
constexpr size_t kTempoScanBytes = 16;
static_assert(sizeof(TempoScan) == kTempoScanBytes, "the tempo ring's tail (runtime.h) is sized by it");
struct TempoRow {
    const float* src;        // the row's samples (device)
    float* dst;              // the time-scaled row (device), [n_out]: another buffer than src
    int64_t n;               // samples, below kTempoMaxSamples; nothing outside [0, n) is read
    int64_t n_out;           // tempo_length(n, the design's speed): made on the host, the kernels compute no length
    int32_t* p;              // [tempo_hops(n_out)]: the hops' positions; k_tempo_plan writes them, k_tempo_store reads them
    int32_t design, pad;     // the index of the row's design among the table's
};
static_assert(sizeof(TempoRow) == 48, "a turn of the tempo ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil(n_out / kDspTile) of a row (0: empty rows only, nothing is launched);
// designs_dev: the table's designs
void launch_tempo(const TempoRow* rows_dev, int n, int max_tiles, const TempoScan* designs_dev, hipStream_t stream);

// The pitch of the parts of a joined text, its resampling step (pitch.hip, pitch.h has the rule, pitch.cpp the host statement; DESIGN.md section 8,
// N3): behind the trim and in front of the tempo, from one buffer into another.  k_pitch_resample, every tile of kPitchTile OUTPUT samples.  A
// table's distinct designs (at most kPitchMaxDesigns: p may differ from row to row) travel behind its rows.
constexpr int kPitchMaxDesigns = 16;
constexpr size_t kPitchScanBytes = 16;
static_assert(sizeof(PitchScan) == kPitchScanBytes, "the pitch ring's tail (runtime.h) is sized by it");
constexpr int kPitchThreads = 512;
constexpr int kPitchTile = 1024;                        // outputs a workgroup
constexpr int kPitchWindow = 2 * kPitchTile + 110;      // the floats of a tile's input window, at the most (p = 2000)
// The prototype table as the kernel reads it: entry q = {h[q], hd[q]} at pair pitch_image_at(q), one unused pair behind every 32 (pitch.hip has why)
PTTS_HD inline int pitch_image_at(int q) { return q + (q >> 5); }
constexpr int kPitchImage = (kPitchEntries + (kPitchEntries >> 5) + 1) & ~1;   // pairs of floats
struct PitchRow {
    const float* src;        // the row's samples (device)
    float* dst;              // the resampled row (device), [n_out]: another buffer than src
    int64_t n;               // samples; nothing outside [0, n) is read
    int64_t n_out;           // pitch_resample_length(n, the design's p), below kTempoMaxSamples: made on the host
    int32_t design, pad;     // the index of the row's design among the table's
};
static_assert(sizeof(PitchRow) == 40, "a turn of the pitch ring holds 256 of them");
// rows_dev: device copy of the n rows; max_tiles: the largest ceil(n_out / kPitchTile) of a row (0: empty rows only, nothing is launched);
// designs_dev: the table's designs; image_dev: the table's image, [kPitchImage][2]
void launch_pitch(const PitchRow* rows_dev, int n, int max_tiles, const PitchScan* designs_dev, const float* image_dev, hipStream_t stream);

// "Keep the formants" around the pitch's resampling step (formant.hip, formant.h has the rule, formant.cpp the host statement; DESIGN.md section 8,
// N3), for the rows that have the option: k_formant_analyse (every frame of the row) and k_formant_whiten (every tile of 240 samples around a frame
// boundary) in front of k_pitch_resample, which then reads the residual e and writes er; k_formant_shape (16 output tiles a wave) behind it.
constexpr int kFormantAnalyseThreads = 256;   // four waves, a frame each
constexpr int kFormantWhitenThreads = 256;    // 240 samples a workgroup
constexpr int kFormantShapeTiles = 16;        // output tiles a wave: kFormantSlots lanes each
struct FormantRow {
    const float* x;          // the part (device), [n]
    float* e;                // its residual, [n]: another buffer
    const float* er;         // the resampled residual, [n_r]
    float* out;              // the shaped row, [n_r]: another buffer than er
    float* coeffs;           // [K][24]: a32[1 .. 24] of every frame
    int64_t n, n_r;          // n_r = pitch_resample_length(n, p), made on the host
    int32_t K, p;            // formant_frames(n), at least 1; pitch_permille, 800 .. 1500
};
static_assert(sizeof(FormantRow) == 64, "a turn of the formant ring holds 256 of them");
// rows_dev: device copy of the n rows (every one with n > 0); max_frames: the largest K of a row; tables_dev: formant_tables() on the device
void launch_formant_analyse(const FormantRow* rows_dev, int n, int64_t max_frames, const double* tables_dev, hipStream_t stream);
// max_tiles: the largest (n + 119) / 240 + 1 of a row
void launch_formant_whiten(const FormantRow* rows_dev, int n, int64_t max_tiles, hipStream_t stream);
// max_tiles: the largest ceil(n_r / 240) of a row
void launch_formant_shape(const FormantRow* rows_dev, int n, int64_t max_tiles, hipStream_t stream);

// One SEANet residual block (+ optionally the final conv) as a single launch, resblock.hip.  u / uo: channels-last
// [B][pad + L][C] with `pad` zero history rows per utterance; rows [t0, t1) of every utterance are produced.
// final_conv with rows: utterance b's samples [0, lim) go straight to dst (f32, or int16 through WritePCM16Samples' arithmetic) --
// dst may be page-locked host memory: the kernel's stores are the device->host transfer
struct PcmRow { void* dst; int32_t lim; int32_t s16; };
struct ResArgs {
    const float* u = nullptr; int64_t u_bs = 0; int pad = 0;
    float* uo = nullptr;                       // elu(u + block(u)), same layout as u (not written when final_conv)
    float* pcm = nullptr; int64_t pcm_bs = 0;  // final_conv: [B][L] samples
    const PcmRow* pcm_rows = nullptr;          // final_conv: if set, used instead of pcm (t0 % 4 == 0, dst 16-byte aligned)
    const void* w1 = nullptr; const void* w1_lo = nullptr; const float* b1 = nullptr;   // conv k1 (3): fragment-ordered [H][3C]
    const void* w2 = nullptr; const void* w2_lo = nullptr; const float* b2 = nullptr;   // conv k2 (1): fragment-ordered [C][H]
    const void* wf_hi = nullptr; const void* wf_lo = nullptr; const float* bf = nullptr;  // final conv as a one-column fragment-ordered matrix (hi + lo planes), bias [1]
    int B = 0, L = 0, t0 = 0, t1 = 0;
    int C = 0, H = 0, k1 = 0, k2 = 0, kf = 0, w_bf16 = 0, final_conv = 0;
    // k_resblock_up (resblock_up.hip): the transposed convolution in front of the block computed in the same kernel -- u is then not read
    // but made from xin, the previous block's rows [B][x_pad + x_L][CI] (x_L = L / up_stride), with the fragment-ordered [stride*C][2*CI]
    // weights wup (bf16) and the bias bup [C]
    int fuse_up = 0; const float* xin = nullptr; int64_t x_bs = 0; int x_pad = 0, x_L = 0, CI = 0, up_stride = 0;
    const void* wup = nullptr; const float* bup = nullptr;
};
bool resblock_supported(const ResArgs& a);                    // the shape conditions; the block has no size threshold of its own
void launch_resblock(const ResArgs& a, hipStream_t stream);   // = launch_resblock_as(a, resblock_plan(..., RES_FORM_AUTO, 0, resblock_cus()))
bool resblock_up_shape_supported(const ResArgs& a);           // the fused form's shape conditions ...
bool resblock_up_supported(const ResArgs& a);                 // ... and its size threshold (resblock_up_plan's automatic choice has a grid)
void launch_resblock_up(const ResArgs& a, hipStream_t stream);
// The launch form: one tile of `tout` new rows per block (grid = B * tiles), or `grid` persistent blocks of nw waves that walk the B * tiles tiles
// (blockIdx.x, + gridDim.x, ...; 1 <= grid <= B * tiles: a block whose first tile is past the end would index past B).  resblock_plan / resblock_up_plan
// are the only places that choose: form AUTO is the production choice (thresholds against `cus` compute units), TILE / PERS with `grid` are for the
// block's test hook; grid 0 in the result: the form does not exist for this block (PERS), or the fused kernel is not taken (AUTO below its threshold).
enum { RES_FORM_AUTO = 0, RES_FORM_TILE = 1, RES_FORM_PERS = 2 };
struct ResPlan { int nw = 0, pers = 0, grid = 0, tiles = 0, tout = 0; };
int resblock_cus();
ResPlan resblock_plan(int C, int final_conv, int w_bf16, int B, int rows, int form, int grid, int cus);
ResPlan resblock_up_plan(int B, int rows, int form, int grid, int cus);
void launch_resblock_as(const ResArgs& a, const ResPlan& p, hipStream_t stream);
void launch_resblock_up_as(const ResArgs& a, const ResPlan& p, hipStream_t stream);


// The feed-forward half of a Mimi decoder-transformer layer as one kernel (ffn_fused.hip): x += ls * linear2(gelu(linear1(LayerNorm(x)))),
// rows of x updated in place; img: the per-chunk weight images of model.cpp add_ffn_image (bf16)
struct FfnArgs {
    float* x = nullptr; RowMap xmap;
    const float* ln_w = nullptr; const float* ln_b = nullptr; float eps = 1e-5f;
    const void* img = nullptr;
    const float* ls = nullptr;      // [D] layer scale or null (1)
    int M = 0, D = 0, F = 0;
};
// LayerNorm + linear (+ RoPE on the first rope_cols output columns, head width 64) with register-resident rows (ffn_fused.hip k_mimi_rowlin):
// y[M][N] = rope(LayerNorm(x)[M][512] * W[N][512]^T); img: W as W1-format chunk images (model.cpp add_w1_image, bf16); no bias
struct RowLinArgs {
    const float* x = nullptr; RowMap xmap;
    const float* ln_w = nullptr; const float* ln_b = nullptr; float eps = 1e-5f;
    const void* img = nullptr;
    float* y = nullptr; RowMap ymap;
    const float* rope_cos = nullptr; const float* rope_sin = nullptr; int rope_cols = 0, rope_pos0 = 0, rope_rows_per_seg = 0;   // tables [pos][32]
    int M = 0, N = 0, K = 0;
};
bool mimi_rowlin_supported(const RowLinArgs& a);
void launch_mimi_rowlin(const RowLinArgs& a, hipStream_t stream);
bool mimi_ffn_supported(const FfnArgs& a);
void launch_mimi_ffn(const FfnArgs& a, hipStream_t stream);

// The residual blocks of the flow net (flow_net.go:116-172: `depth` x [adaLN-modulated LayerNorm -> linear + SiLU -> linear, gated, + residual], all C x C) as ONE
// launch (flow_cluster.hip): 8 workgroups per 16-row tile, each owning 64 output columns of every linear; the rows go round between the eight through tagged
// 8-byte granules.  Weights: the step kernel's fragment-ordered bf16 copies (Lin::wt).
constexpr int FC_MAX_DEPTH = 8;
struct FlowClusterArgs {
    const float* fx_in = nullptr; float* fx_out = nullptr;   // [rows][C] the residual stream in / out (may be the same buffer)
    const float* ada = nullptr; int64_t ldmod = 0;           // adaLN rows [rows][ldmod]: block r at 3 r C: shift | scale | gate
    int rows = 0, depth = 0;
    float eps[FC_MAX_DEPTH] = {};
    const float* ln_w[FC_MAX_DEPTH] = {}; const float* ln_b[FC_MAX_DEPTH] = {};
    const void* w0[FC_MAX_DEPTH] = {}; const float* b0[FC_MAX_DEPTH] = {};
    const void* w2[FC_MAX_DEPTH] = {}; const float* b2[FC_MAX_DEPTH] = {};
    unsigned long long* xbuf = nullptr;   // granules {value, tag}: [tile of 12 rows][2][16][C]
    unsigned long long* stamps = nullptr; // measurement only (null in the product): [workgroup][64] timestamps
    int inject = 0;                       // test hook (0 in the product): workgroup 7 of tile 0 publishes nothing for mlp0 of block inject - 1 -> its peers' sweeps time out
    unsigned* sync = nullptr;             // [tile] the tag base of the tile's next launch, 32 words apart; word 32 * kFlowClusterMaxTiles: fault flags
};
constexpr int kFlowClusterRows = 12;                                        // rows of the batch per tile (8 workgroups each)
constexpr int kFlowClusterMaxTiles = (kStepMaxRows + kFlowClusterRows - 1) / kFlowClusterRows;   // 22 tiles = 176 workgroups at 256 rows: one per CU, all resident at once
constexpr size_t kFlowClusterTileBytes = (size_t)2 * 16 * 512 * 8;          // a tile's two granule buffers
constexpr size_t kFlowClusterSyncBytes = (size_t)(32 * kFlowClusterMaxTiles + 32) * 4;
inline size_t flow_cluster_xbuf_bytes(int rows) { return (size_t)((rows + kFlowClusterRows - 1) / kFlowClusterRows) * kFlowClusterTileBytes; }
// whether a grid of 8 workgroups per 12-row tile is resident at once on `device` (the hand-offs between a tile's workgroups spin: they need their peers running)
bool flow_cluster_fits(int rows, int device);
bool flow_cluster_supported(const FlowClusterArgs& a, int C);
void launch_flow_cluster(const FlowClusterArgs& a, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// AR-step bookkeeping (runtime_native_safetensors.go:176-192 per slot, on device)
struct StepState {
    int32_t* kv_len;        // [B] keys in the cache (== flowTransformerLayerState.offset)
    int32_t* active;        // [B]
    int32_t* step;          // [B] next frame index
    int32_t* countdown;     // [B] -1 == nil
    int32_t* n_frames;      // [B]
    int32_t* eos_step;      // [B]
    int32_t* max_steps;     // [B]
    int32_t* frames_after_eos;  // [B]
    float*   eos_threshold; // [B]
    int32_t* n_active;      // [1]
    int32_t* broke;         // [B] 1 when the loop left through the countdown `break` (no StepCallback for that step)
};
// the NEXT step's opening (what k_step_begin computes), for the step's last launch to carry (k_skinny FIN + CHAIN, step_open.h)
struct StepChain {
    const void* w_in; const float* b_in; float* x; int32_t d_in;      // input_linear [d_in][ldim] row-major -> x [B][d_in]
    const void* w_pj; const float* b_pj; float* fx; int32_t d_pj;     // input_proj [d_pj][ldim] -> fx [B][d_pj]
    const float* bos; float* x0; int32_t w_bf16; int32_t ok;          // x0: [B][ldim], the next step's noise row (or zeros); ok: the shapes fit (ldim == 32, ...)
};
struct StepFinish {         // arguments of k_step_finish, resident in device memory (Batch::fin_dev)
    StepState s;
    const float* eos_logit; // [B]
    float* latents;         // [B][lat_stride]
    int64_t lat_stride;
    int32_t ldim;
    StepChain ch;
};
// prepares the step input: in32[b] = step==0 ? bos : latents[b][step-1] with NaN -> bos, x0[b] = noise of the step (or 0);
// with `lin` also x = input_linear(in32) and fx = input_proj(x0) (the two ldim-wide linears of the step, exact f32)
struct StepOpenLinears {
    const void* w_in = nullptr; const float* b_in = nullptr; int d_in = 0; float* x = nullptr;     // [d_in][ldim] row-major
    const void* w_pj = nullptr; const float* b_pj = nullptr; int d_pj = 0; float* fx = nullptr;    // [d_pj][ldim]
    int w_bf16 = 0;
};
bool step_open_mfma_ok(const StepOpenLinears& lin, int ldim);   // the matrix-core form (step_open.h) takes these shapes; it is the form a step's last launch can chain
void launch_step_begin(const StepState& s, const float* latents, int64_t lat_stride, const float* bos, const float* noise, int64_t noise_stride,
                       int ldim, int b, float* in32, float* x0, const StepOpenLinears* lin, hipStream_t stream);
// stores the decoded frame, applies EOS logic, advances kv_len/step
void launch_step_finish(const StepState& s, const float* frame, const float* eos_logit, int ldim, int b, float* latents,
                        int64_t lat_stride, hipStream_t stream);
// device draw of the sampling noise (flow_lm.go:386-408): slot b gets rows [0, spec[b].rows) of out + b * out_stride as
// N(0,1) * spec[b].sigma, a function of (spec[b].seed, row, element) only; rows == 0 leaves the slot untouched.  ldim % 4 == 0.
struct NoiseSpec { uint64_t seed; float sigma; int32_t rows; };
void launch_noise_fill(const NoiseSpec* spec_dev, int n_slots, int max_rows, float* out, int64_t out_stride, int ldim, hipStream_t stream);
// continuous batching: (re)initialise the bookkeeping of the slots a new utterance moves into; switch cancelled slots off
struct GatherTable { struct Row { int32_t src_row, dst_off, nf, T; }; Row rows[128]; };   // (2 KB of kernel arguments)
void launch_gather_frames(const GatherTable& t, int n, const float* stage, int64_t row_stride, float* dst, int ld, hipStream_t stream);   // ld % 4 == 0
void launch_readback_i32(const int32_t* a, int na, const int32_t* b, int nb, int32_t* host, hipStream_t stream);   // host: page-locked, device-visible; [a | b]
struct SlotAdmit { int32_t slot, max_steps, frames_after_eos; float eos_threshold; int32_t kv_len, pre_len; const void* pre_k; const void* pre_v; };
void launch_slot_admit(const StepState& s, int32_t* pre_len, const void** pre_k, const void** pre_v, const SlotAdmit* dev, int n, hipStream_t stream);
void launch_slot_retire(const StepState& s, const int32_t* slots_dev, int n, hipStream_t stream);
void launch_fill_i32(int32_t* p, int32_t v, int n, hipStream_t stream);
void launch_add_i32(int32_t* p, const int32_t* inc, int n, hipStream_t stream);

// Mimi encoder pieces (encoder.hip; PARITY UNPINNED, inferred chain: DESIGN.md section 7)
// the 1-channel input conv: out[t * ldo + c] = b[c] + sum_x w[c][x] pcm[t + x] for t < L (pcm holds k - 1 zero history samples in front)
void launch_enc_head(const float* pcm, const void* w, int w_bf16, const float* b, int64_t L, int C, int k, float* out, int64_t ldo, hipStream_t stream);
// out[M][N] = A[M][K] * W[N][K]^T + bias (A rows lda apart), split-K: raw planes partial[enc_ds_splits(M, N, K)][M][N] summed in slice order
int enc_ds_splits(int M, int N, int K);
void launch_enc_downsample(const float* A, int64_t lda, const void* W, int w_bf16, const float* bias, int M, int N, int K, float* partial, float* out,
                           hipStream_t stream);

// [B, C, T] <-> channels-last helpers for the op-level entry points
void launch_bct_to_btc(const float* in, int b, int c, int t, float* out, int out_pad_rows, hipStream_t stream);
void launch_btc_to_bct(const float* in, int in_pad_rows, int b, int c, int t, float* out, hipStream_t stream);

}  // namespace ptts
