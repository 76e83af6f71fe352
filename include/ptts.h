/*
 * ptts.h -- C ABI of libptts_hip.so: the MI355X-native PocketTTS synthesis path.
 *
 * Drop-in boundary.  The reference has no FFI; its seam is the Go interface
 *     type Runtime interface { GenerateAudio(ctx, tokens []int64, cfg RuntimeGenerateConfig) ([]float32, error); Close() }
 * (internal/tts/runtime.go:42-45) implemented by nativeSafetensorsRuntime
 * (internal/tts/runtime_native_safetensors.go:20-244) on top of native.Model
 * (internal/native/model.go:25-138).  The entry points below are exactly what a
 * cgo binding of that seam needs; each one names the reference method it
 * replaces.  INTEGRATION.md shows the cgo shim.
 *
 * Conventions (mirroring the reference's):
 *   - every call returns 0 on success or a PTTS_E* code; the message is
 *     ptts_last_error() (thread-local), worded like the reference's Go errors;
 *   - no exceptions cross the ABI; inputs are borrowed and never mutated;
 *   - outputs are library-allocated and released with ptts_free_result(), or
 *     caller-allocated where a size is known up front;
 *   - a model handle may be shared by threads; ptts_generate() calls on one
 *     model are serialised on that model's HIP stream.
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with PTTS_ENODEVICE.
 */
#ifndef PTTS_H
#define PTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTTS_OK          0
#define PTTS_EINVAL      1   /* bad argument / shape / range (reference: fmt.Errorf paths) */
#define PTTS_EIO         2   /* file cannot be read */
#define PTTS_EFORMAT     3   /* not a valid safetensors / missing tensor */
#define PTTS_ENODEVICE   4   /* no HIP device, or a HIP call failed */
#define PTTS_ECANCELLED  5   /* ctx.Err() between steps (runtime_native_safetensors.go:156-159) */
#define PTTS_ENOMEM      6

/* how weights are held in HBM */
#define PTTS_WEIGHTS_F32   0  /* as the reference holds them (every dtype decoded to f32, store.go:339-395) */
#define PTTS_WEIGHTS_BF16  1  /* 2 bytes/param; exact when the file itself is BF16 */
#define PTTS_WEIGHTS_INT8  2  /* weight-only int8 for every matrix the AR step streams (1 byte/param, per-row f32 scale: q = rint(W / s),
                               * s = max|row| / 127; the effective weights q*s are used consistently by prefill and step); the rest as
                               * PTTS_WEIGHTS_BF16.  Not a reference mode (the reference's int8 is ONNX quantize_dynamic,
                               * scripts/export_onnx.py:319-331): tolerance stated against the f32 oracle in tests/test_gpu_int8.py */
/* KV-cache element type */
#define PTTS_KV_F32   0
#define PTTS_KV_BF16  1

typedef struct ptts_model ptts_model;
typedef struct ptts_plan  ptts_plan;
typedef struct ptts_batch ptts_batch;
typedef struct ptts_voice ptts_voice;

typedef struct ptts_opts {
    int32_t device;          /* HIP device ordinal */
    int32_t weights;         /* PTTS_WEIGHTS_* */
    int32_t kv;              /* PTTS_KV_* */
    int32_t max_batch;       /* utterances stepped together on the GPU (default 64, at most 256) */
    int32_t use_graph;       /* 0 (default): the ~47 launches of an AR step are issued per step -- the host stays ~3x ahead of
                                the GPU and there is no gap between steps; 1: the step is captured once into a hipGraph and
                                replayed (one host call per step, ~8 us of idle GPU between replays: up to 3 % slower, but the
                                launching thread needs a fraction of the CPU time) */
    int32_t reserved0;       /* must be 0 (round 2's step_plan: the alternative launch plans were measurements, not options; they live in tools/probes/step_plans) */
    int32_t reserved[10];
} ptts_opts;

void ptts_default_opts(ptts_opts* o);

typedef struct ptts_info {
    int64_t d_model, n_heads, n_layers, ffn, ldim, n_bins;      /* flow_lm.go:13-27 */
    int64_t flow_dim, flow_depth;                               /* flow_net.go:242-248 */
    int64_t mimi_dim, mimi_heads, mimi_layers, mimi_context;    /* mimi.go:16-34 */
    int64_t sample_rate, samples_per_frame, steps_per_latent;   /* MimiTiming(): runtime_native_safetensors.go:40-49 */
    double  frame_rate, encoder_frame_rate;
    int64_t n_params, arena_bytes;
    int32_t weights, kv;
} ptts_info;

/* ---- model lifetime: native.LoadModelFromSafetensors / LoadModelFromStore / Model.Close
 *      (internal/native/model.go:33-71) ---- */
int  ptts_model_open(const char* safetensors_path, const ptts_opts* opts, ptts_model** out);
int  ptts_model_open_bytes(const void* data, size_t len, const ptts_opts* opts, ptts_model** out);
void ptts_model_close(ptts_model* m);                               /* nil-safe, like Model.Close */
int  ptts_model_info(const ptts_model* m, ptts_info* out);
const char* ptts_last_error(void);

/* Two-phase open for multi-GPU start-up: every rank plans from the
 * file header alone, allocates one device arena of ptts_plan_arena_bytes(), rank 0
 * fills it (fill=1: decode, convert, derive tables, upload) and the arena is then
 * broadcast once over RCCL/xGMI; the other ranks adopt it as is (fill=0). */
int    ptts_plan_create(const char* safetensors_path, const ptts_opts* opts, ptts_plan** out);
int    ptts_plan_create_bytes(const void* data, size_t len, const ptts_opts* opts, ptts_plan** out);
size_t ptts_plan_arena_bytes(const ptts_plan* p);
int    ptts_model_open_planned(ptts_plan* p, void* device_arena, int fill, ptts_model** out); /* consumes p */
/* The broadcast itself, for hosts that have no collective library of their own (the reference's Go server): rank 0 makes the id
 * (ncclGetUniqueId), hands the 128 bytes to the other processes over the channel that started them, then EVERY rank calls
 * ptts_rccl_broadcast on its arena (root = rank 0; one ncclCommInitRank + ncclBroadcast + ncclCommDestroy over RCCL / xGMI).
 * librccl is loaded on first use (PTTS_RCCL_LIB overrides the name).
 * STATUS: exercised with n_ranks == 1 only (tests/test_gpu_model.py); the two-rank test (tests/test_gpu_multirank.py) needs a box with
 * two GPUs and has not run.  Compare a checksum of the arena across ranks after the hand-over (bench.py open_model does). */
int    ptts_rccl_unique_id(uint8_t out[128]);
int    ptts_rccl_broadcast(void* device_buf, size_t bytes, int32_t rank, int32_t n_ranks, const uint8_t id[128], int32_t device);
/* host image of the arena (ptts_plan_arena_bytes() bytes), for hosts that upload / broadcast it themselves; needs no GPU */
int    ptts_plan_fill_host(const ptts_plan* p, void* host_arena);
void   ptts_plan_free(ptts_plan* p);

/* ---- the Runtime seam: tts.Runtime.GenerateAudio (runtime_native_safetensors.go:52-238) ---- */
typedef void (*ptts_step_callback)(void* user, int32_t step, int32_t max_steps); /* RuntimeGenerateConfig.StepCallback */

typedef void (*ptts_pcm_callback)(void* user, int64_t sample_offset, int64_t n_samples, const void* samples);

#define PTTS_PCM_F32  0
#define PTTS_PCM_S16  1
#define PTTS_PCM_ULAW 2   /* G.711 mu-law bytes of the PCM16 sample (result.pcm8) */
#define PTTS_PCM_ALAW 3   /* G.711 A-law bytes of the PCM16 sample (result.pcm8) */

/* Post-processing of a request's audio on the device: the request's result is what
 *     ptts_dsp_apply(samples, n, normalize, dc_block, fade_in_ms, fade_out_ms)
 * makes of THAT REQUEST'S OWN 24 kHz f32 audio (n = n_frames * 1920; no padded frame is ever read), and THEN the request's egress
 * (sample_rate, pcm_format) exactly as specified without it.  Order: normalise -> DC block -> fade in -> fade out, every intermediate
 * rounded to f32 where ptts_dsp_apply rounds it.  Normalise and the fades give ptts_dsp_apply's bits; the DC block is the same float64
 * recurrence evaluated as a blocked scan and agrees with it to one f32 step at the row's peak.  It is per request: the reference's CLI
 * runs the chain over a whole text's concatenated chunks (cmd/pockettts/synth.go:361-390); a host that wants that for a multi-chunk
 * text keeps using ptts_dsp_apply, or ptts_dsp_rows, on the concatenation -- or has ptts_generate_joined (below) join the chunks and run the
 * chain once over the whole text on the device.
 *
 * The equaliser (`eq`, a handle of ptts_eq_create below: a cascade of one to four biquad sections chosen by the caller) sits behind the DC
 * block and in front of the fades.  The whole order of a request's chain: the loudness or normalise gain -> DC block -> equaliser -> fade in
 * -> fade out -> egress.  The host statement of the result: ptts_loudness_normalize, or ptts_dsp_apply(normalize, dc_block, 0, 0); then
 * ptts_eq_apply; then ptts_dsp_apply(0, 0, fade_in_ms, fade_out_ms); then the egress.  The equaliser gives ptts_eq_apply's bits.  Peak and
 * loudness are measured on the raw decoded audio, in front of the equaliser: a boosting equaliser can push samples past +-1, and the PCM16
 * and G.711 egress clamps them as it always does (f32 leaves as it is) -- unless the request sets a true-peak ceiling or a limiter.
 *
 * The true-peak ceiling (`ext`, a handle of ptts_dsp_ext_create below with true_peak = 1) is the last stage.  The whole order of a request's
 * chain: the loudness or normalise gain -> DC block -> equaliser -> fade in -> fade out -> true-peak ceiling -> egress.  The host statement of
 * the result: everything before the ceiling as above, then ptts_true_peak_limit(samples, n, ceiling_dbtp, NULL), then the egress; the device
 * gives ptts_true_peak_limit's bits.  It is a STATIC ceiling, not a limiter: the true peak of the whole utterance is measured and, where it
 * exceeds the ceiling, every sample is scaled by the one gain ceiling / true peak -- nothing pumps, and an utterance under the ceiling is not
 * touched.  The ceiling holds for the 24 kHz signal: rate conversion and PCM16 or G.711 quantisation come after it and may add a little.
 *
 * The compressor (attached to the `ext` handle by ptts_dsp_ext_set_compressor below) is the FIRST stage, on the request's own raw 24 kHz
 * audio.  The whole order of a request's chain: compressor -> the loudness or normalise gain -> DC block -> equaliser -> fade in -> fade out
 * -> true-peak ceiling -> egress.  The host statement of the result: ptts_compress_apply, then everything as above; the device gives
 * ptts_compress_apply's bits.  Peak and loudness are measured on the COMPRESSED audio, so a request still lands on its LUFS target.
 *
 * The limiter (attached to the `ext` handle by ptts_dsp_ext_set_limiter below) sits behind the fades and in front of the true-peak ceiling.  The
 * whole order of a request's chain: compressor -> the loudness or normalise gain -> DC block -> equaliser -> fade in -> fade out -> limiter
 * -> true-peak ceiling -> egress.  The host statement of the result: everything in front of the limiter as above, then ptts_limit_apply, then
 * ptts_true_peak_limit if the ceiling is set, then the egress; the device gives ptts_limit_apply's bits.  With a limiter a boosting equaliser
 * or a makeup gain no longer ends in the egress's hard clip: sample peaks stay at or under its ceiling, and the static ceiling behind it has
 * only the inter-sample remainder to take off.
 *
 * The de-esser (attached to the `ext` handle by ptts_dsp_ext_set_deesser below) runs directly behind the compressor: what is said above of the
 * compressor -- everything else is measured and applied behind it -- holds for the pair.  The whole order of a request's chain: compressor ->
 * de-esser -> the loudness or normalise gain -> DC block -> equaliser -> fade in -> fade out -> limiter -> true-peak ceiling -> egress.  The
 * host statement of the result: ptts_compress_apply, then ptts_deess_apply, then everything as above; the device gives ptts_deess_apply's bits. */
#if defined(__GNUC__)
#define PTTS_ANON __extension__
#else
#define PTTS_ANON
#endif
typedef struct ptts_eq ptts_eq;
typedef struct ptts_dsp_ext ptts_dsp_ext;
typedef struct ptts_dsp_opts {
    int32_t normalize;      /* PeakNormalize */
    int32_t dc_block;       /* DCBlock, 20 Hz, Q 0.707, at 24 kHz */
    double  fade_in_ms;     /* <= 0: none */
    double  fade_out_ms;
    PTTS_ANON union {
        int32_t reserved[4];    /* no word is left: eq lies over reserved[0..1], ext over reserved[2..3] */
        PTTS_ANON struct {
            const ptts_eq* eq;           /* NULL, or a live handle of ptts_eq_create (borrowed for the call) */
            const ptts_dsp_ext* ext;     /* NULL, or a live handle of ptts_dsp_ext_create (borrowed for the call): further per-request options */
        };
    };
} ptts_dsp_opts;

typedef struct ptts_request {
    const int64_t* tokens; int64_t n_tokens;          /* must be non-empty (:57-59) */
    float   temperature;                              /* RuntimeGenerateConfig.Temperature: sampling noise = N(0,1) * sqrt(max(t, 0)), drawn on the
                                                       * device per (noise_seed, step) when `noise` is NULL; <= 0: zero noise (flow_lm.go:386-408) */
    float   eos_threshold;                            /* isEOS = logit > threshold (flow_lm.go:281) */
    int32_t max_steps;                                /* <=0: estimated_max_steps, then EstimateMaxFrames (:61-67) */
    int32_t estimated_max_steps;
    int32_t lsd_steps;                                /* <=0 -> 1 (:69-72) */
    int32_t frames_after_eos;                         /* text.FramesAfterEOS */
    /* voice conditioning, mutually exclusive (:100-102) */
    const float* voice_embedding; int64_t voice_frames;        /* [Tv, d_model], prepended (:104-119) */
    const float* const* voice_caches;                           /* per layer [2,1,T,H,Dh] f32 (flow_transformer.go:451-552) */
    const int64_t* voice_cache_steps;                           /* per layer T */
    const int64_t* voice_offsets;                               /* per layer offset, 0 <= offset <= T */
    /* injected sampling noise (reproducible runs, parity tests): [noise_rows, ldim] = N(0,1)*sqrt(temperature) draws, one row
     * per AR step, consumed as x0 of that step's LSD decode (flow_lm.go:283-288); replaces the device draw.  NULL: the library
     * draws (temperature > 0) or uses zeros (temperature <= 0). */
    const float* noise;
    ptts_step_callback step_callback; void* callback_user;
    const volatile int32_t* cancel;                   /* polled between steps; nonzero -> PTTS_ECANCELLED */
    int32_t want_latents;                             /* 1: also return the latent frames */
    int32_t pcm_format;                               /* PTTS_PCM_F32 (0): result.pcm; PTTS_PCM_S16 (1): result.pcm16, encoded on the device;
                                                       * PTTS_PCM_ULAW (2) / PTTS_PCM_ALAW (3): result.pcm8, G.711 of that int16, encoded on the device */
    /* a voice model state already resident in HBM (ptts_voice_create); exclusive with the two host forms above.
     * The reference loads the voice file once per Synthesize call and rebuilds the FlowLM state from it for
     * every chunk (service.go:127,216-246, flow_lm.go:134-145); the device copy is that cached voice. */
    const ptts_voice* voice;
    uint64_t noise_seed;                              /* device draw: the stream of this request; 0 = a fresh one per request from the model's
                                                       * own generator, seeded with the clock at open like the reference's (runtime_native_safetensors.go:27-32) */
    int32_t noise_rows;                               /* rows behind `noise`; must cover the resolved step budget (0: not checked, the caller vouches) */
    /* Loudness normalisation on the device: 0 off; otherwise the target integrated loudness in units of 0.01 LUFS,
     * -7000 .. -100 (-2300: EBU R 128, -1600: streaming, IVR).  The request's result is what
     *     ptts_loudness_normalize(samples, n, loudness / 100.0, NULL)
     * makes of THAT REQUEST'S OWN 24 kHz f32 audio, bit for bit, THEN `dsp` (the gain sits where normalise's gain sits: the DC block reads
     * x * gain, the fades follow), THEN the egress.  Loudness is measured on the decoded audio as the compressor leaves it (the raw decoded
     * audio for a request without one), so the final audio is at the target up to what the DC block and the fades remove.  PTTS_EINVAL naming the field for another value, together with dsp->normalize (one gain slot),
     * and together with pcm_callback (the loudness is not known when samples are handed over). */
    int32_t loudness;
    /* Frame-granular streaming (the /tts/stream path, server.go:354-396, at finer grain than the reference's per-chunk
     * PCMChunk): finished frame ranges are decoded while the AR loop is still running and handed over in order, each sample
     * exactly once, from a library thread; `samples` points into the buffer the result will own (float or int16 per
     * pcm_format).  The callback must not call into this library.  stream_frames: frames per hand-over (<= 0: 12 = 0.96 s). */
    ptts_pcm_callback pcm_callback; void* pcm_user;
    int32_t stream_frames;
    /* output rate in Hz (0: 24000, the decoder's own): a multiple of 25 from 8000 to 48000.  Other than 24000 (or a G.711 format), the
     * decoded samples go through k_resample on the device -- the polyphase filter of DESIGN.md section 8 (N3) -- and n_samples, stream
     * offsets and buffers count samples at this rate: n_frames * 0.08 * sample_rate.  Other values: PTTS_EINVAL naming the rate. */
    int32_t sample_rate;
    /* post-processing on the device, in front of the egress above (borrowed for the call).  NULL, or a struct with nothing switched on:
     * none.  PTTS_EINVAL naming the field for a negative or NaN fade, an `eq` that is not a live handle of ptts_eq_create ("dsp: eq"), an
     * `ext` that is not a live handle of ptts_dsp_ext_create ("dsp: ext ... (reserved[2..3])": junk in those words is refused, never read),
     * and for any switch together with pcm_callback (the peak and the end of the utterance are not known when samples are handed over;
     * dc_block, fade_in_ms, eq and ext are refused with it as well, for now). */
    const ptts_dsp_opts* dsp;
} ptts_request;

typedef struct ptts_result {
    float*  pcm;       int64_t n_samples;             /* fresh copy owned by the caller (:237) */
    float*  latents;   int32_t n_frames;              /* [n_frames, ldim] when want_latents */
    int32_t eos_step;                                 /* first step whose EOS logit crossed the threshold, -1 if none */
    int32_t status;                                   /* per-request PTTS_* code */
    int16_t* pcm16;                                   /* PTTS_PCM_S16: n_samples little-endian samples, v = int16(clamp(s, -1, 1) * 32767)
                                                       * exactly as audio.WritePCM16Samples (internal/audio/wav_stream.go:43-54); pcm is NULL then */
    uint8_t* pcm8;                                    /* PTTS_PCM_ULAW / PTTS_PCM_ALAW: n_samples G.711 bytes (ITU-T G.711, the classic linear2ulaw /
                                                       * linear2alaw of the PCM16 sample); pcm and pcm16 are NULL then.  Freed by ptts_free_result */
} ptts_result;

/* A second ENGINE over the weights of `base` (its own streams, KV caches, workspaces; the weight arena is shared and
 * read-only): two engines on one GPU, e.g. behind one dispatcher, let one batch's Mimi decode run beside the next batch's
 * prefill + AR loop.  `base` must outlive the engine; a device voice belongs to the engine it was uploaded to. */
int  ptts_model_share(ptts_model* base, ptts_model** out);
/* The model on ANOTHER GPU of the same process (one process, N GPUs: the shape of the reference's single server with its N workers,
 * internal/server/server.go:119-143,398-421): a private weight arena on `device`, copied from base's over the GPUs' direct link (hipMemcpyPeer) -- the file
 * is read and decoded once, no collective library is involved.  Independent of `base` afterwards (either may be closed first).  A dispatcher over the N
 * models (ptts_dispatcher_create) deals requests to them; a device voice belongs to the GPU it was uploaded to.  `device` may be base's own. */
int  ptts_model_replicate(ptts_model* base, int32_t device, ptts_model** out);
/* ptts_opts.use_graph of an open model, changed between calls (A/B measurement, hosts that become short of CPU) */
int  ptts_model_set_use_graph(ptts_model* m, int32_t use_graph);
/* ptts_opts.max_batch of an open model or engine (1..256), changed between calls: how many utterances of one ptts_generate call are stepped
 * together (the reference's counterpart is its worker count, internal/server/server.go:132-134, internal/config/config.go:87); the engine's
 * KV caches and workspaces follow on the next call */
int  ptts_model_set_max_batch(ptts_model* m, int32_t max_batch);

/* n_reqs == 1 reproduces GenerateAudio exactly.  n_reqs > 1 is this library's batching
 * extension: independent utterance chunks stepped together (per-row EOS countdown, ragged KV). */
int  ptts_generate(ptts_model* m, const ptts_request* reqs, int32_t n_reqs, ptts_result* results);
void ptts_free_result(ptts_result* r);

/* The 44-byte header audio.WriteWAVHeaderStreaming emits in front of a PCM16 stream (internal/audio/wav_stream.go:15-41):
 * 24 kHz, mono, 16 bit, RIFF and data sizes 0xFFFFFFFF. */
void ptts_wav_header_streaming(uint8_t out[44]);

/* Optional post-processing of a finished utterance, in place, in the order the CLI applies it (cmd/pockettts/synth.go:361-390):
 * PeakNormalize, DCBlock (20 Hz high-pass), FadeIn, FadeOut (internal/audio/dsp.go:12-78); 24 kHz.  Host samples, host code (the device
 * form: ptts_request.dsp, ptts_dsp_rows).
 * Normalise and the fades are bit-exact restatements; the DC block's biquad comes from a third-party module in the reference and
 * is held to the properties the reference's tests state (parity unpinned). */
int  ptts_dsp_apply(float* samples, int64_t n, int32_t normalize, int32_t dc_block, double fade_in_ms, double fade_out_ms);
/* The same chain on the device, by the kernels a request's `dsp` runs: rows of host samples at 24 kHz (in[i]: n[i] floats, any length
 * >= 0), one launch sequence for all rows, out[i] (host, n[i] floats; in[i] == out[i] allowed) receives the result.  opts NULL or with
 * nothing switched on copies.  PTTS_EINVAL as for ptts_request.dsp. */
int  ptts_dsp_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, const ptts_dsp_opts* opts, float* const* out);

/* Integrated loudness after ITU-R BS.1770-4, mono, at 24 kHz, and normalisation to a target.  float64 throughout:
 * the K-weighting (high shelf, high-pass; the bilinear forms that reproduce the standard's 48 kHz table, evaluated for 24 kHz) as a cascade of
 * two direct form II transposed sections, 400 ms blocks every 100 ms (whole blocks only: block j is samples [2400 j, 2400 j + 9600)), the
 * absolute gate at -70 LUFS and the relative gate 10 LU under the mean of the absolutely gated blocks, both applied to the mean squares;
 * LUFS = -0.691 + 10 log10(mean of the gated blocks).  The recurrence is evaluated in the blocked form of the device kernels, with every
 * summation order fixed, so the host functions and the device forms (ptts_request.loudness, ptts_loudness_rows,
 * ptts_loudness_normalize_rows) give the same bits.
 * ptts_loudness: *lufs receives the loudness, -INFINITY when no block passes the gates (fewer than 9600 samples, silence, below -70 LUFS).
 * ptts_loudness_normalize, in place: samples *= gain with gain = min((float)sqrt(T / M), 1.0f / peak) -- T = 10^((target + 0.691) / 10), M the
 * gated mean square, peak the sample peak of ptts_dsp_apply's normalise -- one f32 product per sample; the ceiling means the result never
 * clips and may stay under the target (the SAMPLE peak is held; for the true peak see ptts_true_peak_limit).  The gain stays 1 (samples untouched) when no block passes the gates or M is
 * not finite.  *measured (optional) receives the loudness before the gain.  target_lufs: -70 .. -1, else PTTS_EINVAL.
 * Non-finite samples are not treated specially, as in normalise: a NaN never wins the peak and a block whose energy is NaN fails both gates
 * (every comparison with it is false); an infinite sample makes the peak infinite and the ceiling 0. */
int  ptts_loudness(const float* samples, int64_t n, double* lufs);
int  ptts_loudness_normalize(float* samples, int64_t n, double target_lufs, double* measured);
/* The same on the device, by the kernels a request's `loudness` runs, shaped like ptts_dsp_rows: rows of host samples at 24 kHz (in[i]: n[i]
 * floats, any length >= 0), one launch sequence for all rows.  lufs / measured: [rows] (measured optional); out[i]: n[i] floats, in[i] == out[i]
 * allowed.  A host that wants one loudness over a text's chunks calls these on the concatenation, or ptts_generate_joined with `loudness`. */
int  ptts_loudness_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, double* lufs);
int  ptts_loudness_normalize_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, double target_lufs, float* const* out,
                                  double* measured);

/* A per-request equaliser at 24 kHz: a cascade of one to four biquad sections of the published RBJ cookbook in its
 * Q form -- w0 = 2 pi freq_hz / 24000, alpha = sin(w0) / (2 q), shelves and peaking with A = 10^(gain_db / 40) -- designed in float64,
 * normalised by a0, run in direct form II transposed with float64 state, each output rounded once to f32.
 * Ranges: freq_hz 10 .. 11000, q 0.1 .. 10, gain_db -24 .. +24 for PTTS_EQ_LOWSHELF / HIGHSHELF / PEAKING and exactly 0 for PTTS_EQ_LOWPASS /
 * HIGHPASS, reserved 0, every value finite; anything else is PTTS_EINVAL and the error names the section index and the field.
 * Telephony band-limiting in front of 8 kHz mu-law, as a worked example:
 *     ptts_eq_section s[2] = {{PTTS_EQ_HIGHPASS, 0, 300.0, 0.0, 0.7071}, {PTTS_EQ_LOWPASS, 0, 3400.0, 0.0, 0.7071}};
 *     ptts_eq* eq; ptts_eq_create(s, 2, &eq);
 *     ptts_dsp_opts o = {0}; o.eq = eq;   request.dsp = &o; request.sample_rate = 8000; request.pcm_format = PTTS_PCM_ULAW;
 *     ... ptts_generate ...               ptts_eq_free(eq);   (once no request that names it is running)
 * ptts_eq_design: coeffs receives b0, b1, b2, a1, a2 of one section (y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2).  Host only.
 * ptts_eq_response: *gain_db receives 20 log10 |H| of the cascade of n (1 .. 4) sections at freq_hz (above 0, below 12000).  Host only.
 * ptts_eq_create: the handle of a cascade of n (1 .. 4) sections.  It belongs to no model: it holds host memory only and works with every
 * model, every ptts_model_share engine and every dispatcher of the process.  The caller keeps it alive while requests that name it are running,
 * as with ptts_request.voice.  ptts_eq_free(NULL) does nothing.
 * ptts_eq_apply: the cascade over host samples, in place, evaluated in the blocked form the device kernels run (runs of 30 samples, tiles of
 * 1920): the device forms -- ptts_dsp_opts.eq, ptts_eq_rows -- give these bits.  It agrees with the sample-by-sample recurrence to one f32
 * step at the row's peak.
 * ptts_eq_rows: the same on the device, by the kernels a request's `eq` runs, shaped like ptts_dsp_rows; eq[i] may differ per row, NULL copies
 * the row.  PTTS_EINVAL naming the row for a handle that is not live. */
#define PTTS_EQ_LOWPASS   1
#define PTTS_EQ_HIGHPASS  2
#define PTTS_EQ_LOWSHELF  3
#define PTTS_EQ_HIGHSHELF 4
#define PTTS_EQ_PEAKING   5
typedef struct ptts_eq_section { int32_t type; int32_t reserved; double freq_hz, gain_db, q; } ptts_eq_section;
int  ptts_eq_design(const ptts_eq_section* s, double coeffs[5]);
int  ptts_eq_response(const ptts_eq_section* s, int32_t n, double freq_hz, double* gain_db);
int  ptts_eq_create(const ptts_eq_section* s, int32_t n, ptts_eq** out);
void ptts_eq_free(ptts_eq* e);
int  ptts_eq_apply(const ptts_eq* e, float* samples, int64_t n);
int  ptts_eq_rows(ptts_model* m, const ptts_eq* const* eq, const float* const* in, const int64_t* n, int32_t rows, float* const* out);

/* Further per-request options of ptts_dsp_opts, behind a handle made from a size-versioned struct: the caller sets size =
 * sizeof(ptts_dsp_ext_opts) as it compiled it, fields beyond that size read as 0, and a later library version adds fields at the end.
 * ptts_dsp_ext_create answers PTTS_EINVAL naming the field for a size smaller than the two fields below ("size"), a size larger than the
 * library knows with a non-zero byte beyond what it knows ("size"), a true_peak other than 0 or 1, and a ceiling_dbtp that is not a finite
 * value from -60 to 0.  The handle holds host memory only and belongs to no model, like a ptts_eq; the caller keeps it alive while requests
 * that name it are running.  ptts_dsp_ext_free(NULL) does nothing. */
typedef struct ptts_dsp_ext_opts {
    uint32_t size;          /* sizeof(ptts_dsp_ext_opts) as the caller compiled it; fields beyond it read as 0 */
    int32_t  true_peak;     /* 1: keep the request's audio at or under ceiling_dbtp */
    double   ceiling_dbtp;  /* -60 .. 0, finite (EBU R 128: -1) */
} ptts_dsp_ext_opts;
int  ptts_dsp_ext_create(const ptts_dsp_ext_opts* o, ptts_dsp_ext** out);
void ptts_dsp_ext_free(ptts_dsp_ext* e);

/* True peak at 24 kHz.  The row is oversampled eight times, to the 192 kHz of ITU-R BS.1770-4 Annex 2, by the
 * polyphase filter of this library's resampler for the pair 24000 -> 192000 (8 phases of 54 taps, cutoff 0.45 cycles per sample, Kaiser beta
 * 8.6, float64 rounded once to f32): y[8 i + p], for i in [0, n) and p in [0, 8), is one f32 fmaf chain from 0.0f over ascending k = 0 .. 53
 * of x[i - 26 + k] * h[p][k], samples outside [0, n) reading as zero; nothing before sample 0 or at or beyond sample n is an output.
 *     TP = max(max |x[i]|, max |y[j]|)
 * as an f32, linear (20 log10 is the caller's).  A NaN never wins, as in normalise.  TP is never below the sample peak, so a ceiling at or
 * under 0 dBTP also means that no sample clips.  Host and device run the same function and give the same bits.
 * KNOWN LIMIT: content above about 10 kHz lies in the filter's transition band and is under-read (a 10 kHz tone reads 0.16 dB low).  Speech
 * from this decoder has little energy there.
 * ptts_true_peak: *peak receives TP; n = 0 gives 0.  Host.
 * ptts_true_peak_limit, in place, host: c = (float)pow(10, ceiling_dbtp / 20); if TP > c every sample becomes the f32 product x * g with
 * g = c / TP (an IEEE f32 division), otherwise nothing is written.  *peak_before (optional) receives TP.  ceiling_dbtp: -60 .. 0, finite, else
 * PTTS_EINVAL.  A static gain, not a limiter.
 * ptts_true_peak_rows: TP of rows of host samples on the device, by the measuring kernel a request's ceiling runs; shaped like
 * ptts_loudness_rows.  peaks: [rows]. */
int  ptts_true_peak(const float* samples, int64_t n, float* peak);
int  ptts_true_peak_limit(float* samples, int64_t n, double ceiling_dbtp, float* peak_before);
int  ptts_true_peak_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, float* peaks);

/* Dynamic range compressor at 24 kHz: feed-forward, float64.  Per sample, from p = s = 0:
 *     p = max(|x|, rho p)   with rho = exp(-1 / (release_ms * 24))      (a NaN never wins)
 *     s = alpha s + (1 - alpha) p   with alpha = exp(-1 / (attack_ms * 24))
 *     y = (float)(x * g(s)),   20 log10 g = curve(20 log10 s) + makeup_db
 * The curve is the soft-knee one of Giannoulis, Massberg and Reiss (JAES 2012): with L the level and T, R, W the threshold, ratio and knee,
 * 0 where 2 (L - T) < -W, (1 / R - 1)(L - T) where 2 (L - T) > W, (1 / R - 1)(L - T + W / 2)^2 / (2 W) between.  Both recurrences are evaluated
 * as blocked scans on a fixed grid (runs of 30 samples, tiles of 1920; csrc/compressor.h), and that form is the definition: host and device run
 * the same function and give the same bits.  It agrees with the sample-by-sample statement (libm's log10 and pow) to one f32 step at the
 * row's peak.  No look-ahead, no side-chain filter (the de-esser below is this detector behind one), not a limiter: a transient shorter than
 * the attack passes.
 * Non-finite samples are not treated specially: a NaN sample comes out as NaN and touches nothing else; an infinite sample holds the level
 * at +inf for the rest of the row, which a ratio above 1 thereby silences (csrc/compressor.h).
 * ptts_compressor_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_dsp_ext_set_compressor attaches the compressor to a live handle of ptts_dsp_ext_create (c NULL: off again); a handle that is not live is
 * PTTS_EINVAL and is not read.  Set it before requests name the handle, not while they run.  Refused together with pcm_callback like every
 * other switch of `ext`.
 * ptts_compress_gain: *gain_db receives the static curve at level_db (finite) including the makeup gain, through the library's own log2 and
 * exp2.  Host.
 * ptts_compress_apply: the compressor over samples[0, n) in place.  Host.
 * ptts_compress_rows: the same on rows of host samples on the device, by the kernels a request's compressor runs; shaped like ptts_eq_rows.
 * c[i] NULL copies row i. */
typedef struct ptts_compressor_opts {
    uint32_t size;          /* sizeof(ptts_compressor_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  reserved;      /* 0 */
    double   threshold_db;  /* -60 .. 0 (dBFS of the detector's level) */
    double   ratio;         /* 1 .. 100 (1: the curve does nothing) */
    double   knee_db;       /* 0 .. 24 (0: hard knee) */
    double   attack_ms;     /* 0.05 .. 200 */
    double   release_ms;    /* 5 .. 5000 */
    double   makeup_db;     /* -24 .. +24 */
} ptts_compressor_opts;
int  ptts_dsp_ext_set_compressor(ptts_dsp_ext* e, const ptts_compressor_opts* c);
int  ptts_compress_gain(const ptts_compressor_opts* c, double level_db, double* gain_db);
int  ptts_compress_apply(const ptts_compressor_opts* c, float* samples, int64_t n);
int  ptts_compress_rows(ptts_model* m, const ptts_compressor_opts* const* c, const float* const* in, const int64_t* n, int32_t rows, float* const* out);

/* De-esser at 24 kHz: the compressor's detector behind a side-chain filter, its gain applied to that band alone.
 * Float64.  Per sample, from zero state:
 *     b = (float) HP(x)     one PTTS_EQ_HIGHPASS section at (freq_hz, q) as ptts_eq_design designs it: b is ptts_eq_apply of that section on x
 *     p = max(|b|, rho p),  s = alpha s + (1 - alpha) p       the compressor's two recurrences on the BAND's level (a NaN never wins)
 *     G = max(curve(20 log10 s), -max_reduction_db)            the compressor's soft-knee curve with makeup 0, held at the floor
 *     y = x  where G is exactly 0 (the sample's 32 bits);  elsewhere  y = (float)(x + (g - 1) b),  20 log10 g = G
 * Only the band is turned down, and never by more than max_reduction_db; where the band's level stays under the knee the row comes back bit
 * for bit (so does every row at ratio 1).  The three recurrences are evaluated as blocked scans on the compressor's grid (runs of 30 samples,
 * tiles of 1920; csrc/deesser.h), through the equaliser's and the compressor's own functions and the library's own log2 and exp2, and that form
 * is the definition: host and device run the same functions and give the same bits.  It agrees with the sample-by-sample statement (libm's
 * log10 and pow) to one f32 step at the row's peak.  One band, minimum phase; no split into complementary bands, no wide-band mode.
 * Non-finite samples are not treated specially: a NaN sample poisons what the biquad's state carries -- the band is NaN from that sample to
 * the end of the row, so y is NaN there wherever G is not 0 and x bit for bit wherever it is (the level, which a NaN never enters, decays) --
 * and an infinite one does too: the level stands at +inf for the rest of the row, G at the floor, and every sample from there on comes out
 * non-finite (csrc/deesser.h).  Samples in front of either are untouched.  Host and device agree on which samples are NaN and on every
 * other sample's bits; a NaN's sign and payload are the processor's.
 * Place in a request's chain: directly behind the compressor and in front of everything else -- compressor -> de-esser -> the loudness or
 * normalise gain -> DC block -> equaliser -> fade in -> fade out -> limiter -> true-peak ceiling -> egress.  Peak and loudness are measured on
 * the de-essed audio.  The host statement of the result: ptts_compress_apply, ptts_deess_apply, then everything as above.  A joined call runs
 * it once over the joined audio, like the rest of the chain.
 * ptts_deesser_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_dsp_ext_set_deesser attaches the de-esser to a live handle of ptts_dsp_ext_create (d NULL: off again); a handle that is not live is
 * PTTS_EINVAL and is not read.  Set it before requests name the handle, not while they run.  Refused together with pcm_callback like every
 * other switch of `ext`; a streamed joined call with a callback refuses it by name (its states are not carried from window to window yet).
 * ptts_deess_apply: the de-esser over samples[0, n) in place.  Host.
 * ptts_deess_band: band[0, n) receives b alone (band may be in).  Host.
 * ptts_deess_rows: ptts_deess_apply on rows of host samples on the device, by the kernels a request's de-esser runs; shaped like
 * ptts_limit_rows.  d[i] NULL copies row i; in[i] == out[i] is allowed; a bad row is named. */
typedef struct ptts_deesser_opts {
    uint32_t size;            /* sizeof(ptts_deesser_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  reserved;        /* 0 */
    double   freq_hz;         /* 2000 .. 10000: corner of the side chain's high-pass */
    double   q;               /* 0.3 .. 4 */
    double   threshold_db;    /* -60 .. 0 (dBFS of the BAND's detector level) */
    double   ratio;           /* 1 .. 100 (1: the curve does nothing) */
    double   knee_db;         /* 0 .. 24 (0: hard knee) */
    double   attack_ms;       /* 0.05 .. 200 */
    double   release_ms;      /* 5 .. 5000 */
    double   max_reduction_db;/* 0 .. 40: the band is never turned down by more */
} ptts_deesser_opts;
int  ptts_dsp_ext_set_deesser(ptts_dsp_ext* e, const ptts_deesser_opts* d);
int  ptts_deess_apply(const ptts_deesser_opts* d, float* samples, int64_t n);
int  ptts_deess_band(const ptts_deesser_opts* d, const float* in, int64_t n, float* band);
int  ptts_deess_rows(ptts_model* m, const ptts_deesser_opts* const* d, const float* const* in, const int64_t* n, int32_t rows, float* const* out);

/* Look-ahead peak limiter at 24 kHz: float64, no recurrence that is not a scan.  With c = 10^(ceiling_db / 20),
 * d = 10^(drive_db / 20), L = lrint(lookahead_ms * 24) samples (6 .. 120) and rho = exp(-1 / (release_ms * 24)), per row x[0, n):
 *     a[i] = |x[i]| d                                  the level (a NaN never wins and reads as 0)
 *     m[i] = max a[j], j in [i, i + L]                  the look-ahead peak hold (samples at or beyond n read as 0)
 *     p[i] = max(m[i], rho p[i-1]),  p[-1] = 0          the release
 *     r[i] = p[i] > c ? (float)(c / p[i]) : 1.0f        the required gain, one IEEE division rounded once to f32;  r[i] = r[0] for i < 0
 *     g[i] = (r[i] + r[i-1] + ... + r[i-L]) / (L + 1)   the smoothed gain: a float64 sum in exactly that order, times the double 1.0 / (L + 1)
 *     y[i] = (float)((x[i] d) g[i])
 * The release is evaluated as a blocked scan on the compressor's grid (runs of 30 samples, tiles of 1920; csrc/limiter.h), and that form is
 * the definition: host and device run the same functions and give the same bits.  It agrees with the sample-by-sample statement to one f32
 * step at the row's peak.
 *   - Every term of g[i] comes from a hold window that contains sample i, so |y[i]| <= c (1 + 2^-22): the ceiling holds for every sample.
 *   - Where the driven signal has been under the ceiling for long enough (every p in [i - L, i] at or under c), g[i] is 1 (or the double
 *     just below it), and with drive_db = 0 the sample comes back bit for bit: the limiter engages only where it must.
 *   - y[i] depends on x[0, i + L] only.
 *   - It limits SAMPLE peaks at 24 kHz; inter-sample peaks, rate conversion and quantisation come behind it.  The static true-peak ceiling
 *     may follow it and then has only the inter-sample remainder to take off.
 * Non-finite samples are not treated specially: a NaN sample comes out as NaN and touches nothing else; an infinite sample holds p at +inf
 * from L samples in front of it to the end of the row, so the gain falls to 0 in front of it, the sample itself comes out as NaN (inf * 0)
 * and every later finite sample as a zero (csrc/limiter.h).
 * ptts_limiter_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_dsp_ext_set_limiter attaches the limiter to a live handle of ptts_dsp_ext_create (l NULL: off again); a handle that is not live is
 * PTTS_EINVAL and is not read.  Set it before requests name the handle, not while they run.  Refused together with pcm_callback like every
 * other switch of `ext`.
 * ptts_limit_apply: the limiter over samples[0, n) in place.  Host.
 * ptts_limit_rows: the same on rows of host samples on the device, by the kernels a request's limiter runs; shaped like ptts_compress_rows.
 * l[i] NULL copies row i; in[i] == out[i] is allowed; a bad row is named. */
typedef struct ptts_limiter_opts {
    uint32_t size;          /* sizeof(ptts_limiter_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  reserved;      /* 0 */
    double   ceiling_db;    /* -60 .. 0 (dBFS, sample peak) */
    double   lookahead_ms;  /* 0.25 .. 5: the delay-free look-ahead and the length of the gain's attack ramp */
    double   release_ms;    /* 5 .. 5000 */
    double   drive_db;      /* 0 .. 24: gain in front of the limiter (0: none) */
} ptts_limiter_opts;
int  ptts_dsp_ext_set_limiter(ptts_dsp_ext* e, const ptts_limiter_opts* l);
int  ptts_limit_apply(const ptts_limiter_opts* l, float* samples, int64_t n);
int  ptts_limit_rows(ptts_model* m, const ptts_limiter_opts* const* l, const float* const* in, const int64_t* n, int32_t rows, float* const* out);

/* Joined synthesis: a text's chunks as ONE utterance.  The reference's Service.Synthesize appends the chunks' PCM
 * (internal/tts/service.go:107-153) and its CLI runs the post-processing once over the concatenation (cmd/pockettts/synth.go:361-390); the
 * request's own `dsp`, `loudness` and egress above work per request.  Here the join, the chain over the whole text and the egress stay on the
 * device, and one result comes back.
 *
 * The join.  Parts x_0 .. x_(R-1) of n_i samples at 24 kHz, in order, R from 1 to 4096, n_i >= 0, the joined length below 2^31.  With
 *     G = (int64)(gap_ms / 1000 * 24000),   K = (int64)(crossfade_ms / 1000 * 24000)
 * (the expression of ptts_dsp_apply's fades; each a finite value from 0 to 2000 ms, at most one of the two above 0):
 *   - gap: G zeros between consecutive parts, none in front of the first part or behind the last;
 *   - crossfade: at the seam between parts i and i+1, K_i = min(K, n_i / 2, n_(i+1) / 2) (integer divisions: two seams never touch the same
 *     sample), the last K_i samples of part i overlap the first K_i of part i+1 = b, and for j in [0, K_i)
 *         out = a[n_i - K_i + j] * ((float)(K_i - 1 - j) / (float)K_i) + b[j] * ((float)j / (float)K_i)
 *     -- two f32 divisions, two f32 products, one f32 sum, each rounded once, nothing fused: ptts_dsp_apply's fade out of the tail plus its
 *     fade in of the head;
 *   - every other sample is copied bit for bit (NaN and infinity pass);
 *   - offset_0 = 0, offset_(i+1) = offset_i + n_i + G - K_i is where a part's first sample lies; the joined length is offset_(R-1) + n_(R-1).
 * ptts_join_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field or a broken limit is
 * PTTS_EINVAL and the error names it.
 * ptts_join_length: the joined length of parts of n[0 .. rows) samples, or -PTTS_EINVAL; offsets (optional, [rows]) receives the part offsets.
 *     Only size, gap_ms and crossfade_ms of the options are read.  Host.
 * ptts_join: the join of in[0 .. rows) into out[0, ptts_join_length): the statement of the result.  Host.
 * ptts_join_rows: the same on the device, by the kernel ptts_generate_joined runs (k_join), shaped like ptts_dsp_rows: one upload, one launch
 *     per 256 parts, one download.  It gives ptts_join's bits.
 *
 * ptts_generate_joined: the n requests run exactly as ptts_generate runs them (the same admission checks, groups of max_batch, step callbacks
 * and cancel flags), in text order; every group's decoded audio is joined on the device into one row for the text; after the last group the
 * chain of `dsp` and `loudness` runs ONCE over the joined audio (every stage as documented for ptts_request.dsp: the host statement is the
 * host chain on ptts_join of the chunks' audio) and the egress (sample_rate, pcm_format) delivers ONE result: out->n_samples counts samples of
 * the joined audio at the output rate, out->n_frames is the sum of the chunks' frames, out->eos_step is -1.  parts (optional, [n]) receives
 * each chunk's offset and length in the joined 24 kHz audio, its frame count, EOS step and status: captions and progress.
 * PTTS_EINVAL, nothing launched, naming the field: a request with a non-zero dsp, loudness, sample_rate, pcm_format, pcm_callback or
 * want_latents (these belong in the join options); requests that differ in their resolved lsd_steps (the groups would leave text order); n
 * outside 1 .. 4096; step budgets that allow 2^31 samples or more; and everything ptts_generate refuses, in its own words.  A chunk that is
 * cancelled or runs past the decoder's reach fails the whole call with that chunk's code: *out is zeroed and parts[i].status names the chunk
 * (chunks of later groups have not run: status 0, no frames). */
typedef struct ptts_join_opts {
    uint32_t size;          /* sizeof(ptts_join_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  pcm_format;    /* PTTS_PCM_*: the egress of the joined audio */
    int32_t  sample_rate;   /* 0: 24000; as ptts_request.sample_rate */
    int32_t  loudness;      /* 0: off; as ptts_request.loudness, over the joined audio */
    const ptts_dsp_opts* dsp;   /* NULL, or the chain, run ONCE over the joined audio (borrowed for the call) */
    double   gap_ms;        /* 0 .. 2000: silence between consecutive parts */
    double   crossfade_ms;  /* 0 .. 2000: overlap of consecutive parts; not together with gap_ms */
} ptts_join_opts;
typedef struct ptts_join_part {
    int64_t offset, n_samples;   /* at 24 kHz, in the joined audio (in front of the egress) */
    int32_t n_frames, eos_step, status, reserved;
} ptts_join_part;
int64_t ptts_join_length(const int64_t* n, int32_t rows, const ptts_join_opts* opts, int64_t* offsets /* optional [rows] */);
int  ptts_join(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* opts, float* out);
int  ptts_join_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* opts, float* out);
int  ptts_generate_joined(ptts_model* m, const ptts_request* reqs, int32_t n, const ptts_join_opts* o, ptts_result* out,
                          ptts_join_part* parts /* [n], optional */);

/* Streamed joined synthesis: ptts_generate_joined that hands a text's audio over group by group, so a long text is heard after its first
 * group and not after its last.  A joined call with one request is the single-utterance form.
 *   Groups.  The first group holds parts [0, g0), g0 = first_group ? first_group : max_batch; the following groups hold max_batch parts each,
 *     in text order.  Each group runs exactly as ptts_generate_joined runs its groups: the decode after the loop, the trim and the tempo per
 *     part, k_join.
 *   The result.  With first_group == 0, *out and parts equal those of ptts_generate_joined(m, reqs, n, o, ...) in every byte, callback or not.
 *     With another first_group they are the host statement (the host chain on ptts_join of the chunks' audio) on the chunks' audio as
 *     ptts_generate calls over the same groups give it.
 *   Hand-overs.  A_g: the joined length at 24 kHz after group g; K = (int64)(crossfade_ms / 1000 * 24000), Fo = (int64)(fade_out_ms / 1000 *
 *     24000), neither clamped by a length.  Behind a group that is not the last
 *         P_g = max(P_(g-1), floor(max(0, A_g - max(K, Fo)) / 1920) * 1920)          (P_(-1) = 0; ptts_join_stream_ready(o, A_g) is the floor term)
 *     and behind the last group P = A.  Held back are the tail the next group's seam fades where it lies ([A_g - k, A_g), k <= K) and whatever
 *     the fade out could reach, which needs the final length; the floor keeps every cut on the grid of the chain's blocked scans (1920
 *     samples, one decoder frame).  While A_g is still below the fade in's length nothing is handed over either (that fade is clamped by the
 *     final length): P_g = P_(g-1).  Window g is [P_(g-1), P_g) of the 24 kHz audio: the chain runs over it with the state the window in front
 *     left, and gives the bits of the chain run once.  At 24 kHz in f32 or PCM16 the hand-over is that range; at another rate or in G.711 it is
 *     the outputs [o_(g-1), o_g), o_g the outputs whose filter support lies inside the first P_g samples, as for a streamed request, and
 *     behind the last group all of them.  pcm_callback(pcm_user, offset, count, samples): offset and count in output samples; a window with
 *     nothing new makes no call; the hand-overs tile [0, out->n_samples) in order, each sample once.  `samples` points into the buffer *out
 *     will own, allocated up front for what the step budgets allow.  Callbacks come from a library thread, as a streamed request's, and must
 *     not call into the library.  A group's hand-over is queued before the next group's prefill is issued; the host does not wait for it.
 *   The chain of a call with a callback: compressor, DC block, equaliser, fade in, fade out, in the documented order; around them the parts'
 *     trim and tempo, gap or crossfade, every pcm_format and sample_rate.  PTTS_EINVAL, nothing launched, naming the field: normalize,
 *     loudness and the true-peak ceiling (they need the whole text) and the limiter (its look-ahead is left for a later change), e.g.
 *     "join: stream: loudness needs the whole text; it cannot be combined with pcm_callback".  With pcm_callback NULL nothing is refused beyond
 *     what ptts_generate_joined refuses, and nothing is handed over early: the call differs from it by first_group alone.
 *   Failure.  A chunk that is cancelled or runs past the decoder's reach fails the call as it fails ptts_generate_joined: *out is zeroed, its
 *     buffer freed, parts[i].status names the chunk.  Audio handed over before is the true beginning of the text; the pointers of those
 *     hand-overs die when the call returns.
 *   Also PTTS_EINVAL, naming the field: so NULL, a bad size (the rules of ptts_dsp_ext_opts.size), a first_group outside 0 .. max_batch.
 * ptts_join_stream_ready: the samples of the joined 24 kHz audio that are final once `joined` of them have been joined and more parts follow:
 *     floor(max(0, joined - max(K, Fo)) / 1920) * 1920, Fo of o->dsp (NULL: 0).  -PTTS_EINVAL for bad options or a negative `joined`.  Host. */
typedef struct ptts_join_stream_opts {
    uint32_t size;            /* sizeof(ptts_join_stream_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  first_group;     /* 0: max_batch; else 1 .. max_batch: parts in the FIRST group (first audio sooner); later groups hold max_batch */
    ptts_pcm_callback pcm_callback; void* pcm_user;   /* NULL: nothing is handed over early */
} ptts_join_stream_opts;     /* 24 bytes */
int  ptts_generate_joined_streamed(ptts_model* m, const ptts_request* reqs, int32_t n, const ptts_join_opts* o,
                                   const ptts_join_stream_opts* so, ptts_result* out, ptts_join_part* parts /* [n], optional */);
int64_t ptts_join_stream_ready(const ptts_join_opts* o, int64_t joined);

/* Silence control of the parts of a joined text: a part's silent head and tail cut off and its over-long pauses
 * capped, per part and IN FRONT of the join, so that what a listener hears between two sentences is the join's gap or crossfade and not the
 * chunks' own lead-in and trailing frames around it; a joined call with one request is the single-utterance form (no lead-in latency).  The
 * order of a joined call: trim per part -> join -> the chain of `dsp` and `loudness` once -> egress.
 *
 * On a row x[0, n) at 24 kHz, n below 2^31, with
 *     t = (float)pow(10, threshold_db / 20),   H = (int64)(pad_ms / 1000 * 24000),   M = (int64)(max_pause_ms / 1000 * 24000)
 * a sample is LOUD when fabsf(x) > t (a NaN never is, an infinity is, |x| == t is not), and L is the ascending set of loud indices:
 *   - no loud sample: the row comes back whole; lo = 0, hi = n, n_out = n, cuts = 0, speech = 0;
 *   - otherwise speech = 1 and, with `edges`, lo = max(0, L.first - H) and hi = min(n, L.last + 1 + H); without, lo = 0 and hi = n;
 *   - pauses, when M > 0: consecutive loud indices u < v with q = v - u - 1 > M lose the samples [u + 1 + (M - M / 2), v - M / 2) (integer
 *     division): the first ceil(M / 2) and the last floor(M / 2) samples of the pause stay; `cuts` counts such pairs;
 *   - every sample of [lo, hi) that is not removed is output, in order, moved as its 32 bits: n_out = hi - lo - sum(q - M).
 * Integer comparisons and copies only: the host and the device give the same bits, and no tolerance applies.  The lower bound of 20 ms on
 * max_pause_ms is one period of a 50 Hz voice: the quiet samples between the peaks of voiced speech are never a pause.
 * ptts_trim_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it; edges == 0 with max_pause_ms == 0 is refused too ("trim: nothing switched on").
 * ptts_trim_plan: what the trim makes of x[0, n), into *info; writes nothing else.  Host.
 * ptts_trim_apply: the trimmed row into out, which holds n floats (the first info->n_out are written; out == in is allowed); info is optional.
 *     Host: the statement of the result.
 * ptts_trim_rows: the same on rows of host samples on the device, by the kernels ptts_generate_joined runs (k_trim_mark, k_trim_carry,
 *     k_trim_store), shaped like ptts_limit_rows: one upload, one launch sequence per 256 rows, one download.  t[i] NULL copies row i (its record
 *     says lo = 0, hi = n_out = n[i], cuts = 0, speech = 0); n[i] >= 0; in[i] == out[i] is allowed; out[i] holds n[i] floats; info ([rows]) is
 *     required; a bad row is named.
 * ptts_dsp_ext_set_trim attaches the trim to a live handle of ptts_dsp_ext_create (t NULL: off again); a handle that is not live is PTTS_EINVAL
 *     and is not read.  Set it before calls name the handle, not while they run.  It is served where the lengths are decided on the host behind
 *     the decode: by ptts_generate_joined, whose join options' `dsp` names the handle -- every part is trimmed in front of the join,
 *     parts[i].offset and parts[i].n_samples count the trimmed audio, parts[i].n_frames and out->n_frames still count decoded frames, and the
 *     chain of that `dsp` runs over the joined audio as without a trim (the trim is a stage per part, not a stage of the chain).  Everywhere a
 *     row's length is fixed before the decode it is refused with PTTS_EINVAL, nothing launched ("dsp: ext: trim changes a row's length ..."):
 *     a ptts_request.dsp whose ext carries a trim (ptts_generate, the dispatcher, the continuous engine, streaming) and ptts_dsp_rows. */
typedef struct ptts_trim_opts {
    uint32_t size;           /* sizeof(ptts_trim_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  edges;          /* 0 or 1: trim the row's silent head and tail */
    double   threshold_db;   /* -120 .. 0 (dBFS): a sample is loud when fabsf(x) > (float)pow(10, threshold_db / 20) */
    double   pad_ms;         /* 0 .. 500: audio kept in front of the first and behind the last loud sample */
    double   max_pause_ms;   /* 0: pauses untouched; else 20 .. 5000: the longest pause that stays */
} ptts_trim_opts;
typedef struct ptts_trim_info {
    int64_t lo, hi;          /* the edges: what lies in [lo, hi) and in no cut is output */
    int64_t n_out;           /* samples of the trimmed row */
    int64_t cuts;            /* pauses that were shortened */
    int32_t speech;          /* 1: the row has a loud sample; 0: it came back whole */
    int32_t reserved;
} ptts_trim_info;
int  ptts_trim_plan(const ptts_trim_opts* t, const float* x, int64_t n, ptts_trim_info* info);
int  ptts_trim_apply(const ptts_trim_opts* t, const float* in, int64_t n, float* out, ptts_trim_info* info /* optional */);
int  ptts_trim_rows(ptts_model* m, const ptts_trim_opts* const* t, const float* const* in, const int64_t* n, int32_t rows, float* const* out,
                    ptts_trim_info* info /* [rows] */);
int  ptts_dsp_ext_set_trim(ptts_dsp_ext* e, const ptts_trim_opts* t);

/* The speaking rate of the parts of a joined text: a tempo change that keeps the pitch, per part, behind the trim and
 * IN FRONT of the join.  The order of a joined call: trim per part -> tempo per part -> join -> the chain of `dsp` and `loudness` once ->
 * egress.  ("tempo", not "rate": a rate is a sample rate in this library.)
 *
 * On a row x[0, n) at 24 kHz, n below 2^31 - 240, with s = speed_permille (500 .. 2000; 1000: unchanged, 2000: twice as fast and half as
 * long), the hop Hs = 480 (20 ms) and the search radius D = 240 (+-10 ms).  Every index is an integer; a sample outside [0, n) reads as 0.0f
 * and its quantised value as 0.
 *   - length: n_out = (n * 1000) / s in int64 with integer division, F = ceil(n_out / Hs) hops; n == 0 or n_out == 0 is an empty row;
 *   - quantised view: q[i] = 0 for a NaN, else (int32)(clamp(x[i], -1, 1) * 32767.0f), truncated towards zero; infinities clamp;
 *   - positions: p_0 = 0, and for hop k >= 1 with a_k = (k * Hs * s) / 1000 (where the input should be read) and c_k = p_(k-1) + Hs (where
 *     the previous hop's segment continues):  S(d) = sum over j in [0, Hs) of |q[a_k + d + j] - q[c_k + j]| for d in [-D, D] (it fits an
 *     int32), d* minimises (S(d), |d|, d > 0) lexicographically -- the least S, then the least |d|, then the negative one -- and
 *     p_k = a_k + d*.  A position may be negative or run past n;
 *   - output, m in [0, n_out), k = m / Hs, j = m % Hs:  k == 0 or p_k == c_k (the hop continues its predecessor): out[m] = x[p_k + j], moved
 *     as its 32 bits; otherwise out[m] = x[c_k + j] * ((float)(Hs - j) / (float)Hs) + x[p_k + j] * ((float)j / (float)Hs): two f32
 *     divisions, two f32 products and one f32 sum, each rounded once, nothing fused.
 * Every decision is integer arithmetic: the host and the device choose the same positions and give the same bits, and no tolerance applies.
 * s == 1000 returns the row bit for bit (d = 0 has S = 0 and the least |d|: every hop continues).  The continuation has S = 0 whenever it lies
 * inside the search window, so stretches of the input pass through untouched between splices.  The last hop of a slowed row may fade into
 * the zeros behind n.  Audio above +-1 is clamped in the search only, never in the output.  n stays below 2^31 - 240 so that a position
 * (at most n + 239) is an int32.
 * ptts_tempo_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_tempo_length: n_out for a row of n samples, or -PTTS_EINVAL.  Host.
 * ptts_tempo_plan: the F positions of x[0, n)'s hops into positions (F = ceil(ptts_tempo_length / 480)); for tests and captions.  Host.
 * ptts_tempo_apply: the time-scaled row into out, which holds ptts_tempo_length floats and is not in.  Host: the statement of the result.
 * ptts_tempo_rows: the same on rows of host samples on the device, by the kernels ptts_generate_joined runs (k_tempo_plan, k_tempo_store),
 *     shaped like ptts_trim_rows: one upload, one launch of each kernel per 256 rows, one download.  t[i] NULL copies row i (n_out[i] = n[i]);
 *     n[i] >= 0; out[i] holds ptts_tempo_length(t[i], n[i]) floats and is not in[i] (with t[i] NULL it holds n[i] and may be); n_out ([rows])
 *     is required; a bad row is named.
 * ptts_dsp_ext_set_tempo attaches the tempo to a live handle of ptts_dsp_ext_create (t NULL: off again); a handle that is not live is
 *     PTTS_EINVAL and is not read.  Set it before calls name the handle, not while they run.  It is served by ptts_generate_joined, whose join
 *     options' `dsp` names the handle: parts[i].offset and parts[i].n_samples count the time-scaled audio, parts[i].n_frames and out->n_frames
 *     still count decoded frames, and a text whose step budgets, slowed, allow 2^31 samples or more is refused.  Everywhere a row's length is
 *     fixed before the decode it is refused with PTTS_EINVAL, nothing launched ("dsp: ext: tempo changes a row's length ..."): a
 *     ptts_request.dsp whose ext carries a tempo (ptts_generate, the dispatcher, the continuous engine, streaming) and ptts_dsp_rows. */
typedef struct ptts_tempo_opts {
    uint32_t size;             /* sizeof(ptts_tempo_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  speed_permille;   /* 500 .. 2000: 1000 leaves the row as it is, 1250 is a quarter faster, 800 a quarter slower */
    int32_t  reserved[2];      /* 0 */
} ptts_tempo_opts;
int64_t ptts_tempo_length(const ptts_tempo_opts* t, int64_t n);
int  ptts_tempo_plan(const ptts_tempo_opts* t, const float* x, int64_t n, int32_t* positions /* [F] */);
int  ptts_tempo_apply(const ptts_tempo_opts* t, const float* in, int64_t n, float* out);
int  ptts_tempo_rows(ptts_model* m, const ptts_tempo_opts* const* t, const float* const* in, const int64_t* n, int32_t rows, float* const* out,
                     int64_t* n_out /* [rows] */);
int  ptts_dsp_ext_set_tempo(ptts_dsp_ext* e, const ptts_tempo_opts* t);

/* The pitch of the parts of a joined text: per part, behind the trim and in front of the tempo.  The order of a joined
 * call: trim per part -> pitch resample per part -> tempo at the effective speed per part -> join -> the chain of `dsp` and `loudness` once ->
 * egress.  A pitch change at constant duration is a resampling by the pitch ratio and a tempo change that takes the length back.  FORMANTS MOVE
 * WITH THE PITCH: every frequency of the part is scaled, so a large shift changes the voice's character, not only its height -- unless the
 * handle also carries the option of ptts_formant_opts, below, which keeps them in place.
 *
 * On a part x[0, n) at 24 kHz with p = pitch_permille (500 .. 2000; 1000: unchanged, 1100: 10 % higher, SSML's "+10%"; 2000: an octave up) and
 * s the tempo's speed_permille (1000 when there is no tempo) the stage is two steps.  Every index is an integer.
 *   - resample: z = x read at step p / 1000, so frequencies scale by p / 1000; its length is n_r = (n * 1000 + p - 1) / p (0 for n == 0).
 *     p == 1000: z is x, nothing is computed.
 *   - tempo at the effective speed E = (1000 * s + p / 2) / p, integer division: the tempo's statement above runs on z with speed E, unchanged.
 *     E outside 500 .. 2000 is PTTS_EINVAL, and the error names both fields and both values (at s == 1000 every p is served; at s == 500 p may
 *     run up to 1001, at s == 2000 from 1000 up).  E == 1000 is the identity and nothing is computed.  The final length is
 *     ptts_tempo_length at E of n_r.  For parts of one second and more it differs from (n * 1000) / s by at most 0.1 % of it (shorter parts are
 *     bound by the rounding of the lengths).  Resampling first keeps the tempo's hops at 20 ms of the FINAL audio whatever p is.
 * The resample is band-limited interpolation from one prototype table with linearly interpolated coefficients, so that any p is served without
 * a filter design of its own.  R = 256 table steps per input sample, fc = 0.45, W = 80 / 3 samples, Kaiser beta 8.6:
 *   - table: h[q] = (float)(2 fc sinc(2 fc q / R) I0(beta sqrt(1 - (q / (R W))^2)) / I0(beta)) where 3 q < 80 R, and 0 beyond; computed in
 *     float64 and rounded once; 6828 entries.  hd[q] = h[q + 1] - h[q], one f32 subtraction of the rounded entries (h[6828] counts as 0).
 *   - per row: D = max(1000, p) (above 1000 the filter widens, against aliasing) and g = (float)(1000.0 / D).
 *   - output j in [0, n_r), with c = j * p in int64, sums over the inputs i with 3 |c - 1000 i| < 80 D in ascending i:  a = |c - 1000 i|,
 *     q = (a * R) / D, r = (a * R) % D, frac = (float)r / (float)D (one IEEE f32 division), coef = fmaf(hd[q], frac, h[q]),
 *     acc = fmaf(x[i], coef, acc), starting from 0.0f; x outside [0, n) reads as 0.0f.  Then out[j] = acc * g, one f32 product.
 * Nothing else is rounded and nothing is contracted that the statement does not contract: the host and the device give the same bits.  A NaN
 * or an infinity reaches every output whose support holds it; which NaN bits come out is the processor's choice and not fixed.  Rows whose
 * resampled or final length would reach 2^31 - 240 are refused.
 * ptts_pitch_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_pitch_speed: E for the pair, or -PTTS_EINVAL; t NULL means s = 1000.  Host.
 * ptts_pitch_resample_length: n_r for a row of n samples, or -PTTS_EINVAL.  Host.
 * ptts_pitch_resample: the resample alone into out, which holds ptts_pitch_resample_length floats and is not in.  Host: the statement of
 *     k_pitch_resample.
 * ptts_pitch_length: the final length of a row of n samples, or -PTTS_EINVAL.  Host.
 * ptts_pitch_apply: the whole stage into out, which holds ptts_pitch_length floats and is not in: ptts_tempo_apply at E over
 *     ptts_pitch_resample, by definition.  p == 1000 without a tempo returns the row bit for bit.  Host: the statement of the result.
 * ptts_pitch_table: the prototype table: *h and *hd point at `*entries` (6828) floats each, owned by the library.  Any argument may be NULL.  Host.
 * ptts_pitch_rows: the whole stage on rows of host samples on the device, by the kernels ptts_generate_joined runs (k_pitch_resample, then
 *     k_tempo_plan and k_tempo_store), shaped like ptts_tempo_rows: one upload, one launch sequence per 256 rows, one download.  p[i] NULL
 *     means the tempo t[i] alone, as ptts_tempo_rows; both NULL copies row i (n_out[i] = n[i]).  n[i] >= 0; out[i] holds
 *     ptts_pitch_length(p[i], t[i], n[i]) floats and is not in[i] (with both NULL it holds n[i] and may be); the arrays p and t and n_out
 *     ([rows]) are required; a bad row is named.
 * ptts_dsp_ext_set_pitch attaches the pitch to a live handle of ptts_dsp_ext_create (p NULL: off again); a handle that is not live is
 *     PTTS_EINVAL and is not read.  Set it before calls name the handle, not while they run.  It is served by ptts_generate_joined and
 *     ptts_generate_joined_streamed, whose join options' `dsp` names the handle: the pair (s, p) is resolved to E once, before anything
 *     launches; parts[i].offset and parts[i].n_samples count the final audio, parts[i].n_frames and out->n_frames still count decoded
 *     frames; the bound on the joined length takes, per part, the largest of its step budget, its resampled length and its final length, and a
 *     text that could reach 2^31 samples is refused.  Without a pitch nothing of this is allocated, uploaded or launched.  Everywhere a row's
 *     length is fixed before the decode it is refused with PTTS_EINVAL, nothing launched ("dsp: ext: pitch changes a row's length ..."): a
 *     ptts_request.dsp whose ext carries a pitch (ptts_generate, the dispatcher, the continuous engine, streaming) and ptts_dsp_rows. */
typedef struct ptts_pitch_opts {
    uint32_t size;             /* sizeof(ptts_pitch_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  pitch_permille;   /* 500 .. 2000: 1000 leaves the row as it is, 1100 is 10 % higher, 2000 an octave up; formants move with it */
    int32_t  reserved[2];      /* 0 */
} ptts_pitch_opts;
int32_t ptts_pitch_speed(const ptts_pitch_opts* p, const ptts_tempo_opts* t);
int64_t ptts_pitch_resample_length(const ptts_pitch_opts* p, int64_t n);
int  ptts_pitch_resample(const ptts_pitch_opts* p, const float* in, int64_t n, float* out);
int64_t ptts_pitch_length(const ptts_pitch_opts* p, const ptts_tempo_opts* t, int64_t n);
int  ptts_pitch_apply(const ptts_pitch_opts* p, const ptts_tempo_opts* t, const float* in, int64_t n, float* out);
int  ptts_pitch_table(const float** h, const float** hd, int32_t* entries);
int  ptts_pitch_rows(ptts_model* m, const ptts_pitch_opts* const* p /* [rows] */, const ptts_tempo_opts* const* t /* [rows] */,
                     const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out /* [rows] */);
int  ptts_dsp_ext_set_pitch(ptts_dsp_ext* e, const ptts_pitch_opts* p);

/* Keep the formants: the pitch of a part without its vocal-tract resonances moving with it.  The part's spectral
 * envelope is estimated by linear prediction, the part is flattened (whitened) with it, only the flat residual goes through the pitch's resampler,
 * and the original envelope is put back on the resampled residual; the tempo follows as it does without the option.  The order of a joined call
 * with it: trim per part -> [whiten -> the pitch's resample of the residual -> shape] -> tempo at the effective speed E -> join -> chain ->
 * egress.  The bracket replaces the bare resample; every length stays: ptts_pitch_resample_length, ptts_pitch_speed and ptts_pitch_length hold.
 *
 * Constants: hop 240, window 720, order 24, warm-up 720 samples; bandwidth expansion 0.99; lag window 60 Hz; white-noise factor 1.0001.  On a
 * part x[0, n) at 24 kHz with the pitch p; samples outside a row read as 0.0f:
 *   - frames: K = ceil(n / 240); frame f looks at x[240 f - 240 + j], j in [0, 720): its centre is 240 f + 120.
 *   - analysis, float64, per frame: v[j] = (double)x * w[j], w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / 720).  r[l], l = 0 .. 24, is one fma chain from
 *     0.0 over ascending j = l .. 719 of v[j] * v[j - l].  r[0] not finite or not > 0: the frame is the identity (a[1 .. 24] = 0).  Otherwise
 *     r[l] *= exp(-0.5 (2 pi 60 l / 24000)^2) and r[0] *= 1.0001.  Levinson-Durbin, stage i = 1 .. 24, E = r[0] at the start: acc = r[i], then over
 *     ascending j = 1 .. i - 1 acc = fma(a[j], r[i - j], acc); k = -acc / E; the new a[j] = a[j] + k * a[i - j] for j below i (a product, then a
 *     sum) and a[i] = k; E = E * (1 - k * k), nothing contracted.  A k that is not finite or has |k| >= 1, or an E that is not > 0, makes the frame
 *     the identity.  a32[k] = (float)(a[k] * 0.99^k).  The three tables (w, the lag window, 0.99^k) are made once in float64.  K x 24 floats a part.
 *   - the pair of a source time tau: b = tau - 120, f0 = floor(b / 240), rho = b - 240 f0, fa = clamp(f0, 0, K - 1), fb = clamp(f0 + 1, 0, K - 1),
 *     u = (float)rho / 240.0f (one IEEE f32 division); mix(A, B) = A * (1.0f - u) + B * u: one difference, two products, one sum, each rounded
 *     once, nothing fused.
 *   - whiten: E_f[i] is one f32 chain: acc = x[i], then for k = 1 .. 24 ascending acc = fmaf(a32_f[k], x[i - k], acc); e[i] = mix(E_fa[i], E_fb[i])
 *     with tau = i, for i in [0, n).
 *   - resample: e' = ptts_pitch_resample of e at p, unchanged: n_r samples.
 *   - shape: output j lies in tile t = j / 240, which starts its recursions at m0 = 240 t - 720.  For a frame f, Y[m] for m >= m0 is one f32 chain:
 *     acc = e'[m] (0.0f outside [0, n_r)), then for k = 1 .. 24 ascending acc = fmaf(-a32_f[k], Y[m - k], acc), with Y[m] = 0 for m < m0.
 *     out[j] = mix(Y_fa[j], Y_fb[j]) with tau = (j * p) / 1000 in int64.  A tile needs at most four frames (p = 1500).
 *   - tempo: the tempo's statement at E on out, unchanged.
 * The recursive filter is bounded on purpose: every tile of 240 outputs restarts from zero state 720 samples earlier, so tiles are independent.
 * The host and the device run the same chains in the same order and give the same bits (outside NaNs, whose bits are the processor's).
 *   - A NaN at sample i makes identity frames of the three frames whose windows hold it.  It reaches the residual samples i .. i + 24, and outputs
 *     no further than 720 + 240 samples plus the resampler's support behind its image; nothing else of the row is touched.
 *   - Peaks may grow: there is no gain control here; the chain's limiter and ceiling follow.
 *   - Below p = 1000 the residual is band-limited to p / 1000 of the band, as the plain pitch is.
 * The option is served for p from 800 to 1500; outside it is PTTS_EINVAL, and the error names both fields and both values (at p = 667 a float64
 * prototype of this statement no longer kept the envelope nearer to its place than it moved).  p == 1000, or no pitch at all, means nothing is
 * computed and the part comes back as without the option.
 * ptts_formant_opts is size-versioned by the rules of ptts_dsp_ext_opts.size (every field below is required).  A bad field is PTTS_EINVAL and the
 * error names it.
 * ptts_formant_frames: K for a row of n samples, or -PTTS_EINVAL.  Host.
 * ptts_formant_analyse: the K x 24 coefficients a32[1 .. 24] of x[0, n).  Host: the statement of k_formant_analyse.
 * ptts_formant_whiten: e[0, n) from the coefficients and x; e is not x.  Host: the statement of k_formant_whiten.
 * ptts_formant_shape: out[0, n_r) from the coefficients of the part of n samples, p and the resampled residual e_r[0, n_r); out is not e_r.  Host:
 *     the statement of k_formant_shape.
 * ptts_formant_apply: the whole stage into out, which holds ptts_pitch_length(p, t, n) floats and is not in.  keep == 0 or p == 1000: exactly
 *     ptts_pitch_apply.  Host: the statement of the result.
 * ptts_formant_rows: the whole stage on rows of host samples on the device, shaped like ptts_pitch_rows.  f[i] NULL (or keep 0): row i exactly
 *     as ptts_pitch_rows.  The arrays f, p, t and n_out ([rows]) are required; a bad row is named.
 * ptts_dsp_ext_set_formant attaches the option to a live handle of ptts_dsp_ext_create (f NULL: off again); a handle that is not live is
 *     PTTS_EINVAL and is not read.  It is served where the pitch is: ptts_generate_joined and ptts_generate_joined_streamed resolve the pair
 *     (option, pitch) before anything launches.  Without the option nothing of this is allocated, uploaded or launched. */
typedef struct ptts_formant_opts {
    uint32_t size;             /* sizeof(ptts_formant_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  keep;             /* 0: formants move with the pitch; 1: they stay */
    int32_t  reserved[2];      /* 0 */
} ptts_formant_opts;
int32_t ptts_formant_frames(int64_t n);
int  ptts_formant_analyse(const float* x, int64_t n, float* coeffs /* [K][24] */);
int  ptts_formant_whiten(const float* coeffs, const float* x, int64_t n, float* e);
int  ptts_formant_shape(const float* coeffs, int64_t n, int32_t pitch_permille, const float* e_r, int64_t n_r, float* out);
int  ptts_formant_apply(const ptts_formant_opts* f, const ptts_pitch_opts* p, const ptts_tempo_opts* t, const float* in, int64_t n, float* out);
int  ptts_formant_rows(ptts_model* m, const ptts_formant_opts* const* f /* [rows] */, const ptts_pitch_opts* const* p /* [rows] */,
                       const ptts_tempo_opts* const* t /* [rows] */, const float* const* in, const int64_t* n, int32_t rows, float* const* out,
                       int64_t* n_out /* [rows] */);
int  ptts_dsp_ext_set_formant(ptts_dsp_ext* e, const ptts_formant_opts* f);

/* Per-part prosody of a joined text: a list of one ptts_part_opts per part states that part's trim, pitch (with or
 * without its formants), tempo and volume, and the seam BEHIND it -- a longer break after a heading, one sentence slower, a quote at another
 * pitch, an aside quieter.  The order of such a call: trim -> pitch resample (formants kept where asked) -> tempo at the effective speed ->
 * volume -> join -> the chain of `dsp` / `loudness` once -> egress; the pair (tempo, pitch) is resolved to E per part before anything
 * launches, and a refusal names the part index and both values.
 *   The list.  po[0 .. rows); every element carries the same `size`, which is also the distance in bytes from one element to the next (the
 *     rules of ptts_dsp_ext_opts.size apply to each element).  The structs a part's pointers name are borrowed for the call.
 *   Seams.  For the seam behind part i: gap_ms and crossfade_ms both negative -- the pair of ptts_join_opts; otherwise a negative field reads
 *     as 0, each is a value from 0 to 2000 and at most one is above 0; NaN is refused.  The last part's fields are range-checked and otherwise
 *     unused.  G and K of the join's statement become G_i and K_i = min(K_i, n_i / 2, n_(i+1) / 2) of the seam behind part i.
 *   Volume.  gain_db != 0: every sample of the part becomes the f32 product x * g, g = (float)pow(10, gain_db / 20), rounded once, nothing
 *     fused.  level != 0: the part is what ptts_loudness_normalize(part, n, level / 100.0, NULL) makes of it as the tempo left it: its gain
 *     includes the 1 / peak ceiling and is 1 (the samples stay as they are) when no block passes the gates.  Neither: the part's bits move as
 *     ptts_join moves them.  In a crossfade a and b of the formula are the scaled samples.
 * ptts_join_parts_length: ptts_join_length with per-seam G_i, K_i.  Reads only size, gap_ms and crossfade_ms of each element.  Host.
 * ptts_join_parts: the statement of volume plus join.  Reads only size, level, gain_db, gap_ms and crossfade_ms of each element; gains
 *     (optional, [rows]) receives the f32 gain applied to part i, 1.0f for none.  Host.
 * ptts_join_parts_rows: the same on the device, by the kernels the call runs (k_join_gain where a part of the table has a gain, k_join where
 *     none has; for `level` the measuring kernels of the loudness rows, whose gain word the join reads), shaped like ptts_join_rows.  It gives
 *     ptts_join_parts' bits.
 * ptts_join_parts_stream_ready: ptts_join_stream_ready with K taken from the seam behind the part `last` describes.
 * ptts_generate_joined_parts: ptts_generate_joined_streamed (so NULL: not streamed, every group holds max_batch parts) with the list po [n],
 *     required.  parts[i].offset and .n_samples count the final audio; gains (optional, [n]) receives the parts' gains.  The bound on the
 *     joined length takes, per part, the largest of its step budget, its resampled and its final length, plus the per-seam gaps; 2^31 is
 *     refused.  In a streamed call K of P_g is the crossfade resolved for the seam behind group g's last part.
 *   PTTS_EINVAL, nothing launched, naming the field and the part index: any bad field; level together with gain_db; formant without pitch; a
 *     dsp->ext handle that itself carries a trim, pitch, formant or tempo ("join: parts: ... belongs in the list"); and everything
 *     ptts_generate_joined_streamed refuses, in its own words. */
typedef struct ptts_part_opts {
    uint32_t size;                       /* sizeof(ptts_part_opts) as the caller compiled it; the rules of ptts_dsp_ext_opts.size */
    int32_t  level;                      /* 0: off; else this part's loudness target in 0.01 LUFS, -7000 .. -100; not with gain_db != 0 */
    const ptts_trim_opts*    trim;       /* NULL: this part is not trimmed */
    const ptts_pitch_opts*   pitch;      /* NULL: none */
    const ptts_formant_opts* formant;    /* NULL: none; needs pitch, its own range rules apply */
    const ptts_tempo_opts*   tempo;      /* NULL: none */
    double   gain_db;                    /* -60 .. +24, finite; 0: none */
    double   gap_ms;                     /* the seam BEHIND this part */
    double   crossfade_ms;
} ptts_part_opts;                        /* 64 bytes */
int64_t ptts_join_parts_length(const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, int64_t* offsets /* optional [rows] */);
int  ptts_join_parts(const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po, float* out,
                     float* gains /* optional [rows] */);
int  ptts_join_parts_rows(ptts_model* m, const float* const* in, const int64_t* n, int32_t rows, const ptts_join_opts* o, const ptts_part_opts* po,
                          float* out, float* gains /* optional [rows] */);
int64_t ptts_join_parts_stream_ready(const ptts_join_opts* o, const ptts_part_opts* last, int64_t joined);
int  ptts_generate_joined_parts(ptts_model* m, const ptts_request* reqs, int32_t n, const ptts_join_opts* o, const ptts_part_opts* po /* [n] */,
                                const ptts_join_stream_opts* so /* NULL: not streamed */, ptts_result* out, ptts_join_part* parts /* [n], optional */,
                                float* gains /* optional [n] */);

/* ---- Text front end (internal/text/prepare.go, chunk.go) -------------------------------------------------
 * What Synthesize does before it calls the runtime: normalise the text, cut it into sentence-based chunks of <= max_tokens
 * tokens, and derive each chunk's step budget and EOS tail.  The SentencePiece encoder is the caller's. */
int32_t ptts_text_estimate_max_frames(int64_t token_count, double frame_rate);   /* EstimateMaxFrames, prepare.go:38-48 */
int32_t ptts_text_frames_after_eos(int64_t num_words);                            /* FramesAfterEOS, prepare.go:53-59 */
/* PrepareText (prepare.go:66-100).  Writes up to cap bytes (no terminator) and the full length to *out_len. */
int  ptts_text_prepare(const char* utf8, int64_t len, char* out, int64_t cap, int64_t* out_len);
/* Encoder callback: writes up to cap ids and returns the count (> cap: called again with room), < 0: error. */
typedef int64_t (*ptts_encode_fn)(void* user, const char* utf8, int64_t len, int64_t* ids, int64_t cap);

/* SentencePiece unigram encoder (tokenizer.NewSentencePieceTokenizer / Tokenizer.Encode, internal/tokenizer/sentencepiece.go:19-40;
 * algorithm: internal/tokenizer/sentencepiece_bytes_wasm.go = go-sentencepiece-encoder v1.1.1): reads the pieces of a
 * SentencePiece ModelProto (`tokenizer.model`), normalises (control characters dropped, White_Space -> ' ', NFKC), prepends and
 * substitutes U+2581, Viterbi over the piece trie, consecutive unknowns merged. */
typedef struct ptts_tokenizer ptts_tokenizer;
int     ptts_tokenizer_open(const char* model_path, ptts_tokenizer** out);
int     ptts_tokenizer_open_bytes(const void* data, size_t len, ptts_tokenizer** out);
void    ptts_tokenizer_free(ptts_tokenizer* t);
int64_t ptts_tokenizer_vocab_size(const ptts_tokenizer* t);
/* Encode: writes up to cap ids, returns the count (> cap: call again with room; an empty text gives 0), < 0 on error */
int64_t ptts_tokenizer_encode(const ptts_tokenizer* t, const char* utf8, int64_t len, int64_t* ids, int64_t cap);
/* the same with the signature of the encoder callback, user = the ptts_tokenizer: ptts_text_chunks(text, len, ptts_tokenizer_encode_cb, tok, ...);
 * ptts_text_chunks also takes encode == NULL with user = a ptts_tokenizer as "use the built-in encoder" */
int64_t ptts_tokenizer_encode_cb(void* user, const char* utf8, int64_t len, int64_t* ids, int64_t cap);
/* NFKC as the tokenizer applies it (generated Unicode tables) */
int     ptts_text_nfkc(const char* utf8, int64_t len, char* out, int64_t cap, int64_t* out_len);
typedef struct ptts_chunks ptts_chunks;
typedef struct ptts_chunk_info {
    const char* text; int64_t text_len;            /* PrepareText of the joined sentences */
    const int64_t* token_ids; int64_t n_tokens;
    int32_t num_words;                             /* of the raw sentences (prepare.go:140) */
    int32_t max_frames;                            /* EstimateMaxFrames(n_tokens, frame_rate) */
    int32_t frames_after_eos;
    int32_t reserved;
} ptts_chunk_info;
/* PrepareChunks (prepare.go:105-184); max_tokens: 50 in the reference's service; frame_rate <= 0: 12.5 */
int  ptts_text_chunks(const char* utf8, int64_t len, ptts_encode_fn encode, void* user, int32_t max_tokens, double frame_rate, ptts_chunks** out);
int32_t ptts_chunks_count(const ptts_chunks* c);
int  ptts_chunks_get(const ptts_chunks* c, int32_t i, ptts_chunk_info* out);
void ptts_chunks_free(ptts_chunks* c);

/* ---- Request dispatcher (what the reference's worker pool becomes) ----------------------------------
 * internal/server/server.go:132-134,398-421 admits `workers` concurrent Synthesize calls through a semaphore; here callers
 * block in ptts_dispatch_generate and a worker thread per model coalesces waiting requests (up to max_batch, for at most
 * window_us after the oldest one arrived) into one batched generate.  A request cancelled while it waits is answered
 * PTTS_ECANCELLED without running.  Several models (one per GPU) pull from the same queue; nothing is exchanged between them.
 * A request that carries a device voice is served by the model that voice was uploaded to. */
typedef struct ptts_dispatcher ptts_dispatcher;
typedef struct ptts_dispatch_opts {
    int32_t max_batch;    /* <= 0: the model's max_batch */
    int32_t window_us;    /* coalescing window, counted from the arrival of the oldest waiting request; stretched (to at most
                           * 4 windows) while requests keep arriving less than window_us / 4 apart */
    int32_t queue_cap;    /* <= 0: 4096; a full queue answers PTTS_ENOMEM */
    int32_t continuous;   /* 1: continuous batching -- one long-lived batch per model: between groups of AR steps, utterances that have
                           * ended leave for the decoder and waiting requests take their slots (their prompts prefilled as one ragged
                           * launch).  Requests with a step / PCM callback, lsd_steps > 1 or budgets beyond the two limits below run
                           * batch-at-a-time while the engine is empty.  -1: batch-at-a-time for everything.  0 (the default): continuous
                           * when every model of the dispatcher has its GPU to itself (where it wins uniform AND mixed-length traffic),
                           * batch-at-a-time when two of them share one (ptts_model_share: the two-engine setting) */
    int32_t cont_kv_capacity;      /* keys per slot (voice prefix + prompt + steps), <= 0: 512 (the reach of the one-burst step attention with a bf16 cache) */
    int32_t cont_max_steps;        /* step budget per utterance, <= 0: 256 (EstimateMaxFrames of a 50-token chunk is 234) */
    int32_t cont_steps_per_group;  /* AR steps between two looks at the slots, <= 0: 3 */
    int32_t reserved[1];
} ptts_dispatch_opts;
typedef struct ptts_dispatch_stats {
    int64_t requests, batches, cancelled_waiting, max_queue_depth;
    double  mean_batch, mean_wait_us, mean_exec_us;
    int64_t cont_steps, cont_slot_steps;   /* continuous batching: AR steps launched; utterances stepping in them, summed (ratio = mean occupied slots) */
    int64_t flow_cluster_fallbacks;        /* times a hand-off inside k_flow_cluster timed out on one of the dispatcher's models: the steps concerned were redone as
                                            * launches (same bits, nobody failed) and that engine keeps the launches from then on */
} ptts_dispatch_stats;
int  ptts_dispatcher_create(ptts_model* const* models, int32_t n_models, const ptts_dispatch_opts* opts, ptts_dispatcher** out);
/* queueing logic over a caller-supplied executor (no GPU involved): unit tests of the coalescing / cancellation rules */
typedef int (*ptts_dispatch_exec)(void* user, int32_t worker, const ptts_request* reqs, int32_t n, ptts_result* results, char* err, int32_t errlen);
int  ptts_dispatcher_create_custom(ptts_dispatch_exec exec, void* user, int32_t n_workers, const ptts_dispatch_opts* opts, ptts_dispatcher** out);
int  ptts_dispatch_generate(ptts_dispatcher* d, const ptts_request* req, ptts_result* result);   /* blocks until the request has run */
void ptts_dispatcher_stats(ptts_dispatcher* d, ptts_dispatch_stats* out);
void ptts_dispatcher_close(ptts_dispatcher* d);   /* waits for queued work; later calls are refused */

/* Uploads a voice model state ([2,1,T,H,Dh] f32 per layer + offsets; safetensors.LoadVoiceModelState,
 * reader.go:127-140,273-308) once; requests then reference it by handle. */
int  ptts_voice_create(ptts_model* m, const float* const* caches, const int64_t* cache_steps, const int64_t* offsets, ptts_voice** out);
void ptts_voice_free(ptts_voice* v);

/* ---- voice FILES (internal/safetensors/reader.go:69-155,219-308).  The reference's Service reads the voice path of a request with
 *      InspectVoiceFile and then either LoadVoiceModelState or LoadVoiceEmbedding (internal/tts/service.go:216-246); these entry points
 *      are those three functions plus the consumer-side checks of flowTransformer.initStateFromVoiceModelState
 *      (internal/native/flow_transformer.go:451-590).  Host only: no GPU is touched until ptts_voice_open uploads. ---- */
#define PTTS_VOICE_FILE_UNKNOWN      0   /* VoiceFileUnknown */
#define PTTS_VOICE_FILE_EMBEDDING    1   /* VoiceFileEmbedding: legacy `audio_prompt` (or any first tensor) [T, D] / [1, T, D] */
#define PTTS_VOICE_FILE_MODEL_STATE  2   /* VoiceFileModelState: `<module>/cache` [2,B,T,H,D] + `<module>/offset` (or legacy `<module>/current_end`) */
typedef struct ptts_voice_file ptts_voice_file;
int  ptts_voice_file_open(const char* path, ptts_voice_file** out);                        /* OpenStore + classifyVoiceTensorNames + load */
int  ptts_voice_file_open_bytes(const void* data, size_t len, ptts_voice_file** out);      /* ...FromBytes; the bytes are copied */
void ptts_voice_file_close(ptts_voice_file* f);
int32_t ptts_voice_file_kind(const ptts_voice_file* f);                                    /* InspectVoiceFile: PTTS_VOICE_FILE_* */
/* LoadVoiceEmbedding (reader.go:69-85,219-230): the first tensor (sorted names) as [1, T, D]; *data stays owned by f and is what a
 * request carries as voice_embedding (voice_frames = shape[1]; shape[2] must be the model's d_model).  PTTS_EFORMAT with the
 * reference's message for a model-state file and for a tensor that is not 2-D or 3-D. */
int  ptts_voice_file_embedding(const ptts_voice_file* f, const float** data, int64_t shape[3]);
/* LoadVoiceModelState (reader.go:127-140,273-308) as the reference's map of modules: count, then per module its name and tensors
 * ("cache", "offset"; a legacy `current_end` has already become offset = [float(len(current_end))], shape [1]).  PTTS_EFORMAT with the
 * reference's message for an embedding file or a tensor name without "<module>/<key>". */
typedef struct ptts_voice_tensor { const float* data; int64_t count; int32_t rank; int32_t reserved; int64_t shape[8]; } ptts_voice_tensor;
int  ptts_voice_file_modules(const ptts_voice_file* f, int32_t* n_modules);
int  ptts_voice_file_module(const ptts_voice_file* f, int32_t i, const char** name, ptts_voice_tensor* cache /* data NULL: absent */, ptts_voice_tensor* offset);
/* initStateFromVoiceModelState (flow_transformer.go:451-480,517-590) up to the re-layout: for layers 0..n_layers-1 the module
 * "transformer.layers.{i}.self_attn" must hold a cache [2,1,T,heads,head_dim] and an integral offset 0 <= offset <= T (heads /
 * head_dim 0: unchecked, as a layer without them is in the reference).  Fills what ptts_request.voice_caches / voice_cache_steps /
 * voice_offsets and ptts_voice_create take (pointers owned by f).  PTTS_EINVAL with the reference's messages. */
int  ptts_voice_file_state(const ptts_voice_file* f, int32_t n_layers, int32_t heads, int32_t head_dim,
                           const float** caches, int64_t* cache_steps, int64_t* offsets);
/* a model-state voice file straight into HBM: ptts_voice_file_open[_bytes] + ptts_voice_file_state (the model's dimensions) +
 * ptts_voice_create.  An embedding file answers PTTS_EFORMAT (LoadVoiceModelState's message): read it with ptts_voice_file_embedding. */
int  ptts_voice_open(ptts_model* m, const char* path, ptts_voice** out);
int  ptts_voice_open_bytes(ptts_model* m, const void* data, size_t len, ptts_voice** out);

/* ---- cloned voices as model states.  The reference's `pocket-tts export-voice --format model-state` (cmd/pockettts/export_voice.go) runs the
 *      Python package to turn a voice into per-layer KV caches; here the state is built on the GPU.  A voice embedding prepended to the prompt
 *      (runtime_native_safetensors.go:104-119) is prefilled again by every request; its model state is prefilled once and then shared by
 *      requests like a stock voice (ptts_request.voice). ---- */
/* emb[i]: host [frames[i], width] f32 voice embedding (width == d_model, 1 <= frames[i] <= 8192).  One prefill of all n embeddings, each alone
 * from position 0 (voice first, no text), and their KV rows into n new device voices out[0..n) with offset frames[i]: exactly what
 * ptts_voice_create makes of the same caches.  PTTS_EINVAL (nothing allocated) for a bad count, width, frame count or null pointer. */
int  ptts_voice_from_embeddings(ptts_model* m, const float* const* emb, const int64_t* frames, int64_t width, int32_t n, ptts_voice** out /* [n] */);
/* ptts_voice_encode_audio per clip (PARITY UNPINNED: the inferred encoder), then one ptts_voice_from_embeddings of the n embeddings.
 * PTTS_EFORMAT naming the missing tensor on a checkpoint without encoder or speaker projection weights. */
int  ptts_voice_from_audio(ptts_model* m, const float* const* pcm, const int64_t* n_samples, int32_t n, ptts_voice** out /* [n] */);
int  ptts_voice_offset(const ptts_voice* v, int64_t* offset);   /* keys the voice holds */
/* layer `layer` of a device voice as the reference's cache [2, 1, offset, H, Dh] f32 (flow_transformer.go:517-566; a bf16 cache widened exactly):
 * what ptts_voice_create takes back */
int  ptts_voice_read_state(const ptts_voice* v, int32_t layer, float* cache /* [2,1,offset,H,Dh] */);
/* a device voice as a model-state voice file (reader.go:127-155,273-308): per layer `transformer.layers.{l}.self_attn/cache` F32 [2,1,offset,H,Dh]
 * and `/offset` I64 [1], no padding rows.  _bytes: the file in memory (*data released with ptts_free_bytes). */
int  ptts_voice_write(const ptts_voice* v, const char* path);
int  ptts_voice_write_bytes(const ptts_voice* v, uint8_t** data, size_t* len);
/* the same file from host caches (caches[l]: [2, 1, offset, heads, head_dim] f32); host only */
int  ptts_voice_state_write_bytes(const float* const* caches, int64_t offset, int32_t n_layers, int32_t heads, int32_t head_dim, uint8_t** data, size_t* len);
/* a legacy-embedding voice file (reader.go:69-85,219-230): `audio_prompt` F32 [1, frames, dim] from emb [frames, dim] (host only) */
int  ptts_voice_embedding_write(const float* emb, int64_t frames, int64_t dim, const char* path);
void ptts_free_bytes(uint8_t* data);

/* Measurement hook for bench.py: while enabled the AR step runs eagerly (no graph) with a HIP event pair around
 * every launch of the dominant (weight-streaming linear) kernel on the model's stream. */
typedef struct ptts_profile {
    int64_t launches;
    double  total_ms;            /* sum of the event-pair durations */
    double  algorithmic_bytes;   /* sum over launches of weights + activations in + out */
    char    kernel[64];
    double  weight_bytes;        /* the weights-only part of algorithmic_bytes (each step linear's matrix once per launch) */
    double  prefill_ms, ar_loop_ms, mimi_ms;   /* device time of the phases of the last ptts_generate call (HIP events on its streams) */
} ptts_profile;
int ptts_profile_enable(ptts_model* m, int32_t on);   /* 0: off; 1: per-launch events (plain launches) + phase times; 2: phase times only (the call runs as configured) */
int ptts_profile_read(ptts_model* m, ptts_profile* out);   /* returns and resets the counters */

/* ---- staged entry points = the native.Model methods GenerateAudio calls (model.go:76-138,141,410).
 *      A ptts_batch is n_slots independent FlowLMState objects (flow_lm.go:45-49) held in HBM. ---- */
int  ptts_text_embeddings(ptts_model* m, const int64_t* ids, int64_t n, float* out /* [n, d_model] host */); /* Model.TextEmbeddings */
int  ptts_batch_new(ptts_model* m, int32_t n_slots, int32_t kv_capacity, ptts_batch** out);                 /* Model.NewFlowState x n_slots */
void ptts_batch_free(ptts_batch* b);
int  ptts_batch_reset(ptts_batch* b);
/* Model.NewFlowStateFromVoiceModelState for one slot */
int  ptts_batch_set_voice_state(ptts_batch* b, int32_t slot, const float* const* caches,
                                const int64_t* cache_steps, const int64_t* offsets);
/* Model.PromptFlow for every slot at once: slot s gets emb + row_offsets[s] .. row_offsets[s+1] (rows of d_model floats, host) */
int  ptts_batch_prompt(ptts_batch* b, const float* emb, const int64_t* row_offsets);
/* Model.SampleNextLatentStateful for every slot: frames_in [n_slots, ldim] (NaN = BOS), noise NULL or [n_slots, ldim];
 * outputs (host, caller-allocated, any may be NULL): frames_out [n_slots, ldim], eos_logits [n_slots], last_hidden [n_slots, d_model] */
int  ptts_batch_step(ptts_batch* b, const float* frames_in, int32_t lsd_steps, const float* noise,
                     float* frames_out, float* eos_logits, float* last_hidden);
int  ptts_batch_offsets(ptts_batch* b, int64_t* out /* [n_slots] */);
int  ptts_batch_read_kv(ptts_batch* b, int32_t slot, int32_t layer, float* k, float* v /* [H, offset, Dh] each */);
/* Model.LatentToMimi + Model.MimiDecode: latents [n_utt, frames, ldim] host -> pcm [n_utt, frames*samples_per_frame] host;
 * mimi_latent (optional) receives LatentToMimi's [n_utt, mimi_dim, frames] */
int  ptts_decode_latents(ptts_model* m, const float* latents, int32_t n_utt, int32_t frames,
                         float* pcm, float* mimi_latent);
/* Voice cloning, the part the reference holds natively: projectSpeakerConditioning
 * (internal/onnx/voice_encode.go:119-158) -- Mimi-encoder latents [frames, 512] (host) times flow_lm.speaker_proj_weight
 * [d_model, 512] -> voice embedding [frames, d_model] (host), which a request then carries as `voice_embedding`.  PTTS_EFORMAT when the
 * checkpoint has no speaker projection tensor. */
int  ptts_speaker_project(ptts_model* m, const float* latent, int64_t frames, float* out);
/* The first half: the Mimi encoder (mimi.encode_to_latent, internal/onnx/voice_encode.go:23-158) on the GPU.  PARITY UNPINNED: inferred
 * architecture, no reference fixture -- the reference has no native encoder (mimi.go:14,791-794: ErrMimiEncoderNotImplemented), so the chain is
 * inferred from the decoder and exists only on checkpoints that carry mimi.encoder.* / mimi.encoder_transformer.* /
 * mimi.downsample.* tensors.  pcm[i]: n_samples[i] samples of 24 kHz mono f32 (host; resampling and WAV parsing are the caller's), zero-padded
 * to whole frames; latent_out[i] (host) receives the raw [ptts_mimi_encode_frames(n_samples[i]), 512] latent (no quantizer, no emb_mean/emb_std).
 * Clips are independent: a clip's result does not depend on the others in the call.  PTTS_EINVAL for an empty clip or one longer than
 * 512 frames (40.96 s); PTTS_EFORMAT, naming the missing tensor, on a checkpoint without encoder weights. */
int  ptts_mimi_encode(ptts_model* m, const float* const* pcm, const int64_t* n_samples, int32_t n_clips, float* const* latent_out);
/* frames the encoder makes of n samples: ceil(n / 1920) (sample_rate / frame_rate); 0 for 0 samples (which ptts_mimi_encode rejects),
 * -PTTS_EINVAL for a negative count */
int64_t ptts_mimi_encode_frames(int64_t n_samples);
/* both halves for one clip, the projection on the device: embedding_out (host) receives [frames, d_model], *frames the frame count.
 * PTTS_EFORMAT naming the missing tensor without encoder weights or without the speaker projection. */
int  ptts_voice_encode_audio(ptts_model* m, const float* pcm, int64_t n_samples, float* embedding_out, int64_t* frames);
/* The device draw of FlowLM.makeGaussianNoise (flow_lm.go:386-408) for one request: out[rows, ldim] (host) receives exactly the
 * rows ptts_generate would consume for (noise_seed = seed, temperature) -- so that a test can hand the same noise to a reference. */
int  ptts_noise_rows(ptts_model* m, uint64_t seed, float temperature, int32_t rows, float* out);
/* FlowLM.FlowDirection (flow_lm.go:302-308): c [n, d_model], x [n, ldim] -> out [n, ldim] */
int  ptts_flow_direction(ptts_model* m, const float* c, float s, float t, const float* x, int32_t n, float* out);

/* ---- kernel-level entry points (host buffers in/out) = internal/runtime/ops + tensor, backed by
 *      the same HIP kernels the model path launches; they exist so that the reference's
 *      known-answer tests can be replayed against the GPU kernels. ---- */
int ptts_op_linear(const float* x, const float* w, const float* bias, int64_t rows, int64_t in, int64_t out, float* y);              /* tensor.Linear nn_ops.go:268 */
int ptts_op_layernorm(const float* x, const float* w, const float* b, float eps, int64_t rows, int64_t d, float* y);                 /* tensor.LayerNorm nn_ops.go:79 */
int ptts_op_rope(float* x /* [prefix, seq, dim] in place */, const float* cos_t, const float* sin_t, int64_t table_rows,
                 int64_t prefix, int64_t seq, int64_t dim, int64_t pos);                                                              /* ops.RoPE rope.go:13 */
int ptts_op_attention_positions(const float* q, const float* k, const float* v, int64_t b, int64_t h, int64_t tq, int64_t tk,
                 int64_t d, const int64_t* posq, const int64_t* posk, int64_t context, float* out);                                  /* ops.AttentionWithPositions attention.go:63 */
int ptts_op_conv1d_leftpad(const float* x /* [B,Cin,L] */, const float* w /* [Cout,Cin,k] */, const float* bias,
                 int64_t b, int64_t cin, int64_t len, int64_t cout, int64_t k, float* y /* [B,Cout,L] */);                           /* ops.Conv1DLeftPad conv1d.go:95 (stride 1, leftPad k-1) */
int ptts_op_convtr1d_righttrim(const float* x /* [B,Cin,L] */, const float* w /* [Cin,Cout/groups,k] */, const float* bias,
                 int64_t b, int64_t cin, int64_t len, int64_t cout_per_group, int64_t k, int64_t stride, int64_t groups,
                 float* y /* [B,Cout,L*stride] */);                                                                                  /* ops.ConvTranspose1DRightTrim convtranspose1d.go:213 (k = 2*stride, trim k-stride; groups 1 or Cin) */

/* audio.WritePCM16Samples on the device (internal/audio/wav_stream.go:43-54), without the byte packing */
int ptts_op_pcm16(const float* samples, int64_t n, int16_t* out);

/* ---- sample rates and egress formats.  Rates are multiples of 25 Hz: 8000..48000 out, 8000..192000 in; the filter
 *      is the windowed-sinc polyphase of DESIGN.md (Kaiser, beta 8.6, 24 zero crossings, cutoff 0.45 of the lower Nyquist rate), one f32 fmaf chain
 *      per output in ascending input order -- so batched, streamed and one-shot conversions give the same bits.  A rate pair whose reduced
 *      tap table exceeds the kernel's bound (512 phases, 65536 taps) is refused with PTTS_EINVAL naming both rates. ---- */
/* samples that n_in samples at in_rate become at out_rate: ceil(n_in * L / M).  No GPU.  -PTTS_EINVAL for a bad rate, pair or count */
int64_t ptts_resample_length(int64_t n_in, int32_t in_rate, int32_t out_rate);
/* n rows of host samples resampled on the device in one launch: out[i] (host) receives ptts_resample_length(n_in[i], in_rate, out_rate) floats.
 * in_rate == out_rate copies. */
int  ptts_resample(ptts_model* m, const float* const* in, const int64_t* n_in, int32_t n, int32_t in_rate, int32_t out_rate, float* const* out);
/* the device egress conversion at 24 kHz: n host samples -> out (host) in pcm_format (f32 as is, PCM16 as ptts_op_pcm16, G.711 of that int16) */
int  ptts_pcm_encode(ptts_model* m, const float* in, int64_t n, int32_t pcm_format, void* out);
/* ptts_mimi_encode / ptts_voice_from_audio for clips at their own rates (sample_rates[i], 8000..192000; NULL: all 24000): each clip is uploaded
 * as it is and k_resample writes its 24 kHz samples straight into the encoder's input.  The 512-frame cap applies to the resampled length
 * (ptts_mimi_encode_frames(ptts_resample_length(n_samples[i], sample_rates[i], 24000))) and the error names it. */
int  ptts_mimi_encode_rates(ptts_model* m, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates, int32_t n_clips,
                            float* const* latent_out);
int  ptts_voice_from_audio_rates(ptts_model* m, const float* const* pcm, const int64_t* n_samples, const int32_t* sample_rates, int32_t n,
                                 ptts_voice** out /* [n] */);
/* A WAV header for mono audio of n_samples samples (n_samples < 0: streaming, every size 0xFFFFFFFF) in pcm_format at sample_rate (0: 24000):
 * PCM16 -> the 44-byte PCM header (at 24000 and n_samples < 0 exactly ptts_wav_header_streaming's); f32 (format 3), A-law (6), mu-law (7) ->
 * an 18-byte fmt chunk (cbSize 0) plus a fact chunk: 58 bytes.  Returns the header length, -PTTS_EINVAL for a bad argument or cap too small. */
int  ptts_wav_header(uint8_t* out, int32_t cap, int32_t sample_rate, int32_t pcm_format, int64_t n_samples);

/* build/version string, e.g. "ptts-hip 0.3 gfx950".  0.3: ptts_request.sample_rate, PTTS_PCM_ULAW / PTTS_PCM_ALAW with ptts_result.pcm8
 * (in the place of reserved fields: the struct sizes are those of 0.2), ptts_resample_length, ptts_resample, ptts_pcm_encode,
 * ptts_mimi_encode_rates, ptts_voice_from_audio_rates, ptts_wav_header.  Later additions keep the number (hosts test for the symbol):
 * ptts_request.dsp (in the place of reserved2: the struct's size and every other offset are unchanged) with ptts_dsp_opts, and ptts_dsp_rows;
 * ptts_request.loudness (in the place of reserved[1], likewise), ptts_loudness, ptts_loudness_normalize, ptts_loudness_rows,
 * ptts_loudness_normalize_rows; ptts_dsp_opts.eq (over reserved[0..1] of ptts_dsp_opts: its size and every offset are unchanged) with
 * ptts_eq_section, ptts_eq_design, ptts_eq_response, ptts_eq_create, ptts_eq_free, ptts_eq_apply, ptts_eq_rows; ptts_dsp_opts.ext (over
 * reserved[2..3], likewise) with ptts_dsp_ext_opts, ptts_dsp_ext_create, ptts_dsp_ext_free, ptts_true_peak, ptts_true_peak_limit,
 * ptts_true_peak_rows; ptts_compressor_opts with ptts_dsp_ext_set_compressor (the handle is the extension point: no struct grows),
 * ptts_compress_gain, ptts_compress_apply, ptts_compress_rows; ptts_limiter_opts with ptts_dsp_ext_set_limiter, ptts_limit_apply,
 * ptts_limit_rows; the new structs ptts_join_opts and ptts_join_part, which change no existing one, with ptts_join_length, ptts_join, ptts_join_rows,
 * ptts_generate_joined; the new structs ptts_trim_opts and ptts_trim_info, likewise, with ptts_trim_plan, ptts_trim_apply, ptts_trim_rows,
 * ptts_dsp_ext_set_trim; the new struct ptts_tempo_opts, likewise, with ptts_tempo_length, ptts_tempo_plan, ptts_tempo_apply, ptts_tempo_rows,
 * ptts_dsp_ext_set_tempo; the new struct ptts_join_stream_opts, likewise, with ptts_generate_joined_streamed, ptts_join_stream_ready;
 * the new struct ptts_pitch_opts, likewise, with ptts_pitch_speed, ptts_pitch_resample_length, ptts_pitch_resample, ptts_pitch_length,
 * ptts_pitch_apply, ptts_pitch_table, ptts_pitch_rows, ptts_dsp_ext_set_pitch;
 * the new struct ptts_formant_opts, likewise, with ptts_formant_frames, ptts_formant_analyse, ptts_formant_whiten, ptts_formant_shape,
 * ptts_formant_apply, ptts_formant_rows, ptts_dsp_ext_set_formant;
 * the new struct ptts_deesser_opts, likewise, with ptts_dsp_ext_set_deesser, ptts_deess_apply, ptts_deess_band, ptts_deess_rows;
 * the new struct ptts_part_opts, likewise, with ptts_join_parts_length, ptts_join_parts, ptts_join_parts_rows, ptts_join_parts_stream_ready,
 * ptts_generate_joined_parts */
const char* ptts_version(void);

/* Test and measurement hooks (launch census, in-kernel stamps, micro-benchmarks, staged observation points of the decoder, the fault injection of
 * k_flow_cluster's hand-offs) are NOT in this library: they are declared in ptts_debug.h and live in libptts_hooks.so, which the tests load beside it. */

#ifdef __cplusplus
}
#endif
#endif /* PTTS_H */
