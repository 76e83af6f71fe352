// runtime.h -- host-side engine above the kernels: device model and its table of work buffers (WorkSlot), batch of FlowLM states, prefill, AR step
// (hipGraph), Mimi decode and encode, GenerateAudio loop, the continuous batch, the device side of the staged entry points (staged.cpp).
#pragma once

#include <atomic>
#include <functional>
#include <type_traits>

#include "kernels.h"
#include "model.h"
#include "row_ring.h"
#include "dsp_spec.h"
#include "host_rows.h"
#include "join.h"

namespace ptts {

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void ensure(size_t bytes) {  // grow-only
        if (bytes <= n && p) return;
        release();
        if (bytes == 0) bytes = 256;
        PTTS_HIP(hipMalloc(&p, bytes));
        n = bytes;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct Batch;

// a page-locked host buffer, grow-only: what a small device->host read-back lands in without a staging copy
struct PinnedBuf {
    void* p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    void* ensure(size_t bytes) {
        if (bytes <= n && p) return p;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        PTTS_HIP(hipHostMalloc(&p, std::max<size_t>(bytes, 256), hipHostMallocDefault));
        n = std::max<size_t>(bytes, 256);
        return p;
    }
};

// Model::work's buffers, every one by name: the table of what lives in Model::ws.  Every user holds Model::mu from its first use of a buffer until
// the work that reads it is queued on a stream of the model (the staged entry points and staged_convert even wait for it), so two names for one
// number never hold data at the same time.  Behind each name: who holds the buffer, and until when.  Where one number has several names, the
// comment of the later names says why they never meet the earlier ones.  A holder that asks for more than the buffer has goes through
// DevBuf::ensure's hipFree, which waits for the device: a buffer never moves under queued work.
enum WorkSlot : size_t {
    WORK_TCOMB = 0,              // Model::compute_tcomb: the timestep features, hidden row and the two embeddings; until its launches are queued on Model::stream (tcomb_for waits for them)
    WORK_VOICE_RAW = 1,          // voice_create, batch_set_voice: one layer of a host voice cache in front of its scatter; until the stream wait that follows each layer
    WORK_PROMPT_META = 2,        // batch_prompt: the ragged table (row -> slot | position | offsets); until the prefill is queued on its stream (the model's, or the batch's io_stream)
    WORK_PROMPT_ACT = 3,         // batch_prompt: the prefill's activations (x | xn | qkv | attn | ff); likewise
    WORK_DECODER = 4,            // mimi_setup: the decoder's activations of one group.  A Chunk holds it from decoder_setup to decode_rest's wait for stream2; the staged decode
                                 // until its stream wait; the continuous engine (which keeps Model::mu while busy) from one start_decode to the next: its serial decodes run on
                                 // Model::stream and its concurrent ones on ContEngine::dec, and a decode waits for lat_free[lprev], recorded behind the previous decode whichever
                                 // stream that ran on.  cont_create sizes it for the largest sub-group, so no decode reallocates it under another
    WORK_PROMPT_ROWS = 5,        // stage_prompt: the packed prompt rows (gathered text rows, voice embeddings); until batch_prompt has copied them, in stream order
    WORK_TEXT_ROWS = 5,          // staged_text_embeddings: the gathered rows; until its stream wait.  Under Model::mu from first use to that wait, as every staged_* holder: never beside another
    WORK_PROMPT_UPLOAD = 5,      // staged_prompt: the caller's rows in front of batch_prompt; until its stream wait
    WORK_PROMPT_IDS = 6,         // stage_prompt: the batch's token ids; until the gathers are queued
    WORK_TEXT_IDS = 6,           // staged_text_embeddings: the ids; until its stream wait
    WORK_PCM = 7,                // Chunk (generate, generate_joined): the decoded rows [B][T * spf]; from decoder_setup until the results are read, the last wait of the chunk (under Model::mu throughout)
    WORK_CONT_PCM = 7,           // the continuous engine: one sub-group's decoded rows, sized in cont_create for the largest; sub-groups follow each other in stream order on one stream, decodes
                                 // are ordered by lat_free[lprev] as WORK_DECODER's.  The engine holds Model::mu while busy, so no Chunk runs beside it
    WORK_STREAM_S16 = 8,         // Chunk::stream_s16: the PCM16 image of streamed rows, sized [B][T * spf] in decoder_setup; read by emit_upto's copies on stream2, which decode_rest drains
    WORK_EGRESS_S16 = 8,         // results_deliver: the PCM16 image of a group's rows; until the caller's wait behind the copies.  In a Chunk that also streams, the size is the same
                                 // [B][T * spf] int16 as WORK_STREAM_S16's (n = B, pcm_stride = T * spf), so this ensure never outgrows that one, and it runs behind decode_rest's wait
                                 // for stream2: the streamed copies are done.  In the continuous engine cont_create sizes it for the largest sub-group, ordered as WORK_CONT_PCM
    WORK_DECODE_IO = 8,          // staged_decode: latents | pcm | mimi latent | transformer rows of one call; until its stream wait
    WORK_SPEAKER_IO = 8,         // staged_speaker_project: latents | embedding; until its stream wait
    WORK_NOISE_ROWS = 8,         // staged_noise_rows: the drawn rows; until its stream wait
    WORK_PREFILL_PLANES = 9,     // batch_prompt: linear2's split-K planes [S][R][D]; from the launch that writes them to the next layer's LayerNorm launch, which adds them (stream order)
    WORK_FLOW_DIRECTION = 9,     // staged_flow_direction: its whole workspace; until its stream wait.  It runs no prefill, and every caller of batch_prompt keeps Model::mu until its
                                 // prefill has run (a Chunk and the continuous engine until their results are out; voice_build and staged_prompt until their stream wait)
    WORK_VOICE_SLOTS = 10,       // batch_apply_voice: the slots a device voice is applied to; until the launches are queued on the batch's stream
    WORK_PCM_ROWS = 11,          // Chunk::deliver: the PcmRow table of the decoder's direct store; until decode_rest's wait for stream2
    WORK_NOISE_SPECS = 12,       // stage_noise: the batch's NoiseSpec per slot; until launch_noise_fill is queued
    WORK_NOISE_ROWS_SPEC = 12,   // staged_noise_rows: its one NoiseSpec; until its stream wait
    WORK_CONT_RESERVE = 13,      // cont_create sizes it (a decode's worth of latents); nothing reads it since ContEngine::lat took the gathered frames.  Kept: the footprint is unchanged
    WORK_CONT_RETIRE = 15,       // take_snapshot: the slots that retire; until launch_slot_retire is queued on Model::stream
    WORK_ENCODER = 16,           // mimi_encode_clip: the encoder's activations of one clip; until the caller's stream wait behind the clip
    WORK_ENCODER_LATENTS = 17,   // mimi_encode: one clip's latents; until the stream wait behind each clip's copy out
    WORK_EMBEDDING_IO = 17,      // voice_embedding_device: a clip's latents and their projection; until its stream wait.  It calls mimi_encode_clip, not mimi_encode
    WORK_VOICE_BUILD_ROWS = 18,  // voice_build: the embeddings packed as prompt rows; until the stream wait behind each group
    WORK_VOICE_EXPORT = 19,      // voice_export: the layers in the reference's layout; until the read-back (d2h waits)
    WORK_VOICE_BUILD_TABLE = 20, // voice_build: the VoiceDst table of launch_voice_extract; until the stream wait behind each group
    WORK_EGRESS_PAGEABLE = 24,   // results_deliver: converted rows whose result buffer is pageable, copied out from here
    WORK_CONVERT_IN = 25,        // staged_convert (ptts_resample, ptts_pcm_encode): the packed input rows; until its stream wait
    WORK_CONVERT_OUT = 26,       // ... and the packed output rows
    WORK_ENCODER_CLIP = 26,      // mimi_encode_clip: a voice clip at its own rate, in front of k_resample.  Shares WORK_CONVERT_OUT's storage (see above)
    WORK_STREAM_SNAP = 27,       // Chunk::emit_upto: a hand-over's snapshot of (active, n_frames) for its k_resample rows; ranges follow each other on stream2, which decode_rest drains
    WORK_STREAM_STAGE = 28,      // Chunk::stream_stage: the converted rows of streamed requests, one row of stage_row bytes per slot; from decoder_setup until decode_rest drains stream2
    WORK_DSP_SCRATCH = 29,       // dsp_launch: peak words, then what dsp_scratch (dsp_spec.h) plans for each row's stages
    WORK_HOST_ROWS = 30,         // dsp_rows_device: the packed rows of ptts_dsp_rows and its kin; join_rows_device: the parts, then the joined row; part_rows_device: the rows, then their forms
    WORK_JOINED = 31,            // generate_joined: the text's joined row, sized before the first group runs and kept until the egress has read it
    WORK_TRIMMED = 32,           // generate_joined with a trim: PartRow::trimmed of a group's rows, what k_trim_store keeps of the decoded rows, at the decoder buffer's row stride
    WORK_TRIM_SCRATCH = 33,      // parts_launch, the trim: the rows' ptts_trim_info records, then their TrimTile tables
    WORK_TEMPO = 34,             // generate_joined with a tempo: PartRow::scaled of a group's rows, at the stride of the longest a decoded row can become
    WORK_TEMPO_SCRATCH = 35,     // parts_launch, the tempo: the rows' position tables
    WORK_JOIN_CARRY = 36,        // a streamed joined call: the chain's carried states between its windows (kernels.h kCarryDoubles)
    WORK_JOIN_STAGE = 37,        // ... and its egress where that cannot store into the result's buffer itself, indexed like that buffer
    WORK_PITCH = 38,             // generate_joined with a pitch: PartRow::shifted of a group's rows, at the stride of the longest a decoded row can become
    WORK_FORMANT_COEFFS = 39,    // parts_launch, rows that keep their formants: the frames' coefficients, [K][24] a row, one row behind the other
    WORK_FORMANT_RESIDUAL = 40,  // ... their residuals, what k_pitch_resample reads for them
    WORK_FORMANT_SHIFTED = 41,   // ... and their resampled residuals, what k_formant_shape reads
    WORK_PART_LEVEL = 42,        // level_launch: the peak words and loudness blocks of the parts with a `level`; until the k_join_gain launch that reads their gain words has run (stream order)
};
constexpr size_t kWorkSlots = 43;   // one past the largest value above (14 and 21-23 have no holder and stay empty DevBufs)

// ---- rate and format conversion of delivered audio (resample.cpp; k_resample in resample.hip) ----
constexpr int kNativeRate = 24000;            // the decoder's rate: requests at 0 / 24000 in f32 or PCM16 are delivered as before, without k_resample
constexpr int kResampleMaxL = 512;            // bounds of a reduced rate pair's tap table: L phases, L * K taps
constexpr int kResampleMaxTaps = 65536;
// one reduced rate pair (L = out / g, M = in / g) and its polyphase taps: the prototype h(t) at t = p / L - d for phase p and
// d = dlo + k, rounded once to f32, 0 where |t| >= W.  W = 80 max(L, M) / (3 L) input samples, so the support test is the integer
// 3 |p - d L| < A with A = 80 max(L, M)
struct RateFilter {
    int L = 1, M = 1, K = 0, dlo = 0, tile = 0;
    int64_t A = 0;
    size_t n_taps = 0;            // [L][K], padded to a multiple of 4
    float* staged = nullptr;      // page-locked host copy the upload reads
    DevBuf taps;
    hipEvent_t ready = nullptr;   // recorded behind the upload on `up`; a launch on another stream waits for it (no host wait anywhere)
    hipStream_t up = nullptr;
    RateFilter() = default;
    RateFilter(const RateFilter&) = delete;
    RateFilter& operator=(const RateFilter&) = delete;
    ~RateFilter();
};
// A table that a model makes once and keeps on the device, made and uploaded on first use like a RateFilter's taps (upload_once, dsp_device.cpp):
// k_pitch_resample's prototype table (pitch.h) as the kernel reads it (kernels.h pitch_image_at: [kPitchImage][2] floats, ONE per model whatever
// the pitches) and the formant kernels' float64 tables (formant.h formant_tables)
struct UploadedTable {
    void* staged = nullptr;       // page-locked host copy the upload reads
    DevBuf image;                 // the device copy
    hipEvent_t ready = nullptr;   // recorded behind the upload on `up`; a launch on another stream waits for it
    hipStream_t up = nullptr;
    UploadedTable() = default;
    UploadedTable(const UploadedTable&) = delete;
    UploadedTable& operator=(const UploadedTable&) = delete;
    ~UploadedTable();
};
struct Prof {   // bench.py measurement hook (ptts_profile_*)
    bool on = false;
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    double bytes = 0, wbytes = 0;
    int64_t launches = 0;
    hipEvent_t phase[5] = {};   // setup | prefill | AR loop on the model's stream; Mimi start | end on the decoder's stream
    bool phases_on = false;     // record them (with or without the per-launch events of `on`)
    bool phases = false;
};

// page-locked staging for the small host->device uploads of one generate call (runtime.cpp: h2d)
struct UploadArena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
};

struct Model {
    Desc d;
    ptts_opts opts;
    uint8_t* arena = nullptr;
    bool own_arena = false;
    int device = 0;
    hipStream_t stream = nullptr;    // AR loop / prefill (high priority: latency-bound launches)
    hipStream_t stream2 = nullptr;   // Mimi decode of finished frame ranges, concurrent with the AR loop
    std::vector<hipEvent_t> events;
    std::mutex mu;
    std::map<int, std::unique_ptr<DevBuf>> tcomb;  // lsd_steps -> [n][flow_dim]: 0.5*(embed_s(i/n) + embed_t((i+1)/n))
    DevBuf ws[kWorkSlots];                         // grow-only workspaces, one per WorkSlot value (work() below)
    std::unique_ptr<Batch> cached_batch;
    Prof prof;
    std::map<std::pair<int, int>, std::unique_ptr<RateFilter>> rate_filters;   // (input rate, output rate) -> k_resample's taps (resample.cpp)
    RowRing<ResampleRow> rs_ring;   // k_resample's row tables (resample.cpp)
    RowRing<CmpRow, kCmpMaxDesigns * kCmpScanBytes> cmp_ring;   // the compressor kernels', a table's designs behind its rows (dsp_device.cpp)
    RowRing<LimRow, kLimMaxDesigns * kLimScanBytes> lim_ring;   // the limiter kernels', likewise
    RowRing<DeRow, kDeMaxDesigns * kDeScanBytes> de_ring;       // the de-esser kernels', likewise
    RowRing<JoinRow> join_ring;     // k_join's (join_launch, dsp_device.cpp)
    RowRing<JoinGainRow> join_gain_ring;   // k_join_gain's (join_gain_launch, dsp_device.cpp)
    RowRing<TrimRow, kTrimMaxDesigns * kTrimScanBytes> trim_ring;   // the trim kernels', a table's designs behind its rows (parts_launch, dsp_device.cpp)
    RowRing<TempoRow, kTempoMaxDesigns * kTempoScanBytes> tempo_ring;   // the tempo kernels', likewise (parts_launch, dsp_device.cpp)
    RowRing<PitchRow, kPitchMaxDesigns * kPitchScanBytes> pitch_ring;   // k_pitch_resample's, likewise (parts_launch, dsp_device.cpp)
    std::unique_ptr<UploadedTable> pitch_image;   // ... and its table, from the first call that names a pitch on
    RowRing<FormantRow> formant_ring;          // the formant kernels' (parts_launch, dsp_device.cpp)
    std::unique_ptr<UploadedTable> formant_tables;   // ... and their float64 tables (formant.h formant_tables), uploaded the same way on first use
    PinnedBuf part_gains;           // generate_joined with a list: the parts' gains, [n] floats, where the levels' words are copied to (read under Model::mu, behind a stream wait)
    PinnedBuf trim_info;            // parts_launch: the ptts_trim_info records of its rows with a trim, grown to their count (read under Model::mu, behind a stream wait)
    RowRing<DspRow, kDspMaxEq * kDspEqBytes> dsp_ring;   // the DSP kernels', a table's equalisers behind its rows (dsp_device.cpp)
    int fc_inject = 0;   // test hook: the next k_flow_cluster launch (plain launches) runs with FlowClusterArgs::inject = this, once
    // k_flow_cluster's bounded hand-offs gave up (a tile's workgroups were not running together: a masked or shared device): the steps concerned were
    // re-issued as the 2 x depth launches (same bits) -- fc_fallbacks counts the events -- and this engine's batches keep the launches from then on
    std::atomic<int64_t> fc_fallbacks{0};
    std::atomic<bool> fc_disabled{false};

    ~Model();
    template <class T> const T* at(size_t off) const { return off == NONE ? nullptr : reinterpret_cast<const T*>(arena + off); }
    UploadArena upload;
    // by name only: an integer does not convert to a WorkSlot, so a call with a bare number does not compile
    DevBuf& work(WorkSlot slot, size_t bytes) {
        ws[slot].ensure(bytes);
        return ws[slot];
    }
    static_assert(!std::is_convertible<int, WorkSlot>::value && !std::is_convertible<size_t, WorkSlot>::value, "Model::work takes a WorkSlot name, never a number");
    void use_device() const { PTTS_HIP(hipSetDevice(device)); }
    // seeds of requests that name none (noise_seed == 0): a splitmix64 stream seeded with the clock when the model is opened
    // (the reference seeds its generator the same way, runtime_native_safetensors.go:27-32); never 0
    uint64_t noise_state = 0;
    uint64_t next_noise_seed() {
        uint64_t z = (noise_state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z ? z : 1;
    }
    const float* tcomb_for(int lsd_steps);
    void compute_tcomb(float s, float t, float* dst /* device [flow_dim] */);
};

// host rows packed into one work buffer of the model (host_rows.h: 256-byte aligned, a skipped row takes no bytes), and the copies of a row in
// and out, queued on s.  The caller holds Model::mu.
struct PackedRows {
    std::vector<size_t> bytes, off;
    char* base = nullptr;
    PackedRows(Model& m, WorkSlot slot, std::vector<size_t> row_bytes, const bool* skip = nullptr) : bytes(std::move(row_bytes)), off(bytes.size()) {
        base = m.work(slot, std::max<size_t>(pack_rows(bytes.data(), skip, (int)bytes.size(), off.data()), kRowAlign)).as<char>();
    }
    char* row(int i) const { return base + off[(size_t)i]; }
    void upload(int i, const void* src, hipStream_t s) const { PTTS_HIP(hipMemcpyAsync(row(i), src, bytes[(size_t)i], hipMemcpyHostToDevice, s)); }
    void download(int i, void* dst, hipStream_t s) const { PTTS_HIP(hipMemcpyAsync(dst, row(i), bytes[(size_t)i], hipMemcpyDeviceToHost, s)); }
};

// n_slots independent FlowLMState (flow_lm.go:45-49) in HBM + the per-step workspace
struct Batch {
    Model* m = nullptr;
    int B = 0;
    int cap = 0;             // KV capacity per slot (keys)
    int max_steps = 0;       // rows of `latents` per slot
    DevBuf kcache, vcache;   // [L][B][H][cap][hd]
    DevBuf state_i32;        // StepState arrays
    DevBuf state_f32;
    StepState st{};
    std::vector<int32_t> kv_len_host;
    // shared voice prefix: slots that took their first keys from a device-resident voice read them from the voice's own copy
    // in the AR step (one copy for the whole batch stays in L2) instead of from their private cache rows
    DevBuf pre_k, pre_v, pre_len;          // [B] device pointers to layer 0 of the voice's K / V, [B] prefix length (0: none)
    std::vector<const void*> pre_k_host, pre_v_host;
    std::vector<int32_t> pre_len_host;
    // step workspace
    DevBuf in_raw, in32, x, xn, qkv, attn, ff, last, eos, sy, ada, fx, fh, fh2, cur, noise_step, partial;
    DevBuf latents;          // [B][max_steps][ldim]
    DevBuf noise;            // [B][max_steps][ldim] or empty
    bool has_noise = false;
    bool opened = false;     // x and fx of the COMING step are in place: set by step_open and by a step whose last launch chained the next one's opening
    bool chain_ok = false;   // the shapes allow that chaining (StepFinish::ch in fin_dev)
    // a chained launch runs several blocks per row tile, so what it writes for the next step (fx, x0) must not be what its other blocks still read:
    // fx / cur alternate with fx2 / cur2 from one chained step to the next (par: which pair the coming step reads; 0 after every k_step_begin)
    DevBuf fx2, cur2;
    // the flow net's residual blocks as one launch (flow_cluster.hip): granule buffers and the tag / fault words; fc_ok: the model's shapes take it
    DevBuf fc_xbuf, fc_sync, fc_stamps;   // (fc_stamps: PTTS_FC_STAMPS measurement runs only)
    bool fc_ok = false;
    // tall.hip (batches of kTallMinRows rows and more): bf16 hi + lo row planes of the normalised residual rows [2][B][d_model] and of gelu(linear1) [2][B][ffn]
    DevBuf tp_a, tp_f;
    bool tall_ok = false;
    bool tail_fused = false;   // the step's last transformer launch also produced sy (silu(t + cond_embed)): the flow part can be re-issued from `last` / `sy` / `cur` as they stand
    unsigned* fc_fault() const { return fc_sync.as<unsigned>() + 32 * kFlowClusterMaxTiles; }
    int par = 0;
    float* fx_now() const { return (par ? fx2 : fx).as<float>(); }
    float* cur_now() const { return (par ? cur2 : cur).as<float>(); }
    hipStream_t io_stream = nullptr;   // continuous batch: voice ingestion and prefill of newcomers run here, beside the step chain on the model's stream
    bool slot_local = false; // continuous batch: per-slot device state (kv_len, voice prefix) is written slot by slot by the admit kernel, never as whole arrays
    // host-side upper bound on the cache length of any slot (set by voice/prompt ingestion, +1 per step): lets a step's
    // attention launch issue only the key loads that can be live (AttnArgs::keys_now).  capturing: a graph is being recorded,
    // its launches must cover the whole cache
    int kv_bound = 0;
    bool capturing = false;
    // graph replay of the AR step (use_graph): one captured step per attention round count (attn_step_rounds: the step
    // attention's load rounds follow the cache length, and a captured launch cannot change), captured on first use
    // [with sampling noise][attention rounds][0: one step, 1: graph_steps[.][0] steps (the short graphs), 2: graph_steps[.][1] steps (the long ones)]
    hipGraphExec_t graphs[2][17][3] = {};
    int graph_steps[2][2] = {{0, 0}, {0, 0}};   // steps per graph the second / third column was captured with
    int graph_lsd = 0;
    int capture_keys = 0;    // while capturing: the cache-length bound the recorded attention launches must cover
    // page-locked scratch of the generate loop: [0] live-utterance count, [1, 1+B) n_frames, [1+B, 1+2B) eos_step read back in
    // one copy after the loop; rows_pinned: the B result rows uploaded to the decoder (no pageable staging, no extra sync)
    int32_t* n_active_pinned = nullptr;
    PcmRow* rows_pinned = nullptr;
    DevBuf fin_dev;          // StepFinish: what the step's last launch needs for the bookkeeping it carries

    ~Batch();
    void drop_graphs();      // the captured step graphs go (and what their columns were captured with): the next replay captures again
    size_t kv_elem() const { return m->opts.kv == PTTS_KV_BF16 ? 2 : 4; }
    void* kc(int layer) const { return (char*)kcache.p + (size_t)layer * B * m->d.heads * cap * m->d.hd * kv_elem(); }
    void* vc(int layer) const { return (char*)vcache.p + (size_t)layer * B * m->d.heads * cap * m->d.hd * kv_elem(); }
};

// Result buffers (PCM) are page-locked so that the device-to-host copy runs at link speed (pageable: 12 GB/s measured, 5 ms per
// 64 x 10 s batch; pinned: ~50 GB/s).  Pinning is slow, so freed buffers go back to a process-wide pool.
void* result_alloc(size_t bytes);
void result_free(void* p);   // accepts pool blocks and plain malloc'ed pointers
bool result_is_pinned(const void* p);   // false for the pageable fallback blocks: those must not be written by a kernel

// a voice model state resident in HBM: K and V per layer as [H][offset][hd] in the cache dtype
struct Voice {
    Model* m = nullptr;
    int device = 0;   // m->device (freeing a voice never reads its model)
    int offset = 0;
    DevBuf k, v;
    size_t layer_bytes() const { return (size_t)m->d.heads * offset * m->d.hd * (m->opts.kv == PTTS_KV_BF16 ? 2 : 4); }
};
Voice* voice_create(Model& m, const float* const* caches, const int64_t* steps, const int64_t* offsets);
void batch_apply_voice(Batch& b, const Voice& v, const std::vector<int32_t>& slots);
bool voice_usable_by(const Voice& v, const Model& m);   // same GPU and cache geometry (e.g. engines made by model_share)
// cloned voices as model states (voice_build.cpp): embedding i (host [frames[i]][width] f32, width == d_model, 1 <= frames[i] <= ROPE_SEQ)
// prefilled alone from position 0 -- one batch_prompt of the embeddings as ragged prompts (per kStepMaxRows of them) -- and its first frames[i]
// KV rows of every layer moved into a compact Voice (offset = frames[i]) by one launch_voice_extract: what voice_create makes of the same caches.
// The caller holds m.mu; runs on m.stream.  Nothing is kept on a failure.
std::vector<std::unique_ptr<Voice>> voice_build(Model& m, const float* const* emb, const int64_t* frames, int64_t width, int n);
// layers [layer0, layer0 + n_layers) of a voice as the reference's caches, each [2, 1, offset, H, Dh] f32, one after the other in out (host);
// the exact inverse of what launch_voice_scatter reads (a bf16 cache widened exactly).  The caller holds v.m->mu.
void voice_export(const Voice& v, int layer0, int n_layers, float* out);
void voice_read_state(const Voice& v, int layer, float* out);
std::vector<uint8_t> voice_state_bytes(const Voice& v);   // the whole voice as a model-state file's bytes (voice_export + voice_state_file).  The caller holds v.m->mu

// buffers of one Mimi decode (all channels-last, spanning the whole utterance so that frame ranges can be decoded in order)
struct MimiWs {
    int B = 0, T = 0, P0 = 0;
    int Ls[4] = {0, 0, 0, 0}, Ps[4] = {0, 0, 0, 0};
    float *xp = nullptr, *up = nullptr, *n1 = nullptr, *qkv[MAX_LAYERS] = {nullptr}, *attn = nullptr, *ff = nullptr, *c0 = nullptr;
    float *u[3] = {nullptr, nullptr, nullptr}, *uo[3] = {nullptr, nullptr, nullptr}, *h[3] = {nullptr, nullptr, nullptr};
    bool zeroed = false;
};
constexpr int kMimiGroup = 64;   // utterances decoded together through one decoder workspace (generate: larger batches go group after group)
void mimi_setup(Model& m, MimiWs& w, int B, int T);
// pcm_rows (device array of B PcmRow, whole range only): the fused final block writes every utterance's samples straight to its
// row (page-locked host memory) instead of pcm; *rows_used says whether that path was taken (false: pcm holds the samples)
void mimi_range(Model& m, MimiWs& w, const float* lat, int64_t lat_bstride, int f0, int f1, float* pcm, float* mimi_latent, hipStream_t s,
                const PcmRow* pcm_rows = nullptr, bool* rows_used = nullptr, float* xformer_out = nullptr);

void mimi_layer_qkv(Model& m, int layer, const float* x, RowMap xmap, int R, float* qkv, RowMap qmap, int pos0, int rows_per_seg, float* n1, hipStream_t s);
void mimi_layer_ffn(Model& m, int layer, float* x, RowMap xmap, int R, float* n1, float* ffb, hipStream_t s);
// the same on any layer of that form (the encoder transformer's: Desc::Enc::ml)
void mimi_layer_qkv(Model& m, const Desc::ML& L, const float* x, RowMap xmap, int R, float* qkv, RowMap qmap, int pos0, int rows_per_seg, float* n1, hipStream_t s);
void mimi_layer_ffn(Model& m, const Desc::ML& L, float* x, RowMap xmap, int R, float* n1, float* ffb, hipStream_t s);

// Mimi encoder (encoder.cpp; PARITY UNPINNED, inferred chain: DESIGN.md section 7): clip i (n_samples[i] samples of 24 kHz mono f32, host) ->
// latent_out[i] (host, [mimi_encode_frames(n_samples[i])][mimi_dim]).  Clips are encoded one after another through one workspace sized for
// the longest, each from zero history, so a clip's bits never depend on the others.  stages (optional, one clip): kEncStages host buffers, see
// include/ptts_debug.h ptts_debug_encode_stages.
// A clip is at most mimi_encode_max_frames(d) frames long (PTTS_EINVAL above): the transformer's RoPE table covers ROPE_SEQ rows at the
// transformer's rate (8192 rows at 200 Hz: 512 frames = 40.96 s at full size).
constexpr int kEncStages = 10;
int64_t mimi_encode_max_frames(const Desc& d);
// rates (optional, per clip, 8000..192000): clips at other rates than 24000 are resampled on the device into the encoder's input; the frame cap
// applies to the resampled length
void mimi_encode(Model& m, const float* const* pcm, const int64_t* n_samples, int n_clips, float* const* latent_out, float* const* stages = nullptr,
                 const int32_t* rates = nullptr);
// one clip -> device latents lat_dev [frames][mimi_dim] on m.stream (the caller holds m.mu); returns the frame count
int64_t mimi_encode_clip(Model& m, const float* pcm, int64_t n_samples, float* lat_dev, float* const* stages = nullptr, int rate = kNativeRate);
int64_t mimi_encode_samples(int64_t n_samples, int rate);   // the 24 kHz samples a clip of n_samples at `rate` becomes (PTTS_EINVAL: a bad rate)
void require_encoder(const Desc& d);
void mimi_encode_stage_shapes(const Desc& d, int64_t n_samples, int64_t* shapes /* [kEncStages][2] (rows, channels) */);   // PTTS_EFORMAT naming the missing tensor on a checkpoint without encoder weights
Model* model_open(Plan* plan, void* device_arena, int fill);
void profile_read(Model& m, ptts_profile* out);   // ptts_profile_read behind its lock: the figures of the measurement pass, counters reset (runtime.cpp)
Batch* batch_new(Model& m, int n_slots, int cap, int max_steps);
void batch_reset(Batch& b);
void batch_set_voice(Batch& b, int slot, const float* const* caches, const int64_t* steps, const int64_t* offsets);
// rows: device [R, d_model]; row_offsets host [B+1]
void batch_prompt(Batch& b, const float* rows_dev, const int64_t* row_offsets);
// core of one AR step on device state: in32 [B, ldim], cur [B, ldim] (= x0) -> cur (= frame), eos, last; appends KV at kv_len
// opened: x and fx were produced by step_open; fuse_finish: the bookkeeping of k_step_finish rides in the last launch -- returns
// whether it did (false: the caller launches k_step_finish)
// chain (with fuse_finish): the last launch also opens the next step (sets b.opened); the frame then lives in the latents only, b.cur holds the next x0
bool step_core(Batch& b, int lsd_steps, bool opened = false, bool fuse_finish = false, bool chain = false);
void step_open(Batch& b);
// A hand-off inside k_flow_cluster timed out (the fault word of the batch is set).  flow_cluster_recover clears the exchange state, switches the batch (and
// the engine's later batches) to the 2 x depth launches and counts the event; flow_cluster_fault does that and throws FlowClusterFault: the caller owns a
// retry -- generate() runs the chunk again on the launches, the staged step re-issues its flow part, the dispatcher re-queues what was in flight.
struct FlowClusterFault : Error { using Error::Error; };
void flow_cluster_recover(Batch& b);
void flow_cluster_fault(Batch& b);
void step_flow_again(Batch& b, int lsd_steps);   // the LSD decode of the step just taken, once more, from the intact `last` / `sy` and the caller-restored `cur` (staged API)
                                    // first launch of a generate step (input, noise, the two 32-wide linears)
// xformer_out (optional, staged parity checks): the decoder transformer's output rows [B][T * up_stride][mimi_dim]
void mimi_decode(Model& m, const float* lat_dev, int64_t lat_bstride, int B, int T, float* pcm_dev, float* mimi_latent_dev, float* xformer_out = nullptr);
// pieces of the generate loop that the continuous batch (continuous.cpp) reuses
struct UploadScope { UploadScope(UploadArena& a, hipStream_t s); UploadScope(UploadArena& a, hipEvent_t last_use); ~UploadScope(); };   // small uploads of this thread are staged page-locked, no waits
void h2d(void* dst, const void* src, size_t bytes, hipStream_t s);
void d2h(void* dst, const void* src, size_t bytes, hipStream_t s);
int resolve_max_steps(const ptts_request& r);                                   // runtime_native_safetensors.go:61-67
inline int request_lsd(const ptts_request& r) { return r.lsd_steps <= 0 ? 1 : r.lsd_steps; }   // the Euler steps of the request's LSD decode
// the frames of one utterance the decoder reaches: its RoPE table ends at ROPE_SEQ positions (mimi.go:498)
inline int mimi_frame_limit(const Desc& d) { return ROPE_SEQ / d.up_stride; }
void enqueue_step(Batch& b, int lsd, bool use_graph, int nsteps = 1);           // nsteps > 1 only with use_graph
// the K slices the step's split linear runs a [M][K] x [N][K]^T product in (1: whole); the short prompt's linear2 (batch.cpp) asks as well
int pick_split(int M, int N, int K, bool w_bf16 = false);
// the two ldim-wide linears at the head of a step, as the opening kernels take them; false: shapes they do not take (step_core then runs them as step linears)
bool open_linears(Batch& b, StepOpenLinears& lin);
void mimi_zero_history(Model& m, MimiWs& w, hipStream_t s);
// Request staging and result delivery, one copy for generate() (every slot of its batch) and the continuous batch (its newcomers /
// each group of finished utterances).  The callers keep their own bookkeeping: batch_reset or the slots' host state, the step
// budgets and EOS settings, their UploadScope.
struct SlotReq { int slot; const ptts_request* req; int max_steps; };   // max_steps: resolve_max_steps(*req)
// voices (device voices grouped per Voice, host caches slot by slot), prompt rows packed per slot (list: ascending slots; the others get
// empty segments), embedding gather, batch_prompt; before_prefill (optional) is recorded on s just in front of batch_prompt
void stage_prompt(Batch& b, const std::vector<SlotReq>& list, hipStream_t s, hipEvent_t before_prefill = nullptr);
// the listed slots' noise rows (b.noise, [B][max_steps][ldim]), sampling noise as flow_lm.go:283-288,386-408 makes it: injected rows as
// they are; otherwise N(0,1) * sqrt(temperature) drawn on the device per (seed, step), one launch_noise_fill; temperature <= 0: zeros.
// All of it is resident before the slot's first step, so the AR loop (plain launches or graph replay) just reads row `step` of its slot.
void stage_noise(Batch& b, const std::vector<SlotReq>& list, hipStream_t s);
// one decoded row of a group of finished utterances that one mimi_range call decodes
struct Delivery {
    const ptts_request* req = nullptr;
    ptts_result* res = nullptr;   // nullptr: decoded but not delivered (cancelled, failed)
    int nf = 0, eos = -1;
    bool filled = false;          // res already holds a buffer with every sample (streamed): no allocation, no copy
    int64_t n24 = -1;             // the row's samples at 24 kHz where they are not nf frames' worth (generate_joined's joined row); -1: nf * spf
    int64_t samples(int64_t spf) const { return n24 >= 0 ? n24 : (int64_t)nf * spf; }
};
// before the decode: result buffers into the results (PCM16 or f32), and the device PcmRow table for mimi_range's direct store (host_rows:
// page-locked, g.size() entries, uploaded on s into dev_rows).  With it the decoder's last kernel stores every utterance's samples straight
// into its page-locked result buffer: the kernel's stores ARE the device -> host transfer -- no copies, no conversion launch.  A kernel may
// only store into page-locked memory: if the pool had to fall back to pageable blocks, nullptr (the group takes the device buffer + copy
// path).  A failed allocation leaves its row empty (the request ends with PTTS_ENOMEM); the others keep the direct store.
const PcmRow* results_alloc(const Model& m, const std::vector<Delivery>& g, PcmRow* host_rows, PcmRow* dev_rows, hipStream_t s);
// after it: unless the decoder stored the samples itself, PCM16 conversion and the copies out of pcm (row i at i * pcm_stride); the
// latents (row i at lat + i * lat_stride); status, n_frames, eos_step, n_samples.  Everything is queued on s.
void results_deliver(Model& m, const std::vector<Delivery>& g, bool stored, const float* pcm, int64_t pcm_stride, const float* lat, int64_t lat_stride,
                     hipStream_t s);
// rates (resample.cpp): positive multiples of 25 Hz, 8000..48000 for output and 8000..192000 for input; the message names a bad rate or a
// pair whose tap table exceeds kResampleMaxL / kResampleMaxTaps (empty: fine)
std::string rate_error(int64_t rate, bool input);
std::string rate_pair_error(int in_rate, int out_rate);
int64_t resample_length(int64_t n_in, int in_rate, int out_rate);           // ceil(n_in L / M); the pair must be valid
// the pair's filter, built and uploaded on first use (nullptr: in_rate == out_rate, the identity); throws PTTS_EINVAL for a bad pair
const RateFilter* rate_filter(Model& m, int in_rate, int out_rate, hipStream_t s);
int64_t resample_ready(const RateFilter* f, int64_t n_dec);                  // outputs whose filter support lies inside the first n_dec inputs
ResampleRow resample_row(const RateFilter* f, const float* src, int64_t n_in, void* dst, int64_t o0, int64_t o1, int fmt);
void resample_launch(Model& m, const std::vector<ResampleRow>& rows, hipStream_t s);   // one k_resample launch per RowRing::kRows rows
// a request's egress: its rate (0 -> 24000), whether it needs k_resample (another rate, or G.711), the bytes per sample of its format, and
// its result buffer (pcm / pcm16 / pcm8 by format)
inline int request_rate(const ptts_request& r) { return r.sample_rate ? r.sample_rate : kNativeRate; }
// post-processing on the device (dsp_device.cpp, dsp.hip).  A row is resolved into a DspSpec (dsp_spec.h) before it is launched; whether a
// request may have any at all is asked without resolving it (dsp_active: one registry look-up at the most, no error).  An ext counts unseen
// here, as an eq does in dsp_active: the answer decides before the decode whether the decoder may store straight into the result
// (results_alloc), and must not turn to "no" because the handle died since admission -- such a request stays on the device-buffer path, where
// results_deliver resolves it and refuses it.  (A live ext that switches nothing on costs its request the direct store, nothing else.)
inline bool request_postprocesses(const ptts_request& r) { return dsp_active(r.dsp) || (r.dsp && r.dsp->ext) || r.loudness != 0; }
inline bool request_converts(const ptts_request& r) {   // (a request with post-processing leaves through the device buffer as well)
    return request_rate(r) != kNativeRate || r.pcm_format == PTTS_PCM_ULAW || r.pcm_format == PTTS_PCM_ALAW || request_postprocesses(r);
}
double loud_target_power(double target_lufs);   // 10^((target + 0.691) / 10)
// a row's loudness: measured, and normalised to *target_lufs (NULL: measured only, for a dsp_launch with apply == false)
inline void dsp_spec_loudness(DspSpec& spec, const double* target_lufs) { spec.loud = true; spec.target_power = target_lufs ? loud_target_power(*target_lufs) : 1.0; }
// one row of the chain: x, n samples at 24 kHz on the device, rewritten in place as spec says.  dsp_launch sets loud_out to a loudness row's two
// device words (the mean square M as a double, then the f32 gain) and tp_out to a true-peak row's (the true peak's uint32 image); both are valid
// until the model's next DSP launch
struct DspJob {
    float* x; int64_t n; DspSpec spec; double* loud_out = nullptr; uint32_t* tp_out = nullptr;
    // a window of the row (kernels.h; only the causal stages: dsp_window_refusal): the launches cover tiles [t0, ceil(n / 1920)), n the samples up
    // to the window's end; open: more samples follow behind n (a multiple of 1920), n_row is then the length the fade in is clamped by; carry:
    // the row's carried states on the device, [kCarryDoubles], zero in front of its first window (null: a one-shot row)
    int64_t t0 = 0; bool open = false; int64_t n_row = INT64_MAX; double* carry = nullptr;
};
// the launches for a table of rows on s.  apply false: loudness and true-peak rows are measured only, no sample is rewritten
void dsp_launch(Model& m, std::vector<DspJob>& jobs, hipStream_t s, bool apply = true);
// the chain on host rows, one round trip: rows packed into one device buffer and uploaded, dsp_launch, the outputs read back, one wait.  Takes
// Model::mu.  A row of no samples, or whose spec switches nothing on, takes no device bytes (and is copied on the host when out is given).
// Outputs, each optional: out [rows] the samples (out[i] == in[i] is fine); M [rows] the mean squares of loudness rows (0: none); sub [rows] their
// [4 ceil(n / 1920)] sub-block energies as the device computed them; true_peaks [rows] (0: none)
struct DspRowsOut { float* const* out = nullptr; double* M = nullptr; std::vector<double>* sub = nullptr; float* true_peaks = nullptr; };
void dsp_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const DspSpec* per_row, bool apply, const DspRowsOut& o);
// ptts_debug_dsp_windows: spec's causal stages over rows of host samples, window after window by the launches a streamed joined call runs: window
// w is [cuts[w - 1], cuts[w]) of every row that has samples there (cuts: ascending multiples of 1920, checked by the caller), behind the last cut
// one more to each row's end; a row is open in a window when it goes on behind it.  The carried states stay on the device.  Takes Model::mu
void dsp_windows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const DspSpec& spec, const int64_t* cuts, int32_t n_cuts, float* const* out);
inline size_t pcm_bytes(int fmt) { return fmt == PTTS_PCM_F32 ? 4 : fmt == PTTS_PCM_S16 ? 2 : 1; }
inline void* result_buffer(const ptts_result& r, int fmt) {
    return fmt == PTTS_PCM_F32 ? (void*)r.pcm : fmt == PTTS_PCM_S16 ? (void*)r.pcm16 : (void*)r.pcm8;
}
inline void set_result_buffer(ptts_result& r, int fmt, void* p) {
    if (fmt == PTTS_PCM_F32) r.pcm = (float*)p;
    else if (fmt == PTTS_PCM_S16) r.pcm16 = (int16_t*)p;
    else r.pcm8 = (uint8_t*)p;
}
inline int64_t egress_length(const ptts_request& r, int64_t n24) {   // samples at the request's rate of n24 decoded ones
    return request_rate(r) == kNativeRate ? n24 : resample_length(n24, kNativeRate, request_rate(r));
}
Model* model_share(Model& base);   // another engine over base's weight arena (base must outlive it)
Model* model_replicate(Model& base, int device);   // the model on another GPU of this process: own arena, copied from base's by hipMemcpyPeer
void generate(Model& m, const ptts_request* reqs, int n, ptts_result* res);
std::string request_error(const Desc& d, const ptts_request& q);   // empty: the request is well formed
// Joined synthesis (join.h has the rule; include/ptts.h ptts_generate_joined): the requests as generate() runs them, in text order; each
// group's decoded rows go through k_join into one device row for the text (Chunk::deliver, behind the fault check), then one DspJob over that
// row and the egress of one row into *out.  parts: [n] or null.  Throws for a refusal (nothing launched) and for a failed chunk
// so (include/ptts.h ptts_generate_joined_streamed; null: ptts_generate_joined): the first group's size, and with a pcm_callback the chain runs
// window after window behind each group's k_join (DspJob's windows) and the audio that is final is handed over from a host function
// list (include/ptts.h ptts_generate_joined_parts; null: one setting for the whole call): one ptts_part_opts per part -- its stages, its volume and the
// seam behind it -- and where the parts' gains go ([n] or null)
struct JoinPartsList { const ptts_part_opts* po; float* gains; };
void generate_joined(Model& m, const ptts_request* reqs, int n, const ptts_join_opts& o, const ptts_join_stream_opts* so, ptts_result* out, ptts_join_part* parts,
                     const JoinPartsList* list = nullptr);
// k_join over a list of rows on s, one launch per RowRing::kRows rows
void join_launch(Model& m, const std::vector<JoinRow>& rows, hipStream_t s);
// ptts_join_rows: the parts packed into one device buffer with the joined row behind them, uploaded, join_launch, the joined row back, one wait.
// Takes Model::mu.  The lengths are planned (join_plan) and out holds the joined length
void join_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const JoinLens& l, float* out);
// Per-part options (include/ptts.h ptts_part_opts; join.h).  A part's volume on the device: none, a fixed gain, or a level whose gain the loudness
// rows' measuring kernels leave in a device word (level_launch)
struct PartGain { bool fixed = false; float g = 1.0f; const float* word = nullptr; };
// the measuring launches of the loudness rows (k_dsp_peak, k_loud_summary .. k_loud_gate) over device rows x[i][0, n[i]) with target power
// target[i], on s: nothing is rewritten.  words[i] receives where row i's f32 gain lies (WORK_PART_LEVEL, valid until the model's next level_launch)
void level_launch(Model& m, const std::vector<const float*>& x, const std::vector<int64_t>& n, const std::vector<double>& target, std::vector<const float*>& words,
                  hipStream_t s);
// k_join_gain over a list of rows on s, one launch per RowRing::kRows rows; a table of the list in which no row has a flag goes to k_join
void join_gain_launch(Model& m, const std::vector<JoinGainRow>& rows, hipStream_t s);
// a JoinRow with its gains: mine the part's, prev (null: none, or a tail that lies in the joined row and is already scaled) its predecessor's
JoinGainRow join_gain_row(const JoinRow& r, const PartGain& mine, const PartGain* prev);
// the parts' volumes on device rows x[i][0, n[i]): the fixed gains as they are, the levels' words from one level_launch over the rows that have one
std::vector<PartGain> part_gains_launch(Model& m, const std::vector<const float*>& x, const std::vector<int64_t>& n, const std::vector<PartVolume>& vol, hipStream_t s);
// ptts_join_parts_rows: join_rows_device with the seams of the list and the parts' volumes; gains (optional, [rows]) receives the gains applied
void join_parts_rows_device(Model& m, const float* const* in, const int64_t* n, int32_t rows, const JoinSeams& seams, const std::vector<PartVolume>& vol, float* out,
                            float* gains);
// What one part of a joined text gets in front of the join (and one row of ptts_trim_rows, ptts_tempo_rows, ptts_pitch_rows), resolved: the trim,
// then the resampling step of the pitch (p is not 1000), then the tempo (behind a pitch it carries the effective speed E, pitch.h pitch_steps).
// Null: the step is not run.  formant (with a pitch alone): the resampling step runs on the row's residual, between k_formant_whiten and k_formant_shape
struct PartStages { const TrimScan* trim = nullptr; const PitchScan* pitch = nullptr; const TempoScan* tempo = nullptr; bool formant = false; };
// One row of parts_launch.  The caller states src, n and st, and a device destination for each step the row has, sized for the bound that step's
// own length function gives for the longest the row can be in front of it (trimmed: n; shifted: pitch_resample_length; scaled: tempo_length).
// parts_launch states where the row's final form lies (src itself without a step), its length, and its trim record (without a trim: untouched)
struct PartRow {
    const float* src; int64_t n; PartStages st;
    float* trimmed = nullptr; float* shifted = nullptr; float* scaled = nullptr;
    const float* out = nullptr; int64_t n_out = 0; ptts_trim_info info{};
};
// The one chain of the part stages on device rows, on s, in this order: the trim's launches (trim.hip; trim.h has the rule) for the rows with a trim,
// their records back in one copy into page-locked memory (Model::trim_info) behind one stream wait -- the lengths decide everything behind them --
// then k_pitch_resample (pitch.hip; pitch.h) for the rows with a pitch -- for those that keep their formants (formant.hip; formant.h) on the residual,
// between k_formant_analyse and k_formant_whiten in front and k_formant_shape behind, in work buffers made here -- and the tempo's launches (tempo.hip; tempo.h) for the rows with a tempo.
// Each stage's scratch and row tables are made here, one launch sequence per table.  phase (optional) is called with "trim", "pitch" and "tempo"
// behind the launches of a stage that ran; unit: what the caller's rows are called in the internal check of the records.  The caller holds Model::mu
void parts_launch(Model& m, std::vector<PartRow>& rows, hipStream_t s, const std::function<void(const char*)>& phase = nullptr, const char* unit = "row");
// ptts_trim_rows, ptts_tempo_rows and ptts_pitch_rows, one round trip: the rows packed into one device buffer with the forms each row's steps need
// behind them, uploaded, parts_launch, each row's final form back, one wait behind the copies.  Takes Model::mu.  A row with no step is copied on
// the host; one whose result is empty is left alone.  n_out [rows] (optional): what out[i] received; info [rows] (optional): the trim records,
// preset to "nothing cut"
void part_rows_device(Model& m, const PartStages* per_row, const float* const* in, const int64_t* n, int32_t rows, float* const* out, int64_t* n_out,
                      ptts_trim_info* info);

// ---- the staged entry points' device side (staged.cpp): the pipeline's pieces one call at a time, behind include/ptts.h's ptts_text_embeddings,
// ptts_batch_prompt / _step / _read_kv, ptts_decode_latents, ptts_noise_rows, ptts_flow_direction, ptts_speaker_project, ptts_resample / ptts_pcm_encode
// and the voice entry points.  One convention: the CALLER holds Model::mu and has selected the device (the extern "C" function, behind its argument
// checks); each function runs on Model::stream, takes host operands and results unless it says otherwise, and returns with the stream drained ----
void staged_text_embeddings(Model& m, const int64_t* ids, int64_t n, float* out);   // n > 0 ids, checked -> out [n][d_model]
void staged_prompt(Batch& b, const float* emb, const int64_t* row_offsets);         // the rows uploaded, then batch_prompt
// one AR step: NaN rows of frames_in replaced by BOS, noise (null: zeros) as x0, step_core; a k_flow_cluster hand-off that gave up is recovered here
// (flow_cluster_recover, the flow part again from the saved x0: the same bits); kv_len + 1; the optional outputs back
void staged_step(Batch& b, const float* frames_in, int lsd_steps, const float* noise, float* frames_out, float* eos_logits, float* last_hidden);
void staged_read_kv(const Batch& b, int slot, int layer, float* k, float* v);       // a slot's keys and values of one layer as f32 [H][kv_len][hd]
// LatentToMimi + MimiDecode of [n_utt][frames][ldim]; pcm, mimi_latent, transformer_out (the decoder transformer's rows, staged parity checks) optional
void staged_decode(Model& m, const float* latents, int n_utt, int frames, float* pcm, float* mimi_latent, float* transformer_out);
void staged_noise_rows(Model& m, uint64_t seed, float temperature, int rows, float* out);   // stage_noise's draw for one seed: [rows][ldim]
void staged_flow_direction(Model& m, const float* c, float sv, float tv, const float* x, int n, float* out);   // flowNet.Forward on n rows, many-row kernels only
// n host rows -> n host rows through one device buffer each way (PackedRows), one k_resample launch per RowRing::kRows rows; f null: format only
void staged_convert(Model& m, const float* const* in, const int64_t* n_in, int32_t n, const RateFilter* f, const int64_t* n_out, int fmt, void* const* out);
// the speaker projection, THE one place that builds it: device latents [frames][speaker_proj.in] -> device rows [frames][d_model], queued, no wait
void speaker_project_device(Model& m, const float* lat, int64_t frames, float* out);
void staged_speaker_project(Model& m, const float* latent, int64_t frames, float* out);     // ... on host latents
// one clip -> its voice embedding in out (host, [ceil(n24 / hop)][d_model]): mimi_encode_clip, then the projection where the encoder left the latents; the frame count
int64_t voice_embedding_device(Model& m, const float* pcm, int64_t n_samples, float* out, int rate = kNativeRate);

// text front end (text.cpp; internal/text/prepare.go, chunk.go)
struct TextChunk {
    std::string text;
    std::vector<int64_t> token_ids;
    int num_words = 0, max_frames = 0, frames_after_eos = 0;
};
typedef std::function<std::vector<int64_t>(const std::string&)> TextEncodeFn;
int text_count_words(const std::string& s);
int text_estimate_max_frames(int64_t token_count, double frame_rate);
int text_frames_after_eos(int64_t num_words);
std::string text_prepare(const std::string& input);
std::vector<std::string> text_split_sentences(const std::string& text);
std::vector<TextChunk> text_chunks(const std::string& input, const TextEncodeFn& encode, int max_tokens, double frame_rate);

// SentencePiece unigram encoder (tokenizer.cpp; internal/tokenizer/sentencepiece.go, sentencepiece_bytes_wasm.go)
struct Tokenizer;
Tokenizer* tokenizer_from_bytes(const void* data, size_t len);
Tokenizer* tokenizer_from_path(const std::string& path);
std::vector<int64_t> tokenizer_encode(const Tokenizer& t, const std::string& text);
size_t tokenizer_vocab(const Tokenizer& t);
void tokenizer_free(Tokenizer* t);
std::string nfkc_utf8(const std::string& s);

// voice files (voicefile.cpp; internal/safetensors/reader.go:69-140,232-308, internal/native/flow_transformer.go:451-590): host only
struct VoiceFile {
    StFile st;
    int kind = 0;                                        // PTTS_VOICE_FILE_*
    std::vector<float> emb; std::vector<int64_t> emb_shape;   // LoadVoiceEmbedding: [1, T, D]
    std::string emb_error;                               // why the first tensor is no embedding (1-D, 4-D ...)
    struct Tensor { std::vector<int64_t> shape; std::vector<float> data; };
    struct Module { std::string name; std::map<std::string, Tensor> tensors; };
    std::vector<Module> modules;                         // LoadVoiceModelState: sorted by name; "current_end" already turned into "offset"
    std::string state_error;
};
VoiceFile* voice_file_from_path(const std::string& path);
VoiceFile* voice_file_from_bytes(const void* data, size_t len);
void voice_file_embedding(const VoiceFile& v, const float** data, int64_t shape[3]);
void voice_file_require_state(const VoiceFile& v);
void voice_file_state(const VoiceFile& v, int n_layers, int heads, int head_dim, const float** caches, int64_t* steps, int64_t* offsets);
// the writer (voicefile_write.cpp): a model-state file (per layer `transformer.layers.{l}.self_attn/cache` F32 [2,1,offset,heads,head_dim] from
// caches[l] and `/offset` I64 [1]; no padding rows) and a legacy-embedding file (`audio_prompt` F32 [1, frames, dim]), as file bytes
std::vector<uint8_t> voice_state_file(const float* const* caches, int64_t offset, int n_layers, int heads, int head_dim);
std::vector<uint8_t> voice_embedding_file(const float* emb, int64_t frames, int64_t dim);
void write_file(const std::string& path, const std::vector<uint8_t>& bytes);   // PTTS_EIO on failure

// optional post-processing of a finished utterance (dsp.cpp; internal/audio/dsp.go)
void dsp_peak_normalize(float* s, int64_t n);
void dsp_dc_block(float* s, int64_t n, int sample_rate);
void dsp_fade_in(float* s, int64_t n, int sample_rate, double ms);
void dsp_fade_out(float* s, int64_t n, int sample_rate, double ms);
struct DspScan;
DspScan dsp_scan_coeffs(int sample_rate);                          // the DC block's section and the powers of its state matrix (scan_block.h)
void dsp_dc_block_blocked(float* s, int64_t n, int sample_rate);   // dsp_dc_block in the device's blocked form, on the host

// integrated loudness, ITU-R BS.1770-4 mono at 24 kHz (loudness.cpp; scan_block.h is the arithmetic, shared with dsp.hip)
struct LoudScan;
void loud_kweight_coeffs(int sample_rate, double out[10]);         // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
LoudScan loud_scan_coeffs(int sample_rate);
const LoudScan& loud_scan();                                       // at kNativeRate
double loud_lufs(double M);                                        // -0.691 + 10 log10(M); -inf for M == 0
std::string loud_target_error(double target_lufs);                 // empty: -70 <= target <= -1
void loud_sub_energies(const float* x, int64_t n, std::vector<double>& sub);   // [4 ceil(n / 1920)]: 480-sample energies, blocked form
double loud_gated_mean(const double* sub, int64_t n);              // the doubly gated mean square M (0: nothing above the gates)
double loud_measure(const float* x, int64_t n);                    // M of a row
float loud_measure_gain(const float* x, int64_t n, double target_power, double* M_out);   // min((float)sqrt(T / M), 1 / peak), or 1
double loud_normalize(float* x, int64_t n, double target_lufs);    // in place; returns M as measured before

// the weight broadcast of a multi-GPU start-up (broadcast.cpp)
void rccl_unique_id(uint8_t out[128]);
void rccl_broadcast(void* device_buf, size_t bytes, int rank, int n_ranks, const uint8_t id[128], int device);

// continuous batch of one model (continuous.cpp): fixed slots / KV capacity / step budget; used by the dispatcher's continuous mode
struct ContEngine;
ContEngine* cont_create(Model& m, int slots, int kv_cap, int max_steps);
void cont_destroy(ContEngine* e);
bool cont_accepts(const ContEngine& e, const ptts_request& r);   // fits the geometry and needs no per-step host work
int cont_free_slots(const ContEngine& e);
int cont_busy(const ContEngine& e);                               // utterances generating + groups being decoded
bool cont_admit_now(const ContEngine& e, int waiting);              // admission pacing: see continuous.cpp
void cont_admit(ContEngine& e, const ptts_request* const* reqs, ptts_result* const* results, void* const* tags, int n);
void cont_advance(ContEngine& e, int steps, std::vector<void*>& done, bool drain);
void cont_occupancy(const ContEngine& e, int64_t* steps, int64_t* slot_steps);   // AR steps launched so far; utterances stepping in them, summed
void cont_abort(ContEngine& e, int code, std::vector<void*>& done);

// request dispatcher (dispatcher.cpp)
struct Dispatcher;
typedef int (*ExecFn)(void* user, int worker, const ptts_request* reqs, int32_t n, ptts_result* results, char* err, int32_t errlen);
struct DispatchCont { int on = 0, kv_capacity = 0, max_steps = 0, steps_per_group = 0; };   // ptts_dispatch_opts: continuous batching
Dispatcher* dispatcher_create(Model* const* models, int n_models, ExecFn exec, void* user, int n_workers, int max_batch, int window_us, int queue_cap,
                              const DispatchCont* cont = nullptr);
void dispatcher_close(Dispatcher* d);
int dispatcher_generate(Dispatcher* d, const ptts_request* req, ptts_result* res, std::string* err);
void dispatcher_stats(Dispatcher* d, ptts_dispatch_stats* out);

}  // namespace ptts
