"""Host-side mirror of the reference's Runtime seam over the C ABI (include/ptts.h).

Reference: `tts.Runtime` (internal/tts/runtime.go:42-45), `RuntimeGenerateConfig` (:17-31),
`VoiceEmbedding` (:11-14), `nativeSafetensorsRuntime` (runtime_native_safetensors.go:20-244).
The reference toolchain (Go) is absent from the build image, so this ctypes layer plays the
role the cgo shim in INTEGRATION.md plays for the Go service: same method names, argument
meaning and error behaviour.  There is no CPU fallback: if libptts_hip.so is missing or no
HIP device is visible, every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTTS_LIB_PATH") or os.path.join(_HERE, "libptts_hip.so")   # PTTS_LIB_PATH: A/B of two builds on one box (tools/gpu_r3.sh)

PTTS_OK, PTTS_EINVAL, PTTS_EIO, PTTS_EFORMAT, PTTS_ENODEVICE, PTTS_ECANCELLED, PTTS_ENOMEM = range(7)
WEIGHTS_F32, WEIGHTS_BF16, WEIGHTS_INT8 = 0, 1, 2
KV_F32, KV_BF16 = 0, 1
PCM_F32, PCM_S16, PCM_ULAW, PCM_ALAW = 0, 1, 2, 3   # ptts_request.pcm_format
_PCM_DTYPES = {PCM_F32: "<f4", PCM_S16: "<i2", PCM_ULAW: "|u1", PCM_ALAW: "|u1"}

_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int64)
_DP = C.POINTER(C.c_double)
_I32P = C.POINTER(C.c_int32)
_U16P = C.POINTER(C.c_uint16)
_STEP_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32)
_PCM_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)


class PttsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class Cancelled(PttsError):
    """ctx.Err() of the reference (runtime_native_safetensors.go:156-159)."""


class _Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("weights", C.c_int32), ("kv", C.c_int32), ("max_batch", C.c_int32),
                ("use_graph", C.c_int32), ("reserved0", C.c_int32), ("reserved", C.c_int32 * 10)]


class _Info(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("d_model", "n_heads", "n_layers", "ffn", "ldim", "n_bins", "flow_dim", "flow_depth",
                                         "mimi_dim", "mimi_heads", "mimi_layers", "mimi_context", "sample_rate",
                                         "samples_per_frame", "steps_per_latent")] + \
               [("frame_rate", C.c_double), ("encoder_frame_rate", C.c_double), ("n_params", C.c_int64),
                ("arena_bytes", C.c_int64), ("weights", C.c_int32), ("kv", C.c_int32)]


class _DspHandles(C.Structure):   # eq lies over reserved[0..1], ext over reserved[2..3]
    _fields_ = [("eq", C.c_void_p), ("ext", C.c_void_p)]


class _DspTail(C.Union):   # the anonymous union at the end of ptts_dsp_opts
    _anonymous_ = ("_handles",)
    _fields_ = [("reserved", C.c_int32 * 4), ("_handles", _DspHandles)]


class DspOpts(C.Structure):   # ptts_dsp_opts
    _anonymous_ = ("_tail",)
    _fields_ = [("normalize", C.c_int32), ("dc_block", C.c_int32), ("fade_in_ms", C.c_double), ("fade_out_ms", C.c_double), ("_tail", _DspTail)]


class DspExtOpts(C.Structure):   # ptts_dsp_ext_opts
    _fields_ = [("size", C.c_uint32), ("true_peak", C.c_int32), ("ceiling_dbtp", C.c_double)]


class CompressorOpts(C.Structure):   # ptts_compressor_opts
    """A dynamic range compressor's options (ptts_compressor_opts): threshold_db -60 .. 0, ratio 1 .. 100, knee_db 0 .. 24, attack_ms 0.05 .. 200,
    release_ms 5 .. 5000, makeup_db -24 .. 24.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_int32), ("threshold_db", C.c_double), ("ratio", C.c_double), ("knee_db", C.c_double),
                ("attack_ms", C.c_double), ("release_ms", C.c_double), ("makeup_db", C.c_double)]

    def __init__(self, threshold_db: float = -24.0, ratio: float = 4.0, knee_db: float = 6.0, attack_ms: float = 5.0, release_ms: float = 120.0,
                 makeup_db: float = 0.0, size: Optional[int] = None, reserved: int = 0):
        super().__init__(C.sizeof(CompressorOpts) if size is None else int(size), int(reserved), float(threshold_db), float(ratio), float(knee_db),
                         float(attack_ms), float(release_ms), float(makeup_db))


class LimiterOpts(C.Structure):   # ptts_limiter_opts
    """A look-ahead peak limiter's options (ptts_limiter_opts): ceiling_db -60 .. 0, lookahead_ms 0.25 .. 5, release_ms 5 .. 5000, drive_db 0 .. 24.
    size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_int32), ("ceiling_db", C.c_double), ("lookahead_ms", C.c_double),
                ("release_ms", C.c_double), ("drive_db", C.c_double)]

    def __init__(self, ceiling_db: float = -1.0, lookahead_ms: float = 1.5, release_ms: float = 80.0, drive_db: float = 0.0,
                 size: Optional[int] = None, reserved: int = 0):
        super().__init__(C.sizeof(LimiterOpts) if size is None else int(size), int(reserved), float(ceiling_db), float(lookahead_ms),
                         float(release_ms), float(drive_db))


class DeesserOpts(C.Structure):   # ptts_deesser_opts
    """A de-esser's options (ptts_deesser_opts): freq_hz 2000 .. 10000 and q 0.3 .. 4 of the side chain's high-pass, then the compressor's detector on
    that band -- threshold_db -60 .. 0, ratio 1 .. 100, knee_db 0 .. 24, attack_ms 0.05 .. 200, release_ms 5 .. 5000 -- and max_reduction_db 0 .. 40,
    the most the band is turned down by.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_int32), ("freq_hz", C.c_double), ("q", C.c_double), ("threshold_db", C.c_double),
                ("ratio", C.c_double), ("knee_db", C.c_double), ("attack_ms", C.c_double), ("release_ms", C.c_double), ("max_reduction_db", C.c_double)]

    def __init__(self, freq_hz: float = 5000.0, q: float = 0.7071, threshold_db: float = -30.0, ratio: float = 4.0, knee_db: float = 6.0,
                 attack_ms: float = 1.0, release_ms: float = 60.0, max_reduction_db: float = 12.0, size: Optional[int] = None, reserved: int = 0):
        super().__init__(C.sizeof(DeesserOpts) if size is None else int(size), int(reserved), float(freq_hz), float(q), float(threshold_db),
                         float(ratio), float(knee_db), float(attack_ms), float(release_ms), float(max_reduction_db))


class TrimOpts(C.Structure):   # ptts_trim_opts
    """Silence control of a joined call's parts (ptts_trim_opts): edges 0 / 1 (cut the silent head and tail), threshold_db -120 .. 0 (a sample is
    loud when |x| > 10^(threshold_db / 20)), pad_ms 0 .. 500 (kept around the first and last loud sample), max_pause_ms 0 (pauses untouched) or
    20 .. 5000 (the longest pause that stays).  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("edges", C.c_int32), ("threshold_db", C.c_double), ("pad_ms", C.c_double), ("max_pause_ms", C.c_double)]

    def __init__(self, edges: int = 1, threshold_db: float = -50.0, pad_ms: float = 30.0, max_pause_ms: float = 0.0, size: Optional[int] = None):
        super().__init__(C.sizeof(TrimOpts) if size is None else int(size), int(edges), float(threshold_db), float(pad_ms), float(max_pause_ms))


class TrimInfo(C.Structure):   # ptts_trim_info: what a trim made of one row
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64), ("n_out", C.c_int64), ("cuts", C.c_int64), ("speech", C.c_int32), ("reserved", C.c_int32)]

    def astuple(self):
        return (int(self.lo), int(self.hi), int(self.n_out), int(self.cuts), int(self.speech))


class TempoOpts(C.Structure):   # ptts_tempo_opts
    """The speaking rate of a joined call's parts (ptts_tempo_opts): speed_permille 500 .. 2000 (1000: unchanged, 1250: a quarter faster and a
    fifth shorter), the pitch kept.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("speed_permille", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, speed_permille: int = 1000, size: Optional[int] = None, reserved=(0, 0)):
        super().__init__(C.sizeof(TempoOpts) if size is None else int(size), int(speed_permille), (C.c_int32 * 2)(*[int(v) for v in reserved]))


class FormantOpts(C.Structure):   # ptts_formant_opts
    """Keep the formants around the pitch of a joined call's parts (ptts_formant_opts): keep 1 holds the spectral envelope where it was while the
    pitch moves (served for a pitch from 800 to 1500), keep 0 lets it move with the pitch.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("keep", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, keep: int = 1, size: Optional[int] = None, reserved=(0, 0)):
        super().__init__(C.sizeof(FormantOpts) if size is None else int(size), int(keep), (C.c_int32 * 2)(*[int(v) for v in reserved]))


class PitchOpts(C.Structure):   # ptts_pitch_opts
    """The pitch of a joined call's parts (ptts_pitch_opts): pitch_permille 500 .. 2000 (1000: unchanged, 1100: 10 % higher, 2000: an octave up) at
    the same duration; formants move with it.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("pitch_permille", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, pitch_permille: int = 1000, size: Optional[int] = None, reserved=(0, 0)):
        super().__init__(C.sizeof(PitchOpts) if size is None else int(size), int(pitch_permille), (C.c_int32 * 2)(*[int(v) for v in reserved]))


class JoinOpts(C.Structure):   # ptts_join_opts
    """How a text's parts become one utterance (ptts_join_opts): gap_ms of silence between consecutive parts or crossfade_ms of overlap (each
    0 .. 2000, not both), and -- for Model.generate_joined -- the chain (dsp: a DspOpts; loudness in 0.01 LUFS), run once over the joined audio,
    and its egress (pcm_format, sample_rate).  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("pcm_format", C.c_int32), ("sample_rate", C.c_int32), ("loudness", C.c_int32), ("dsp", C.POINTER(DspOpts)),
                ("gap_ms", C.c_double), ("crossfade_ms", C.c_double)]

    def __init__(self, gap_ms: float = 0.0, crossfade_ms: float = 0.0, pcm_format: int = 0, sample_rate: int = 0, loudness: int = 0,
                 dsp: Optional[DspOpts] = None, size: Optional[int] = None):
        super().__init__(C.sizeof(JoinOpts) if size is None else int(size), int(pcm_format), int(sample_rate), int(loudness),
                         C.pointer(dsp) if dsp is not None else None, float(gap_ms), float(crossfade_ms))
        self._dsp = dsp   # (borrowed by the struct: kept alive with it)


class JoinStreamOpts(C.Structure):   # ptts_join_stream_opts
    """How a joined call hands its audio over (ptts_join_stream_opts): first_group parts in the first group (0: max_batch) and the callback of the
    hand-overs, a _PCM_CB or None.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("first_group", C.c_int32), ("pcm_callback", _PCM_CB), ("pcm_user", C.c_void_p)]

    def __init__(self, first_group: int = 0, pcm_callback=None, size: Optional[int] = None):
        super().__init__(C.sizeof(JoinStreamOpts) if size is None else int(size), int(first_group))
        if pcm_callback is not None:
            self.pcm_callback = pcm_callback
        self._cb = pcm_callback   # (borrowed by the struct: kept alive with it)


class PartOpts(C.Structure):   # ptts_part_opts
    """One part's prosody in a joined call (ptts_part_opts): its trim, pitch, formant option and tempo (a TrimOpts, PitchOpts, FormantOpts, TempoOpts;
    None: none), its volume -- gain_db -60 .. +24 (0: none) or level, a loudness target in 0.01 LUFS (0: off), not both -- and the seam BEHIND it:
    gap_ms / crossfade_ms, both negative (the default) for the pair of the JoinOpts.  size: sizeof as the caller compiled it (None: this mirror's)."""
    _fields_ = [("size", C.c_uint32), ("level", C.c_int32), ("trim", C.POINTER(TrimOpts)), ("pitch", C.POINTER(PitchOpts)), ("formant", C.POINTER(FormantOpts)),
                ("tempo", C.POINTER(TempoOpts)), ("gain_db", C.c_double), ("gap_ms", C.c_double), ("crossfade_ms", C.c_double)]

    def __init__(self, gain_db: float = 0.0, level: int = 0, gap_ms: float = -1.0, crossfade_ms: float = -1.0, trim: Optional[TrimOpts] = None,
                 pitch: Optional[PitchOpts] = None, formant: Optional[FormantOpts] = None, tempo: Optional[TempoOpts] = None, size: Optional[int] = None):
        ptr = lambda v: C.pointer(v) if v is not None else None  # noqa: E731
        super().__init__(C.sizeof(PartOpts) if size is None else int(size), int(level), ptr(trim), ptr(pitch), ptr(formant), ptr(tempo), float(gain_db),
                         float(gap_ms), float(crossfade_ms))
        self._borrowed = (trim, pitch, formant, tempo)   # (borrowed by the struct: kept alive with it)


def _part_list(parts_opts):
    """A sequence of PartOpts as the contiguous list the C entry points take (the elements' borrowed structs stay alive with the sequence)."""
    arr = (PartOpts * max(len(parts_opts), 1))()
    for i, p in enumerate(parts_opts):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(PartOpts))
    return arr


class JoinPart(C.Structure):   # ptts_join_part: one chunk of a joined call, offset and n_samples at 24 kHz in the joined audio
    _fields_ = [("offset", C.c_int64), ("n_samples", C.c_int64), ("n_frames", C.c_int32), ("eos_step", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]


class EqSection(C.Structure):   # ptts_eq_section
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("freq_hz", C.c_double), ("gain_db", C.c_double), ("q", C.c_double)]


EQ_LOWPASS, EQ_HIGHPASS, EQ_LOWSHELF, EQ_HIGHSHELF, EQ_PEAKING = 1, 2, 3, 4, 5   # ptts_eq_section.type


class _Request(C.Structure):
    _fields_ = [("tokens", _IP), ("n_tokens", C.c_int64), ("temperature", C.c_float), ("eos_threshold", C.c_float),
                ("max_steps", C.c_int32), ("estimated_max_steps", C.c_int32), ("lsd_steps", C.c_int32),
                ("frames_after_eos", C.c_int32), ("voice_embedding", _FP), ("voice_frames", C.c_int64),
                ("voice_caches", C.POINTER(_FP)), ("voice_cache_steps", _IP), ("voice_offsets", _IP), ("noise", _FP),
                ("step_callback", _STEP_CB), ("callback_user", C.c_void_p), ("cancel", C.POINTER(C.c_int32)),
                ("want_latents", C.c_int32), ("pcm_format", C.c_int32), ("voice", C.c_void_p), ("noise_seed", C.c_uint64), ("noise_rows", C.c_int32), ("loudness", C.c_int32),
                ("pcm_callback", _PCM_CB), ("pcm_user", C.c_void_p), ("stream_frames", C.c_int32), ("sample_rate", C.c_int32), ("dsp", C.POINTER(DspOpts))]


class _Profile(C.Structure):
    _fields_ = [("launches", C.c_int64), ("total_ms", C.c_double), ("algorithmic_bytes", C.c_double), ("kernel", C.c_char * 64),
                ("weight_bytes", C.c_double), ("prefill_ms", C.c_double), ("ar_loop_ms", C.c_double), ("mimi_ms", C.c_double)]


class _Result(C.Structure):
    _fields_ = [("pcm", _FP), ("n_samples", C.c_int64), ("latents", _FP), ("n_frames", C.c_int32), ("eos_step", C.c_int32),
                ("status", C.c_int32), ("pcm16", C.POINTER(C.c_int16)), ("pcm8", C.POINTER(C.c_uint8))]


# the same layout as a numpy record (generate_batch reads a whole batch of results as one table)
_RESULT_DTYPE = np.dtype({"names": ["pcm", "n_samples", "latents", "n_frames", "eos_step", "status", "pcm16", "pcm8"],
                          "formats": ["<u8", "<i8", "<u8", "<i4", "<i4", "<i4", "<u8", "<u8"],
                          "offsets": [_Result.pcm.offset, _Result.n_samples.offset, _Result.latents.offset, _Result.n_frames.offset,
                                      _Result.eos_step.offset, _Result.status.offset, _Result.pcm16.offset, _Result.pcm8.offset],
                          "itemsize": C.sizeof(_Result)})

class _VoiceTensor(C.Structure):   # ptts_voice_tensor
    _fields_ = [("data", C.POINTER(C.c_float)), ("count", C.c_int64), ("rank", C.c_int32), ("reserved", C.c_int32), ("shape", C.c_int64 * 8)]


_lib = None

# every symbol include/ptts.h declares (tests check that the built library exports all of them -- and none of HOOK_SYMBOLS)
ABI_SYMBOLS = [
    "ptts_default_opts", "ptts_model_open", "ptts_model_open_bytes", "ptts_model_close", "ptts_model_info", "ptts_last_error",
    "ptts_plan_create", "ptts_plan_create_bytes", "ptts_plan_arena_bytes", "ptts_model_open_planned", "ptts_plan_free",
    "ptts_generate", "ptts_free_result", "ptts_text_embeddings", "ptts_batch_new", "ptts_batch_free", "ptts_batch_reset",
    "ptts_batch_set_voice_state", "ptts_batch_prompt", "ptts_batch_step", "ptts_batch_offsets", "ptts_batch_read_kv",
    "ptts_decode_latents", "ptts_noise_rows", "ptts_speaker_project", "ptts_mimi_encode", "ptts_mimi_encode_frames", "ptts_voice_encode_audio", "ptts_flow_direction", "ptts_op_linear", "ptts_op_layernorm", "ptts_op_rope",
    "ptts_op_attention_positions", "ptts_op_conv1d_leftpad", "ptts_op_convtr1d_righttrim", "ptts_version",
        "ptts_voice_create", "ptts_voice_free", "ptts_profile_enable", "ptts_profile_read", "ptts_plan_fill_host", "ptts_wav_header_streaming", "ptts_op_pcm16",
    "ptts_dispatcher_create", "ptts_dispatcher_create_custom", "ptts_dispatch_generate", "ptts_dispatcher_stats", "ptts_dispatcher_close",
    "ptts_model_share", "ptts_model_replicate", "ptts_model_set_use_graph", "ptts_model_set_max_batch", "ptts_text_estimate_max_frames", "ptts_text_frames_after_eos", "ptts_text_prepare", "ptts_text_chunks", "ptts_chunks_count",
    "ptts_chunks_get", "ptts_chunks_free",
    "ptts_tokenizer_open", "ptts_tokenizer_open_bytes", "ptts_tokenizer_free", "ptts_tokenizer_vocab_size", "ptts_tokenizer_encode",
    "ptts_tokenizer_encode_cb", "ptts_text_nfkc", "ptts_rccl_unique_id", "ptts_rccl_broadcast", "ptts_dsp_apply",
    "ptts_voice_file_open", "ptts_voice_file_open_bytes", "ptts_voice_file_close", "ptts_voice_file_kind", "ptts_voice_file_embedding",
    "ptts_voice_file_modules", "ptts_voice_file_module", "ptts_voice_file_state", "ptts_voice_open", "ptts_voice_open_bytes",
    "ptts_voice_from_embeddings", "ptts_voice_from_audio", "ptts_voice_offset", "ptts_voice_read_state", "ptts_voice_write", "ptts_voice_write_bytes",
    "ptts_voice_state_write_bytes", "ptts_voice_embedding_write", "ptts_free_bytes",
    "ptts_resample_length", "ptts_resample", "ptts_pcm_encode", "ptts_mimi_encode_rates", "ptts_voice_from_audio_rates", "ptts_wav_header",
    "ptts_dsp_rows", "ptts_loudness", "ptts_loudness_normalize", "ptts_loudness_rows", "ptts_loudness_normalize_rows",
    "ptts_eq_design", "ptts_eq_response", "ptts_eq_create", "ptts_eq_free", "ptts_eq_apply", "ptts_eq_rows",
    "ptts_dsp_ext_create", "ptts_dsp_ext_free", "ptts_true_peak", "ptts_true_peak_limit", "ptts_true_peak_rows",
    "ptts_dsp_ext_set_compressor", "ptts_compress_gain", "ptts_compress_apply", "ptts_compress_rows",
    "ptts_dsp_ext_set_limiter", "ptts_limit_apply", "ptts_limit_rows",
    "ptts_dsp_ext_set_deesser", "ptts_deess_apply", "ptts_deess_band", "ptts_deess_rows",
    "ptts_join_length", "ptts_join", "ptts_join_rows", "ptts_generate_joined", "ptts_generate_joined_streamed", "ptts_join_stream_ready",
    "ptts_join_parts_length", "ptts_join_parts", "ptts_join_parts_rows", "ptts_join_parts_stream_ready", "ptts_generate_joined_parts",
    "ptts_trim_plan", "ptts_trim_apply", "ptts_trim_rows", "ptts_dsp_ext_set_trim",
    "ptts_tempo_length", "ptts_tempo_plan", "ptts_tempo_apply", "ptts_tempo_rows", "ptts_dsp_ext_set_tempo",
    "ptts_pitch_speed", "ptts_pitch_resample_length", "ptts_pitch_resample", "ptts_pitch_length", "ptts_pitch_apply", "ptts_pitch_table",
    "ptts_pitch_rows", "ptts_dsp_ext_set_pitch",
    "ptts_formant_frames", "ptts_formant_analyse", "ptts_formant_whiten", "ptts_formant_shape", "ptts_formant_apply", "ptts_formant_rows",
    "ptts_dsp_ext_set_formant",
    ]
# the test / measurement hooks of include/ptts_debug.h: exported by libptts_hooks.so, never by libptts_hip.so (checked by __graft_entry__.build())
HOOK_SYMBOLS = [
    "ptts_decode_stages", "ptts_mimi_layer_piece", "ptts_debug_last_attention_kernel", "ptts_debug_launch_counts", "ptts_debug_flow_cluster_inject",
    "ptts_debug_time_skinny", "ptts_debug_skinny_stamps", "ptts_debug_gemm", "ptts_debug_step_stamps", "ptts_debug_tall",
    "ptts_debug_encode_stages", "ptts_debug_resample_launches", "ptts_debug_dsp_blocked_host",
    "ptts_debug_loudness_energies", "ptts_debug_kweighting", "ptts_debug_step_linear", "ptts_debug_true_peak_taps", "ptts_debug_true_peak_oversample",
    "ptts_debug_dsp_opts_error", "ptts_debug_resblock", "ptts_debug_resblock_plan", "ptts_debug_seanet_pack", "ptts_debug_plan_seanet_frags",
    "ptts_debug_gemm_rows", "ptts_debug_attn_step", "ptts_debug_attn_step_rounds", "ptts_debug_attn_window", "ptts_debug_flow_cluster",
    "ptts_debug_mimi_fused", "ptts_debug_mimi_pack", "ptts_debug_dsp_windows", "ptts_debug_step_edge",
]


def build(force: bool = False) -> str:
    """Compiles the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", _HERE, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PttsError(PTTS_ENODEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; two HSA runtimes in one process leave the
        # second without a GPU.  Importing torch first makes the dynamic linker resolve our DT_NEEDED libamdhip64.so.7
        # to the copy torch already loaded, so tests / bench.py (torch.distributed plumbing) and this library share one
        # runtime.  Hosts that never load torch (the Go service) set PTTS_NO_TORCH_PRELOAD=1 or simply lack torch.
        if "torch" not in sys.modules and not os.environ.get("PTTS_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:  # noqa: BLE001
                pass
        L = C.CDLL(LIB_PATH)
        L.ptts_last_error.restype = C.c_char_p
        L.ptts_version.restype = C.c_char_p
        L.ptts_plan_arena_bytes.restype = C.c_size_t
        L.ptts_plan_arena_bytes.argtypes = [C.c_void_p]
        L.ptts_plan_free.argtypes = [C.c_void_p]
        L.ptts_model_close.argtypes = [C.c_void_p]
        L.ptts_batch_free.argtypes = [C.c_void_p]
        L.ptts_model_open.argtypes = [C.c_char_p, C.POINTER(_Opts), C.POINTER(C.c_void_p)]
        L.ptts_model_open_bytes.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_Opts), C.POINTER(C.c_void_p)]
        L.ptts_plan_create.argtypes = [C.c_char_p, C.POINTER(_Opts), C.POINTER(C.c_void_p)]
        L.ptts_plan_create_bytes.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_Opts), C.POINTER(C.c_void_p)]
        L.ptts_model_open_planned.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.ptts_plan_fill_host.argtypes = [C.c_void_p, C.c_void_p]
        L.ptts_model_info.argtypes = [C.c_void_p, C.POINTER(_Info)]
        L.ptts_generate.argtypes = [C.c_void_p, C.POINTER(_Request), C.c_int32, C.POINTER(_Result)]
        L.ptts_free_result.argtypes = [C.POINTER(_Result)]
        L.ptts_text_embeddings.argtypes = [C.c_void_p, _IP, C.c_int64, _FP]
        L.ptts_batch_new.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.ptts_batch_reset.argtypes = [C.c_void_p]
        L.ptts_batch_set_voice_state.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_FP), _IP, _IP]
        L.ptts_batch_prompt.argtypes = [C.c_void_p, _FP, _IP]
        L.ptts_batch_step.argtypes = [C.c_void_p, _FP, C.c_int32, _FP, _FP, _FP, _FP]
        L.ptts_batch_offsets.argtypes = [C.c_void_p, _IP]
        L.ptts_batch_read_kv.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _FP, _FP]
        L.ptts_decode_latents.argtypes = [C.c_void_p, _FP, C.c_int32, C.c_int32, _FP, _FP]
        L.ptts_noise_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_int32, _FP]
        L.ptts_flow_direction.argtypes = [C.c_void_p, _FP, C.c_float, C.c_float, _FP, C.c_int32, _FP]
        L.ptts_voice_create.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, _IP, C.POINTER(C.c_void_p)]
        L.ptts_voice_free.argtypes = [C.c_void_p]
        L.ptts_voice_file_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.ptts_voice_file_open_bytes.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.ptts_voice_file_close.argtypes = [C.c_void_p]
        L.ptts_voice_file_close.restype = None
        L.ptts_voice_file_kind.argtypes = [C.c_void_p]
        L.ptts_voice_file_kind.restype = C.c_int32
        L.ptts_voice_file_embedding.argtypes = [C.c_void_p, C.POINTER(_FP), _IP]
        L.ptts_voice_file_modules.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.ptts_voice_file_module.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(_VoiceTensor), C.POINTER(_VoiceTensor)]
        L.ptts_voice_file_state.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_FP), _IP, _IP]
        L.ptts_voice_open.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.ptts_voice_open_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.ptts_voice_from_embeddings.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        L.ptts_voice_from_audio.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(C.c_void_p)]
        L.ptts_voice_offset.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.ptts_voice_read_state.argtypes = [C.c_void_p, C.c_int32, _FP]
        L.ptts_voice_write.argtypes = [C.c_void_p, C.c_char_p]
        L.ptts_voice_write_bytes.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        L.ptts_voice_state_write_bytes.argtypes = [C.POINTER(_FP), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.POINTER(C.c_uint8)),
                                                   C.POINTER(C.c_size_t)]
        L.ptts_voice_embedding_write.argtypes = [_FP, C.c_int64, C.c_int64, C.c_char_p]
        L.ptts_free_bytes.argtypes = [C.POINTER(C.c_uint8)]
        L.ptts_free_bytes.restype = None
        L.ptts_profile_enable.argtypes = [C.c_void_p, C.c_int32]
        L.ptts_profile_read.argtypes = [C.c_void_p, C.POINTER(_Profile)]
        L.ptts_op_linear.argtypes = [_FP, _FP, _FP, C.c_int64, C.c_int64, C.c_int64, _FP]
        L.ptts_op_layernorm.argtypes = [_FP, _FP, _FP, C.c_float, C.c_int64, C.c_int64, _FP]
        L.ptts_op_rope.argtypes = [_FP, _FP, _FP] + [C.c_int64] * 5
        L.ptts_op_attention_positions.argtypes = [_FP, _FP, _FP] + [C.c_int64] * 5 + [_IP, _IP, C.c_int64, _FP]
        L.ptts_op_conv1d_leftpad.argtypes = [_FP, _FP, _FP] + [C.c_int64] * 5 + [_FP]
        L.ptts_op_convtr1d_righttrim.argtypes = [_FP, _FP, _FP] + [C.c_int64] * 7 + [_FP]
        L.ptts_resample_length.restype = C.c_int64
        L.ptts_resample_length.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.ptts_resample.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_FP)]
        L.ptts_pcm_encode.argtypes = [C.c_void_p, _FP, C.c_int64, C.c_int32, C.c_void_p]
        L.ptts_dsp_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(DspOpts), C.POINTER(_FP)]
        L.ptts_eq_rows.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP)]
        L.ptts_true_peak_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, _FP]
        L.ptts_dsp_ext_set_compressor.argtypes = [C.c_void_p, C.POINTER(CompressorOpts)]
        L.ptts_compress_gain.argtypes = [C.POINTER(CompressorOpts), C.c_double, _DP]
        L.ptts_compress_apply.argtypes = [C.POINTER(CompressorOpts), _FP, C.c_int64]
        L.ptts_compress_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(CompressorOpts)), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP)]
        L.ptts_dsp_ext_set_limiter.argtypes = [C.c_void_p, C.POINTER(LimiterOpts)]
        L.ptts_limit_apply.argtypes = [C.POINTER(LimiterOpts), _FP, C.c_int64]
        L.ptts_limit_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(LimiterOpts)), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP)]
        L.ptts_dsp_ext_set_deesser.argtypes = [C.c_void_p, C.POINTER(DeesserOpts)]
        L.ptts_deess_apply.argtypes = [C.POINTER(DeesserOpts), _FP, C.c_int64]
        L.ptts_deess_band.argtypes = [C.POINTER(DeesserOpts), _FP, C.c_int64, _FP]
        L.ptts_deess_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DeesserOpts)), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP)]
        L.ptts_join_length.restype = C.c_int64
        L.ptts_join_length.argtypes = [_IP, C.c_int32, C.POINTER(JoinOpts), _IP]
        L.ptts_join.argtypes = [C.POINTER(_FP), _IP, C.c_int32, C.POINTER(JoinOpts), _FP]
        L.ptts_join_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(JoinOpts), _FP]
        L.ptts_generate_joined.argtypes = [C.c_void_p, C.POINTER(_Request), C.c_int32, C.POINTER(JoinOpts), C.POINTER(_Result), C.POINTER(JoinPart)]
        L.ptts_generate_joined_streamed.argtypes = [C.c_void_p, C.POINTER(_Request), C.c_int32, C.POINTER(JoinOpts), C.POINTER(JoinStreamOpts), C.POINTER(_Result),
                                                    C.POINTER(JoinPart)]
        L.ptts_join_stream_ready.restype = C.c_int64
        L.ptts_join_stream_ready.argtypes = [C.POINTER(JoinOpts), C.c_int64]
        L.ptts_join_parts_length.restype = C.c_int64
        L.ptts_join_parts_length.argtypes = [_IP, C.c_int32, C.POINTER(JoinOpts), C.POINTER(PartOpts), _IP]
        L.ptts_join_parts.argtypes = [C.POINTER(_FP), _IP, C.c_int32, C.POINTER(JoinOpts), C.POINTER(PartOpts), _FP, _FP]
        L.ptts_join_parts_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(JoinOpts), C.POINTER(PartOpts), _FP, _FP]
        L.ptts_join_parts_stream_ready.restype = C.c_int64
        L.ptts_join_parts_stream_ready.argtypes = [C.POINTER(JoinOpts), C.POINTER(PartOpts), C.c_int64]
        L.ptts_generate_joined_parts.argtypes = [C.c_void_p, C.POINTER(_Request), C.c_int32, C.POINTER(JoinOpts), C.POINTER(PartOpts), C.POINTER(JoinStreamOpts),
                                                 C.POINTER(_Result), C.POINTER(JoinPart), _FP]
        L.ptts_trim_plan.argtypes = [C.POINTER(TrimOpts), _FP, C.c_int64, C.POINTER(TrimInfo)]
        L.ptts_trim_apply.argtypes = [C.POINTER(TrimOpts), _FP, C.c_int64, _FP, C.POINTER(TrimInfo)]
        L.ptts_trim_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(TrimOpts)), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP), C.POINTER(TrimInfo)]
        L.ptts_dsp_ext_set_trim.argtypes = [C.c_void_p, C.POINTER(TrimOpts)]
        L.ptts_tempo_length.argtypes = [C.POINTER(TempoOpts), C.c_int64]
        L.ptts_tempo_length.restype = C.c_int64
        L.ptts_tempo_plan.argtypes = [C.POINTER(TempoOpts), _FP, C.c_int64, C.POINTER(C.c_int32)]
        L.ptts_tempo_apply.argtypes = [C.POINTER(TempoOpts), _FP, C.c_int64, _FP]
        L.ptts_tempo_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(TempoOpts)), C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP), _IP]
        L.ptts_dsp_ext_set_tempo.argtypes = [C.c_void_p, C.POINTER(TempoOpts)]
        L.ptts_pitch_speed.argtypes = [C.POINTER(PitchOpts), C.POINTER(TempoOpts)]
        L.ptts_pitch_speed.restype = C.c_int32
        L.ptts_pitch_resample_length.argtypes = [C.POINTER(PitchOpts), C.c_int64]
        L.ptts_pitch_resample_length.restype = C.c_int64
        L.ptts_pitch_resample.argtypes = [C.POINTER(PitchOpts), _FP, C.c_int64, _FP]
        L.ptts_pitch_length.argtypes = [C.POINTER(PitchOpts), C.POINTER(TempoOpts), C.c_int64]
        L.ptts_pitch_length.restype = C.c_int64
        L.ptts_pitch_apply.argtypes = [C.POINTER(PitchOpts), C.POINTER(TempoOpts), _FP, C.c_int64, _FP]
        L.ptts_pitch_table.argtypes = [C.POINTER(_FP), C.POINTER(_FP), C.POINTER(C.c_int32)]
        L.ptts_pitch_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(PitchOpts)), C.POINTER(C.POINTER(TempoOpts)), C.POINTER(_FP), _IP, C.c_int32,
                                      C.POINTER(_FP), _IP]
        L.ptts_dsp_ext_set_pitch.argtypes = [C.c_void_p, C.POINTER(PitchOpts)]
        L.ptts_formant_frames.argtypes = [C.c_int64]
        L.ptts_formant_frames.restype = C.c_int32
        L.ptts_formant_analyse.argtypes = [_FP, C.c_int64, _FP]
        L.ptts_formant_whiten.argtypes = [_FP, _FP, C.c_int64, _FP]
        L.ptts_formant_shape.argtypes = [_FP, C.c_int64, C.c_int32, _FP, C.c_int64, _FP]
        L.ptts_formant_apply.argtypes = [C.POINTER(FormantOpts), C.POINTER(PitchOpts), C.POINTER(TempoOpts), _FP, C.c_int64, _FP]
        L.ptts_formant_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(FormantOpts)), C.POINTER(C.POINTER(PitchOpts)), C.POINTER(C.POINTER(TempoOpts)),
                                        C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_FP), _IP]
        L.ptts_dsp_ext_set_formant.argtypes = [C.c_void_p, C.POINTER(FormantOpts)]
        L.ptts_loudness_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, _DP]
        L.ptts_loudness_normalize_rows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.c_double, C.POINTER(_FP), _DP]
        L.ptts_mimi_encode_rates.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.POINTER(C.c_int32), C.c_int32, C.POINTER(_FP)]
        L.ptts_voice_from_audio_rates.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
        L.ptts_wav_header.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
        _lib = L
    return _lib


HOOKS_PATH = os.path.join(_HERE, "libptts_hooks.so")   # (also beside another build of the product library named by PTTS_LIB_PATH: it binds to the libptts_hip.so SONAME already loaded)
_hooks = None


def hooks():
    """libptts_hooks.so: the entry points of include/ptts_debug.h (launch census, staged decoder observation points, in-kernel stamps, micro-benchmarks,
    fault injection).  Loaded beside the product library by tests and tools only; it resolves its internals against the libptts_hip.so already mapped."""
    global _hooks
    if _hooks is None:
        lib()   # the product library first: the hooks' DT_NEEDED libptts_hip.so then resolves to the copy already in the process
        if not os.path.exists(HOOKS_PATH):
            raise PttsError(PTTS_ENODEVICE, f"{HOOKS_PATH} is missing: run __graft_entry__.build()")
        H = C.CDLL(HOOKS_PATH, mode=C.RTLD_GLOBAL)
        H.ptts_decode_stages.argtypes = [C.c_void_p, _FP, C.c_int32, C.c_int32, _FP, _FP, _FP]
        H.ptts_debug_last_attention_kernel.restype = C.c_char_p
        H.ptts_debug_launch_counts.restype = C.c_int64
        H.ptts_debug_launch_counts.argtypes = [C.c_int32, C.c_char_p, C.c_int64]
        H.ptts_mimi_layer_piece.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _FP, C.c_int64, C.c_int32, C.c_int32, _FP]
        H.ptts_debug_flow_cluster_inject.argtypes = [C.c_void_p, C.c_int32]
        H.ptts_debug_loudness_energies.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(_DP)]
        H.ptts_debug_dsp_windows.argtypes = [C.c_void_p, C.POINTER(_FP), _IP, C.c_int32, C.POINTER(DspOpts), _IP, C.c_int32, C.POINTER(_FP)]
        H.ptts_debug_dsp_opts_error.restype = C.c_int64
        H.ptts_debug_dsp_opts_error.argtypes = [C.POINTER(DspOpts), C.c_char_p, C.c_int64]
        for name, args in (("flow_cluster", _FlowClusterArgs), ("step_linear", _StepLinearArgs), ("step_edge", _StepEdgeArgs), ("attn_step", _AttnStepArgs), ("attn_window", _AttnWindowArgs),
                           ("gemm_rows", _GemmRowsArgs), ("mimi_fused", _MimiFusedArgs), ("resblock", _ResblockArgs)):   # the hooks on a struct of host operands
            getattr(H, "ptts_debug_" + name).argtypes = [C.POINTER(args)]
        _hooks = H
    return _hooks


def _check(rc: int):
    if rc != PTTS_OK:
        msg = lib().ptts_last_error().decode(errors="replace")
        raise (Cancelled if rc == PTTS_ECANCELLED else PttsError)(rc, msg)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _row_ptrs(arrays, ptr=_FP):
    """The pointer array over a list of arrays (never of length 0: an empty list gives one NULL entry)."""
    return (ptr * max(len(arrays), 1))(*[C.cast(a.ctypes.data, ptr) for a in arrays])


def _rows_in(x):
    """An array, or a list of arrays, as mono f32 rows for a rows entry point: (single, rows, n, their pointer array, their lengths as int64)."""
    single = not isinstance(x, (list, tuple))
    rows = [_f32(x).reshape(-1)] if single else [_f32(r).reshape(-1) for r in x]
    return single, rows, len(rows), _row_ptrs(rows), np.array([r.size for r in rows] or [0], np.int64)


def _tempo_size(r, t):
    """The floats of row r's output at the tempo t (None: a copy), with the speed clamped into the range the library takes."""
    return r.size if t is None else r.size * 1000 // min(max(int(t.speed_permille), 500), 2000)


def _fp(a: Optional[np.ndarray]):
    return C.cast(a.ctypes.data, _FP) if a is not None else None   # (ndarray.ctypes.data_as is three times slower; 64 requests per call)


def _ip(a: np.ndarray):
    return C.cast(a.ctypes.data, _IP)


class _Keep:
    """Pointers for the fields of a ctypes struct: None gives a null pointer, anything else is made a contiguous array that stays referenced as long as
    this object does (the struct itself holds addresses only)."""

    def __init__(self):
        self.arrays = []

    def _ptr(self, a, dtype, ptr):
        if a is None:
            return C.cast(None, ptr)
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        self.arrays.append(a)
        return C.cast(a.ctypes.data, ptr)

    def f32(self, a):
        return self._ptr(a, np.float32, _FP)

    def i32(self, a):
        return self._ptr(a, np.int32, _I32P)

    def u16(self, a):
        return self._ptr(a, np.uint16, _U16P)


def _census_dict(buf) -> dict:
    """{kernel: count} of a census string "k=v;k=v;" in a ctypes buffer."""
    return {k: int(v) for k, v in (item.split("=") for item in buf.value.decode().split(";") if item)}


# ----------------------------------------------------------------------------- reference-shaped types

@dataclass
class VoiceEmbedding:
    """tts.VoiceEmbedding (runtime.go:11-14): shape [1, T, D]."""
    data: np.ndarray
    shape: Sequence[int]

    def save(self, path: str) -> None:
        """A legacy-embedding voice file: `audio_prompt` F32 [1, T, D] (ptts_voice_embedding_write)."""
        d = _f32(self.data).reshape(-1, int(self.shape[-1]))
        _check(lib().ptts_voice_embedding_write(_fp(d), d.shape[0], d.shape[1], os.fsencode(path)))


@dataclass
class VoiceModelState:
    """safetensors.VoiceModelState (reader.go:29-31): modules[name]["cache" | "offset"]."""
    modules: dict


@dataclass
class RuntimeGenerateConfig:
    """tts.RuntimeGenerateConfig (runtime.go:17-31).  `noise` is this build's explicit form of the
    reference's rng draws (flow_lm.go:386-408): [max_steps, 32] rows of N(0,1)*sqrt(temperature)."""
    temperature: float = 0.0
    eos_threshold: float = -4.0
    max_steps: int = 0
    estimated_max_steps: int = 0
    lsd_decode_steps: int = 1
    frames_after_eos: int = 0
    mimi_steps_per_latent: int = 0   # accepted and ignored, like the native reference runtime
    mimi_sequence_length: int = 0
    voice_embedding: Optional[VoiceEmbedding] = None
    voice_model_state: Optional[VoiceModelState] = None
    device_voice: Optional["DeviceVoice"] = None   # a VoiceModelState already uploaded with Model.upload_voice
    step_callback: Optional[Callable[[int, int], None]] = None
    noise: Optional[np.ndarray] = None
    noise_seed: int = 0   # device draw (temperature > 0, no injected noise): 0 = a fresh stream per request, like the reference's clock-seeded rng
    cancel: Optional[np.ndarray] = None  # int32[1]; nonzero = cancelled (the ctx of GenerateAudio)
    want_latents: bool = False
    pcm16: bool = False   # PCM egress on the device: GenerateResult.pcm is int16 = audio.WritePCM16Samples (wav_stream.go:43-54)
    g711: str = ""        # "ulaw" / "alaw": GenerateResult.pcm is uint8 G.711 of that int16, encoded on the device (takes precedence over pcm16)
    sample_rate: int = 0  # output rate in Hz (0: 24000); other rates are resampled on the device (k_resample)
    # frame-granular streaming: pcm_callback(sample_offset, samples) is called from a library thread for consecutive ranges of
    # `stream_frames` frames while generation is still running (samples: a copy, float32, int16 or uint8 per the format; offsets count samples at sample_rate)
    pcm_callback: Optional[Callable[[int, np.ndarray], None]] = None
    stream_frames: int = 0
    # post-processing on the device (ptts_request.dsp): dsp_apply's chain on this request's own 24 kHz audio, in front of the egress above
    normalize: bool = False
    dc_block: bool = False
    fade_in_ms: float = 0.0
    fade_out_ms: float = 0.0
    dsp_opts: Optional[DspOpts] = None   # a ptts_dsp_opts handed over as it is (takes precedence; an all-off struct is a valid request)
    # loudness normalisation on the device (ptts_request.loudness): 0 off, else the BS.1770 target in 0.01 LUFS (-2300: EBU R 128, -1600: streaming);
    # the result is loudness_normalize(this request's own 24 kHz audio, loudness / 100), then the switches above, then the egress
    loudness: int = 0
    # a per-request equaliser (ptts_dsp_opts.eq): an Eq, applied behind the DC block and in front of the fades; the caller keeps it alive
    eq: Optional["Eq"] = None
    # a true-peak ceiling in dBTP (ptts_dsp_opts.ext; -60 .. 0, None: off): the last stage of the chain, true_peak_limit of what the stages above
    # made of this request's 24 kHz audio -- a static gain where the utterance's true peak exceeds the ceiling, not a limiter
    true_peak_dbtp: Optional[float] = None
    # a dynamic range compressor (ptts_dsp_opts.ext, ptts_dsp_ext_set_compressor; None: off): the FIRST stage of the chain, compress_apply of this
    # request's own raw 24 kHz audio; loudness and normalise are measured behind it
    compressor: Optional[CompressorOpts] = None
    # a look-ahead peak limiter (ptts_dsp_opts.ext, ptts_dsp_ext_set_limiter; None: off): behind the fades and in front of the true-peak ceiling,
    # limit_apply of what the stages above made of this request's 24 kHz audio
    limiter: Optional[LimiterOpts] = None
    # a de-esser (ptts_dsp_opts.ext, ptts_dsp_ext_set_deesser; None: off): directly behind the compressor and in front of everything else,
    # deess_apply of what the compressor made of this request's 24 kHz audio
    deesser: Optional[DeesserOpts] = None


def _free_addr(addr: int):
    """Hand one result buffer back to the library's page-locked pool."""
    r = _Result()
    r.pcm = C.cast(C.c_void_p(addr), _FP)
    lib().ptts_free_result(C.byref(r))


class _OwnedBuffer:
    """A result buffer handed over by the library: exposes it to numpy without a copy and frees it on collection."""

    def __init__(self, ptr, n: int, typestr: str):
        self._addr = ptr if type(ptr) is int else C.cast(ptr, C.c_void_p).value
        self.__array_interface__ = {"shape": (n,), "typestr": typestr, "data": (self._addr, False), "version": 3}

    def __del__(self):
        if self._addr and sys is not None and not sys.is_finalizing():
            _free_addr(self._addr)
            self._addr = None


@dataclass
class GenerateResult:
    pcm: np.ndarray
    n_frames: int
    eos_step: int
    latents: Optional[np.ndarray] = None


@dataclass
class JoinedResult:
    """One joined call's result: the whole text's audio in the join options' egress format; n_frames summed over the chunks; parts: a JoinPart per
    chunk (offset and n_samples at 24 kHz in the joined audio, in front of the egress; n_frames; eos_step; status); gains: a call with a list of
    PartOpts: the f32 gain applied to every part (None otherwise)."""
    pcm: np.ndarray
    n_frames: int
    parts: list
    gains: Optional[np.ndarray] = None


@dataclass
class ModelInfo:
    d_model: int; n_heads: int; n_layers: int; ffn: int; ldim: int; n_bins: int
    flow_dim: int; flow_depth: int; mimi_dim: int; mimi_heads: int; mimi_layers: int; mimi_context: int
    sample_rate: int; samples_per_frame: int; steps_per_latent: int
    frame_rate: float; encoder_frame_rate: float; n_params: int; arena_bytes: int; weights: int; kv: int


def _opts(device=0, weights=WEIGHTS_F32, kv=KV_F32, max_batch=64, use_graph=False) -> _Opts:
    o = _Opts()
    lib().ptts_default_opts(C.byref(o))
    o.device, o.weights, o.kv, o.max_batch, o.use_graph = device, weights, kv, max_batch, 1 if use_graph else 0
    return o


class Model:
    """native.Model (internal/native/model.go:25-138) resident in HBM."""

    def __init__(self, handle: int):
        self.h = handle
        i = _Info()
        _check(lib().ptts_model_info(self.h, C.byref(i)))
        self.info = ModelInfo(**{n: getattr(i, n) for n, _ in _Info._fields_})

    @staticmethod
    def open(path: str, **kw) -> "Model":
        """LoadModelFromSafetensors (model.go:33-40)."""
        h = C.c_void_p()
        o = _opts(**kw)
        _check(lib().ptts_model_open(path.encode(), C.byref(o), C.byref(h)))
        return Model(h.value)

    @staticmethod
    def open_bytes(data: bytes, **kw) -> "Model":
        """LoadModelFromStore over OpenStoreFromBytes (store.go:65)."""
        h = C.c_void_p()
        o = _opts(**kw)
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        _check(lib().ptts_model_open_bytes(buf, len(data), C.byref(o), C.byref(h)))
        return Model(h.value)

    @staticmethod
    def plan(path: str, **kw) -> tuple[int, int]:
        """Returns (plan handle, arena bytes) for the two-phase multi-GPU open."""
        p = C.c_void_p()
        o = _opts(**kw)
        _check(lib().ptts_plan_create(path.encode(), C.byref(o), C.byref(p)))
        return p.value, int(lib().ptts_plan_arena_bytes(p.value))

    @staticmethod
    def plan_fill_host(plan: int, nbytes: int) -> np.ndarray:
        """Host image of the arena (decode + convert + derive), no GPU needed."""
        buf = np.zeros(nbytes, np.uint8)
        _check(lib().ptts_plan_fill_host(plan, buf.ctypes.data_as(C.c_void_p)))
        return buf

    @staticmethod
    def plan_free(plan: int):
        lib().ptts_plan_free(plan)

    @staticmethod
    def open_planned(plan: int, device_arena_ptr: int, fill: bool) -> "Model":
        h = C.c_void_p()
        _check(lib().ptts_model_open_planned(plan, C.c_void_p(device_arena_ptr), 1 if fill else 0, C.byref(h)))
        return Model(h.value)

    def set_use_graph(self, on: bool):
        """ptts_opts.use_graph of an open model: hipGraph replay of the AR step (True) or plain launches (False)."""
        lib().ptts_model_set_use_graph.argtypes = [C.c_void_p, C.c_int32]
        _check(lib().ptts_model_set_use_graph(self.h, 1 if on else 0))

    def set_max_batch(self, n: int):
        """ptts_opts.max_batch of an open model / engine (1..256): utterances of one call that are stepped together."""
        lib().ptts_model_set_max_batch.argtypes = [C.c_void_p, C.c_int32]
        _check(lib().ptts_model_set_max_batch(self.h, int(n)))

    def share(self) -> "Model":
        """A second engine over this model's weights (own streams, KV caches, workspaces); this model must outlive it."""
        h = C.c_void_p()
        lib().ptts_model_share.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _check(lib().ptts_model_share(self.h, C.byref(h)))
        return Model(h.value)

    def replicate(self, device: int) -> "Model":
        """This model on another GPU of the process (own arena, filled from this one's by hipMemcpyPeer); independent of this one afterwards."""
        h = C.c_void_p()
        lib().ptts_model_replicate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        _check(lib().ptts_model_replicate(self.h, int(device), C.byref(h)))
        return Model(h.value)

    def close(self):
        if self.h:
            lib().ptts_model_close(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():   # the HIP runtime may already be gone at interpreter teardown
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # -- staged methods
    def text_embeddings(self, ids) -> np.ndarray:
        ids = np.ascontiguousarray(ids, np.int64)
        out = np.empty((ids.size, self.info.d_model), np.float32)
        _check(lib().ptts_text_embeddings(self.h, _ip(ids), ids.size, _fp(out)))
        return out

    def upload_voice(self, state: VoiceModelState) -> "DeviceVoice":
        """Keeps a voice model state in HBM (the reference re-reads the file per Synthesize call: service.go:127,216-246)."""
        ptrs, steps, offs, arrs = _voice_arrays(state, self.info.n_layers)
        h = C.c_void_p()
        _check(lib().ptts_voice_create(self.h, ptrs, _ip(steps), _ip(offs), C.byref(h)))
        return DeviceVoice(h.value, int(offs[0]), self.info)

    def mimi_layer_qkv(self, layer: int, x, pos0: int = 0, rows_per_seg: int = 0) -> np.ndarray:
        """norm1 -> in_proj -> RoPE(q, k) of Mimi decoder-transformer layer `layer` on rows x [R, 512] -> [R, 1536] (ptts_mimi_layer_piece)."""
        x = _f32(x)
        out = np.empty((x.shape[0], 3 * x.shape[1]), np.float32)
        _check(hooks().ptts_mimi_layer_piece(self.h, layer, 0, _fp(x), x.shape[0], pos0, rows_per_seg, _fp(out)))
        return out

    def debug_flow_cluster_inject(self, block: int) -> None:
        """Test hook: the next plain-launched AR step's k_flow_cluster runs with one workgroup withholding its publish for flow-net block `block` (1-based)."""
        _check(hooks().ptts_debug_flow_cluster_inject(self.h, int(block)))

    def mimi_layer_ffn(self, layer: int, x) -> np.ndarray:
        """x + layer_scale_2 * linear2(gelu(linear1(norm2(x)))) of Mimi decoder-transformer layer `layer` on rows x [R, 512]."""
        x = _f32(x)
        out = np.empty_like(x)
        _check(hooks().ptts_mimi_layer_piece(self.h, layer, 1, _fp(x), x.shape[0], 0, 0, _fp(out)))
        return out

    def open_voice(self, src) -> "DeviceVoice":
        """A model-state voice file (path, or the file's bytes) straight into HBM: safetensors.LoadVoiceModelState +
        initStateFromVoiceModelState + the upload (ptts_voice_open / ptts_voice_open_bytes)."""
        h = C.c_void_p()
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = bytes(src)
            _check(lib().ptts_voice_open_bytes(self.h, buf, len(buf), C.byref(h)))
        else:
            _check(lib().ptts_voice_open(self.h, os.fsencode(src), C.byref(h)))
        return DeviceVoice(h.value, None, self.info)

    def voice_from_embedding(self, emb):
        """A voice embedding (VoiceEmbedding or [T, d_model] array; a list: one build for all) as a model state in HBM
        (ptts_voice_from_embeddings): served like a stock voice instead of being prefilled again by every request."""
        single = not isinstance(emb, (list, tuple))
        items = [emb] if single else list(emb)
        arrs = [_f32(e.data if isinstance(e, VoiceEmbedding) else e) for e in items]
        arrs = [a.reshape(-1, a.shape[-1]) if a.ndim else a for a in arrs]
        n = len(arrs)
        width = arrs[0].shape[-1] if n and arrs[0].ndim else 0
        for a in arrs:
            if a.ndim != 2 or a.shape[-1] != width:
                raise PttsError(PTTS_EINVAL, f"voice embeddings must be [T, D] with one D, got {[list(x.shape) for x in arrs]}")
        pp = (_FP * max(n, 1))(*[_fp(a) for a in arrs])
        fr = np.array([a.shape[0] for a in arrs] or [0], np.int64)
        hs = (C.c_void_p * max(n, 1))()
        _check(lib().ptts_voice_from_embeddings(self.h, pp, _ip(fr), width, n, hs))
        out = [DeviceVoice(hs[i], int(fr[i]), self.info) for i in range(n)]
        return out[0] if single else out

    def voice_state_from_audio(self, pcm, sample_rate=24000):
        """Mono clips (a list: one call) at sample_rate (one rate, or one per clip; resampled to 24 kHz on the device) -> encoder + speaker
        projection + one model-state build (ptts_voice_from_audio_rates).  PARITY UNPINNED like voice_from_audio: the encoder's chain is inferred."""
        single = not isinstance(pcm, (list, tuple))
        clips = [_f32(pcm).reshape(-1)] if single else [_f32(p).reshape(-1) for p in pcm]
        n = len(clips)
        pp = (_FP * max(n, 1))(*[_fp(c) for c in clips])
        ns = np.array([c.size for c in clips] or [0], np.int64)
        rates = _rates(sample_rate, n)
        hs = (C.c_void_p * max(n, 1))()
        _check(lib().ptts_voice_from_audio_rates(self.h, pp, _ip(ns), rates.ctypes.data_as(C.POINTER(C.c_int32)), n, hs))
        out = [DeviceVoice(hs[i], None, self.info) for i in range(n)]
        return out[0] if single else out

    def profile_enable(self, on):   # False / 0: off; True / 1: per-launch events + phases; 2: phases only
        _check(lib().ptts_profile_enable(self.h, int(on)))

    def profile_read(self) -> dict:
        p = _Profile()
        _check(lib().ptts_profile_read(self.h, C.byref(p)))
        return {"kernel": p.kernel.decode(), "launches": int(p.launches), "total_ms": float(p.total_ms),
                "algorithmic_bytes": float(p.algorithmic_bytes), "weight_bytes": float(p.weight_bytes),
                "prefill_ms": float(p.prefill_ms), "ar_loop_ms": float(p.ar_loop_ms), "mimi_ms": float(p.mimi_ms)}

    def new_batch(self, n_slots: int, kv_capacity: int) -> "Batch":
        return Batch(self, n_slots, kv_capacity)

    def decode_latents(self, latents, want_mimi_latent: bool = False):
        """LatentToMimi + MimiDecode (model.go:141,410): [n, frames, 32] -> pcm [n, frames*1920]."""
        lat = _f32(latents)
        if lat.ndim == 2:
            lat = lat[None]
        n, fr, _ = lat.shape
        pcm = np.empty((n, fr * self.info.samples_per_frame), np.float32)
        ml = np.empty((n, self.info.mimi_dim, fr), np.float32) if want_mimi_latent else None
        _check(lib().ptts_decode_latents(self.h, _fp(lat), n, fr, _fp(pcm), _fp(ml)))
        return (pcm, ml) if want_mimi_latent else pcm

    def decode_stages(self, latents):
        """decode_latents plus the decoder transformer's output rows [n, 16 frames, mimi_dim] (mimi.go:733-748):
        returns (pcm, mimi_latent, transformer_out)."""
        lat = _f32(latents)
        if lat.ndim == 2:
            lat = lat[None]
        n, fr, _ = lat.shape
        pcm = np.empty((n, fr * self.info.samples_per_frame), np.float32)
        ml = np.empty((n, self.info.mimi_dim, fr), np.float32)
        xf = np.empty((n, fr * self.info.steps_per_latent, self.info.mimi_dim), np.float32)
        _check(hooks().ptts_decode_stages(self.h, _fp(lat), n, fr, _fp(pcm), _fp(ml), _fp(xf)))
        return pcm, ml, xf

    def speaker_project(self, latent) -> np.ndarray:
        """projectSpeakerConditioning (onnx/voice_encode.go:119-158): Mimi-encoder latents [T, 512] -> voice embedding [T, d_model]."""
        lat = _f32(latent)
        lat = lat.reshape(-1, lat.shape[-1])
        out = np.empty((lat.shape[0], self.info.d_model), np.float32)
        L = lib()
        L.ptts_speaker_project.argtypes = [C.c_void_p, _FP, C.c_int64, _FP]
        _check(L.ptts_speaker_project(self.h, _fp(lat), lat.shape[0], _fp(out)))
        return out

    # ---- the Mimi encoder (PARITY UNPINNED: inferred architecture, no reference fixture; include/ptts.h ptts_mimi_encode) ----
    def encode_audio(self, pcm, sample_rate=24000):
        """mimi.encode_to_latent (onnx/voice_encode.go:23-158) on the GPU: mono f32 PCM at sample_rate (one rate, or one per clip; resampled to
        24 kHz on the device) -> the raw latent [ceil(n24 / 1920), 512].  A list of clips is encoded in one call and gives a list of latents (each
        clip's result is independent of the others)."""
        single = not isinstance(pcm, (list, tuple))
        clips = [_f32(pcm).reshape(-1)] if single else [_f32(p).reshape(-1) for p in pcm]
        n = len(clips)
        rates = _rates(sample_rate, n)
        n24 = [c.size if int(r) == 24000 else max(resample_length(c.size, int(r), 24000), 0) for c, r in zip(clips, rates)]
        outs = [np.empty((max(mimi_encode_frames(k), 0), self.info.mimi_dim), np.float32) for k in n24]
        ns = np.array([c.size for c in clips], np.int64)
        _check(lib().ptts_mimi_encode_rates(self.h, _row_ptrs(clips), _ip(ns), rates.ctypes.data_as(C.POINTER(C.c_int32)), n, _row_ptrs(outs)))
        return outs[0] if single else outs

    def resample(self, x, in_rate: int, out_rate: int):
        """ptts_resample: mono f32 rows (an array, or a list: one launch for all) from in_rate to out_rate on the device."""
        single, rows, n, pp, ns = _rows_in(x)
        outs = [np.empty(max(resample_length(r.size, in_rate, out_rate), 0), np.float32) for r in rows]
        _check(lib().ptts_resample(self.h, pp, _ip(ns), n, int(in_rate), int(out_rate), _row_ptrs(outs)))
        return outs[0] if single else outs

    def dsp_rows(self, x, normalize: bool = False, dc_block: bool = False, fade_in_ms: float = 0.0, fade_out_ms: float = 0.0, opts: Optional[DspOpts] = None):
        """ptts_dsp_rows: dsp_apply's chain on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all)."""
        single, rows, n, pp, ns = _rows_in(x)
        outs = [np.empty(r.size, np.float32) for r in rows]
        o = opts if opts is not None else DspOpts(1 if normalize else 0, 1 if dc_block else 0, float(fade_in_ms), float(fade_out_ms))
        _check(lib().ptts_dsp_rows(self.h, pp, _ip(ns), n, C.byref(o), _row_ptrs(outs)))
        return outs[0] if single else outs

    def _stage_rows(self, entry, x, each, pointer_type, pointer_of):
        """The host-rows entry points that take one option per row: each is one for every row, or one per row (None copies that row)."""
        single, rows, n, pp, ns = _rows_in(x)
        per_row = list(each) if isinstance(each, (list, tuple)) else [each] * n
        outs = [np.empty(r.size, np.float32) for r in rows]
        po = (pointer_type * max(n, 1))(*[pointer_of(o) if o is not None else None for o in per_row])
        _check(entry(self.h, po, pp, _ip(ns), n, _row_ptrs(outs)))
        return outs[0] if single else outs

    def eq_rows(self, x, eq):
        """ptts_eq_rows: Eq.apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all).  eq: one Eq for
        every row, or one per row (None copies that row)."""
        return self._stage_rows(lib().ptts_eq_rows, x, eq, C.c_void_p, lambda e: e.h)

    def compress_rows(self, x, compressor):
        """ptts_compress_rows: compress_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all).
        compressor: one CompressorOpts for every row, or one per row (None copies that row)."""
        return self._stage_rows(lib().ptts_compress_rows, x, compressor, C.POINTER(CompressorOpts), C.pointer)

    def limit_rows(self, x, limiter):
        """ptts_limit_rows: limit_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all).
        limiter: one LimiterOpts for every row, or one per row (None copies that row)."""
        return self._stage_rows(lib().ptts_limit_rows, x, limiter, C.POINTER(LimiterOpts), C.pointer)

    def deess_rows(self, x, deesser):
        """ptts_deess_rows: deess_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all).
        deesser: one DeesserOpts for every row, or one per row (None copies that row)."""
        return self._stage_rows(lib().ptts_deess_rows, x, deesser, C.POINTER(DeesserOpts), C.pointer)

    def trim_rows(self, x, trim):
        """ptts_trim_rows: trim_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all), by the kernels
        generate_joined runs.  trim: one TrimOpts for every row, or one per row (None copies that row).  Returns (rows, their TrimInfo records);
        for a single array (the row, its record)."""
        single, outs, infos = self._part_rows(lib().ptts_trim_rows, x, [(trim, TrimOpts)], lambda r, o: r.size, TrimInfo, lambda v: v.n_out)
        recs = [TrimInfo(v.lo, v.hi, v.n_out, v.cuts, v.speech, 0) for v in infos[:len(outs)]]
        return (outs[0], recs[0]) if single else (outs, recs)

    def _part_rows(self, entry, x, each, size_of, back=C.c_int64, n_out=int):
        """The host-rows entry points of a joined call's part stages (trim, tempo, pitch).  each: per option array the entry point takes, (the options
        -- one for every row, or one per row -- and their struct); size_of(row, its options...): the floats the row's output holds; back: what the
        entry point reports per row behind the outputs, n_out(one of them) the row's length.  Returns (single, the outputs cut to length, the reports)."""
        single, rows, n, pp, ns = _rows_in(x)
        per = [list(o) if isinstance(o, (list, tuple)) else [o] * n for o, _ in each]
        outs = [np.empty(size_of(*ro), np.float32) for ro in zip(rows, *per)]
        po = [(C.POINTER(t) * max(n, 1))(*[C.pointer(o) if o is not None else None for o in col]) for col, (_, t) in zip(per, each)]
        got = (back * max(n, 1))()
        _check(entry(self.h, *po, pp, _ip(ns), n, _row_ptrs(outs), got))
        return single, [o[:n_out(got[i])] for i, o in enumerate(outs)], got

    def tempo_rows(self, x, tempo):
        """ptts_tempo_rows: tempo_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch of each kernel for all), by the
        kernels generate_joined runs.  tempo: one TempoOpts for every row, or one per row (None copies that row).  Returns the time-scaled rows."""
        # (sized here, so that options the library refuses reach the library: it names the row)
        single, outs, _ = self._part_rows(lib().ptts_tempo_rows, x, [(tempo, TempoOpts)], _tempo_size)
        return outs[0] if single else outs

    def pitch_rows(self, x, pitch, tempo=None):
        """ptts_pitch_rows: pitch_apply on the device, on mono f32 rows at 24 kHz (an array, or a list: one launch sequence for all), by the kernels
        generate_joined runs.  pitch, tempo: one PitchOpts / TempoOpts for every row, or one per row (a row with a pitch of None gets its tempo
        alone, with both None it is copied).  Returns the shifted rows."""
        L = lib()

        def size(r, p, t):
            # (a row whose length the library refuses is sized 1, so that the options reach the library: it names the row, and writes nothing)
            return max(_tempo_size(r, t) if p is None else int(L.ptts_pitch_length(C.byref(p), None if t is None else C.byref(t), r.size)), 1)
        single, outs, _ = self._part_rows(L.ptts_pitch_rows, x, [(pitch, PitchOpts), (tempo, TempoOpts)], size)
        outs = [o.copy() for o in outs]
        return outs[0] if single else outs

    def formant_rows(self, x, formant, pitch, tempo=None):
        """ptts_formant_rows: formant_apply on the device, on mono f32 rows at 24 kHz, by the kernels generate_joined runs.  formant, pitch, tempo: one
        FormantOpts / PitchOpts / TempoOpts for every row, or one per row (a row with a formant of None is exactly pitch_rows' row).  Returns the rows."""
        L = lib()

        def size(r, f, p, t):
            return max(_tempo_size(r, t) if p is None else int(L.ptts_pitch_length(C.byref(p), None if t is None else C.byref(t), r.size)), 1)
        single, outs, _ = self._part_rows(L.ptts_formant_rows, x, [(formant, FormantOpts), (pitch, PitchOpts), (tempo, TempoOpts)], size)
        outs = [o.copy() for o in outs]
        return outs[0] if single else outs

    def true_peak_rows(self, x):
        """ptts_true_peak_rows: true_peak() of mono f32 rows at 24 kHz (an array, or a list: one launch for all), measured on the device."""
        single, rows, n, pp, ns = _rows_in(x)
        peaks = np.zeros(max(n, 1), np.float32)
        _check(lib().ptts_true_peak_rows(self.h, pp, _ip(ns), n, _fp(peaks)))
        return peaks[0] if single else peaks[:n]

    def _loudness_rows(self, x, target):
        single, rows, n, pp, ns = _rows_in(x)
        lufs = np.zeros(max(n, 1), np.float64)
        dp = lufs.ctypes.data_as(_DP)
        if target is None:
            _check(lib().ptts_loudness_rows(self.h, pp, _ip(ns), n, dp))
            return float(lufs[0]) if single else lufs[:n]
        outs = [np.empty(r.size, np.float32) for r in rows]
        _check(lib().ptts_loudness_normalize_rows(self.h, pp, _ip(ns), n, float(target), _row_ptrs(outs), dp))
        return (outs[0], float(lufs[0])) if single else (outs, lufs[:n])

    def loudness_rows(self, x):
        """ptts_loudness_rows: BS.1770-4 integrated loudness (LUFS, -inf: nothing above the gates) of mono f32 rows at 24 kHz, measured on the device."""
        return self._loudness_rows(x, None)

    def loudness_normalize_rows(self, x, target_lufs: float):
        """ptts_loudness_normalize_rows: (rows at the target -- never above peak 1 --, the loudness measured before), on the device."""
        return self._loudness_rows(x, float(target_lufs))

    def loudness_energies(self, x):
        """Test hook (libptts_hooks.so ptts_debug_loudness_energies): the rows' 480-sample K-weighted energies as the device kernels compute them."""
        return loudness_energies(x, self)

    def dsp_windows(self, x, cuts, opts: Optional[DspOpts] = None):
        """ptts_debug_dsp_windows (libptts_hooks.so): the causal chain of opts over rows of 24 kHz samples in windows cut at `cuts` (ascending multiples
        of 1920), state carried on the device, by the launches a streamed joined call runs.  The bits of dsp_rows."""
        single, rows, n, pp, ns = _rows_in(x)
        outs = [np.empty(r.size, np.float32) for r in rows]
        cs = np.ascontiguousarray(cuts, np.int64).reshape(-1)
        _check(hooks().ptts_debug_dsp_windows(self.h, pp, _ip(ns), n, C.byref(opts) if opts is not None else None,
                                              _ip(cs) if cs.size else None, int(cs.size), _row_ptrs(outs)))
        return outs[0] if single else outs

    def join_rows(self, parts, join: Optional[JoinOpts] = None) -> np.ndarray:
        """ptts_join_rows: join() on the device, by the kernel generate_joined runs: one upload, k_join, one download."""
        rows, n, pp, ns = _join_in(parts)
        o = join if join is not None else JoinOpts()
        out = np.empty(max(join_length(ns[:n], o), 1), np.float32)
        _check(lib().ptts_join_rows(self.h, pp, _ip(ns), n, C.byref(o), _fp(out)))
        return out[:join_length(ns[:n], o)]

    def join_parts_rows(self, parts, parts_opts, join: Optional[JoinOpts] = None, gains: bool = False):
        """ptts_join_parts_rows: join_parts() on the device, by the kernels a joined call with a list runs: one upload, the loudness rows' measuring
        kernels for the levels, k_join_gain (k_join for a table without a gain), one download.  gains: also the f32 gain of every part."""
        rows, n, pp, ns = _join_in(parts)
        o = join if join is not None else JoinOpts()
        po = _part_list(parts_opts)
        total = join_parts_length(ns[:n], parts_opts, o)
        out = np.empty(max(total, 1), np.float32)
        g = np.ones(max(n, 1), np.float32)
        _check(lib().ptts_join_parts_rows(self.h, pp, _ip(ns), n, C.byref(o), po, _fp(out), _fp(g)))
        return (out[:total], g[:n]) if gains else out[:total]

    def pcm_encode(self, x, pcm_format: int) -> np.ndarray:
        """ptts_pcm_encode: the device egress conversion of 24 kHz f32 samples into PCM_F32 / PCM_S16 / PCM_ULAW / PCM_ALAW."""
        x = _f32(x).reshape(-1)
        out = np.empty(x.size, _PCM_DTYPES.get(int(pcm_format), "<f4"))
        _check(lib().ptts_pcm_encode(self.h, _fp(x), x.size, int(pcm_format), out.ctypes.data))
        return out

    def voice_from_audio(self, pcm, sample_rate=24000) -> VoiceEmbedding:
        """EncodeVoice (onnx/voice_encode.go:23-158): encoder + speaker projection on the device -> a VoiceEmbedding [1, frames, d_model]
        for RuntimeGenerateConfig.voice_embedding.  A clip at another sample_rate is resampled to 24 kHz on the device first."""
        if int(sample_rate) != 24000:
            lat = self.encode_audio(pcm, sample_rate)
            return VoiceEmbedding(self.speaker_project(lat), (1, lat.shape[0], self.info.d_model))   # (the layout of the 24 kHz call's data)
        x = _f32(pcm).reshape(-1)
        out = np.empty((max(mimi_encode_frames(x.size), 0), self.info.d_model), np.float32)
        frames = C.c_int64(0)
        L = lib()
        L.ptts_voice_encode_audio.argtypes = [C.c_void_p, _FP, C.c_int64, _FP, C.POINTER(C.c_int64)]
        _check(L.ptts_voice_encode_audio(self.h, _fp(x), x.size, _fp(out), C.byref(frames)))
        return VoiceEmbedding(out, (1, int(frames.value), self.info.d_model))

    def encode_stages(self, pcm) -> list:
        """Test hook (libptts_hooks.so ptts_debug_encode_stages): the encoder's ten observation points on one clip, channels-last arrays."""
        x = _f32(pcm).reshape(-1)
        H = hooks()
        H.ptts_debug_encode_stages.argtypes = [C.c_void_p, _FP, C.c_int64, C.POINTER(_FP), _IP]
        shapes = np.zeros((10, 2), np.int64)
        _check(H.ptts_debug_encode_stages(self.h, _fp(x), x.size, None, _ip(shapes)))
        outs = [np.empty((int(r), int(c)), np.float32) for r, c in shapes]
        po = (_FP * len(outs))(*[_fp(o) for o in outs])
        _check(H.ptts_debug_encode_stages(self.h, _fp(x), x.size, po, _ip(shapes)))
        return outs

    def noise_rows(self, seed: int, temperature: float, rows: int) -> np.ndarray:
        """The device draw of makeGaussianNoise (flow_lm.go:386-408) a request with (noise_seed, temperature) consumes."""
        out = np.empty((rows, self.info.ldim), np.float32)
        _check(lib().ptts_noise_rows(self.h, C.c_uint64(seed), C.c_float(temperature), rows, _fp(out)))
        return out

    def flow_direction(self, c, s: float, t: float, x) -> np.ndarray:
        c = _f32(c).reshape(-1, self.info.d_model)
        x = _f32(x).reshape(-1, self.info.ldim)
        out = np.empty_like(x)
        _check(lib().ptts_flow_direction(self.h, _fp(c), s, t, _fp(x), c.shape[0], _fp(out)))
        return out

    # -- batched GenerateAudio
    def _fill_request(self, r, toks, cfg, keep):
        t = toks if type(toks) is np.ndarray and toks.dtype == np.int64 and toks.flags.c_contiguous else np.ascontiguousarray(toks, np.int64)
        keep.append(t)
        r.tokens, r.n_tokens = _ip(t), t.size
        r.temperature, r.eos_threshold = cfg.temperature, min(cfg.eos_threshold, 3.0e38)
        r.max_steps, r.estimated_max_steps = cfg.max_steps, cfg.estimated_max_steps
        r.lsd_steps, r.frames_after_eos = cfg.lsd_decode_steps, cfg.frames_after_eos
        if cfg.voice_embedding is not None:
            ve = _f32(cfg.voice_embedding.data).reshape(-1, self.info.d_model)
            keep.append(ve)
            r.voice_embedding, r.voice_frames = _fp(ve), ve.shape[0]
        if cfg.voice_model_state is not None:
            ptrs, steps, offs, arrs = _voice_arrays(cfg.voice_model_state, self.info.n_layers)
            keep += [ptrs, steps, offs, arrs]
            r.voice_caches, r.voice_cache_steps, r.voice_offsets = ptrs, _ip(steps), _ip(offs)
        if cfg.device_voice is not None:
            r.voice = cfg.device_voice.h
        if cfg.noise is not None:
            nz = _f32(cfg.noise).reshape(-1, self.info.ldim)
            keep.append(nz)
            r.noise = _fp(nz)
            r.noise_rows = nz.shape[0]
        r.noise_seed = int(cfg.noise_seed)
        if cfg.step_callback is not None:
            cb = _STEP_CB(lambda _u, s, m, f=cfg.step_callback: f(s, m))
            keep.append(cb)
            r.step_callback = cb
        if cfg.cancel is not None:
            r.cancel = cfg.cancel.ctypes.data_as(C.POINTER(C.c_int32))
        r.want_latents = 1 if cfg.want_latents else 0
        r.pcm_format = _pcm_format(cfg)
        r.sample_rate = int(getattr(cfg, "sample_rate", 0))
        dsp = _dsp_opts(cfg)
        if dsp is not None:
            keep.append(dsp)
            r.dsp = C.pointer(dsp)
        r.loudness = int(getattr(cfg, "loudness", 0))
        if cfg.pcm_callback is not None:
            dt = np.dtype(_PCM_DTYPES.get(r.pcm_format, "<f4"))

            def _pcm(_u, off, n, ptr, f=cfg.pcm_callback, dt=dt):
                f(int(off), np.frombuffer(C.string_at(ptr, int(n) * np.dtype(dt).itemsize), dtype=dt))

            pcb = _PCM_CB(_pcm)
            keep.append(pcb)
            r.pcm_callback = pcb
            r.stream_frames = int(cfg.stream_frames)

    def _take_result(self, rs, cfg) -> "GenerateResult":
        fmt = _pcm_format(cfg)   # PCM16 / G.711 egress: int16 / uint8 samples encoded on the device
        field = {PCM_F32: "pcm", PCM_S16: "pcm16"}.get(fmt, "pcm8")
        if rs.n_samples:
            # zero-copy: the array views the library's (page-locked) result buffer and gives it back to the pool
            # when it is garbage-collected
            pcm = np.asarray(_OwnedBuffer(getattr(rs, field), int(rs.n_samples), _PCM_DTYPES[fmt]))
            setattr(rs, field, None)
        else:
            pcm = np.zeros(0, _PCM_DTYPES[fmt])
        lat = None
        if cfg.want_latents:
            lat = np.ctypeslib.as_array(rs.latents, (rs.n_frames, self.info.ldim)).copy()
        return GenerateResult(pcm, int(rs.n_frames), int(rs.eos_step), lat)

    def generate_batch(self, token_lists: Sequence[Sequence[int]], cfgs: Sequence[RuntimeGenerateConfig]) -> list[GenerateResult]:
        n = len(token_lists)
        reqs = (_Request * n)()
        ress = (_Result * n)()
        keep = []
        for i, (toks, cfg) in enumerate(zip(token_lists, cfgs)):
            self._fill_request(reqs[i], toks, cfg, keep)
        rc = lib().ptts_generate(self.h, reqs, n, ress)
        out = []
        raw = np.frombuffer(ress, dtype=_RESULT_DTYPE, count=n)   # the result structs as one table: no per-field ctypes objects
        try:
            _check(rc)
            if raw["latents"].any():                                # want_latents: the general (slower) path
                for i in range(n):
                    out.append(self._take_result(ress[i], cfgs[i]))
            else:
                nf, es, ns = raw["n_frames"].tolist(), raw["eos_step"].tolist(), raw["n_samples"].tolist()
                a32, a16, a8 = raw["pcm"].tolist(), raw["pcm16"].tolist(), raw["pcm8"].tolist()
                raw["pcm"][:] = 0                                   # ownership moves to the arrays below (zero-copy, freed on collection)
                raw["pcm16"][:] = 0
                raw["pcm8"][:] = 0
                for i in range(n):
                    fmt = _pcm_format(cfgs[i])
                    addr = a8[i] if fmt >= PCM_ULAW else a16[i] if fmt == PCM_S16 else a32[i]
                    if ns[i] and addr:
                        pcm = np.asarray(_OwnedBuffer(addr, ns[i], _PCM_DTYPES[fmt]))
                    else:
                        if addr:
                            _free_addr(addr)
                        pcm = np.zeros(0, _PCM_DTYPES[fmt])
                    out.append(GenerateResult(pcm, nf[i], es[i], None))
        finally:
            if raw["pcm"].any() or raw["pcm16"].any() or raw["pcm8"].any() or raw["latents"].any():
                for i in range(n):
                    lib().ptts_free_result(C.byref(ress[i]))
        return out


    def generate_joined(self, token_lists: Sequence[Sequence[int]], cfgs: Sequence[RuntimeGenerateConfig], join: Optional[JoinOpts] = None,
                        pcm_callback=None, first_group: Optional[int] = None, stream: Optional[JoinStreamOpts] = None,
                        parts: Optional[Sequence[PartOpts]] = None) -> JoinedResult:
        """ptts_generate_joined: the chunks of one text, generated as generate_batch generates them, joined on the device (gap or crossfade), the
        chain of `join` run once over the joined audio, one egress.  The cfgs carry no post-processing, rate or format of their own.  A failed call
        raises PttsError with the chunks' records in its `parts`.
        pcm_callback(offset, samples), first_group or stream (a JoinStreamOpts as it is) make it ptts_generate_joined_streamed: the audio is handed
        over group by group, from a library thread, while the later groups run; offsets count samples of the egress, `samples` is a copy in its format.
        parts (one PartOpts per chunk) makes it ptts_generate_joined_parts: each part's own trim, pitch, tempo and volume and the seam behind it; the
        result then carries the parts' gains (JoinedResult.gains)."""
        n = len(token_lists)
        part_opts = parts
        reqs = (_Request * max(n, 1))()
        parts = (JoinPart * max(n, 1))()
        res = _Result()
        keep = []
        for i, (toks, cfg) in enumerate(zip(token_lists, cfgs)):
            self._fill_request(reqs[i], toks, cfg, keep)
        o = join if join is not None else JoinOpts()
        if stream is None and (pcm_callback is not None or first_group is not None):
            cb = None
            if pcm_callback is not None:
                dt = np.dtype(_PCM_DTYPES.get(int(o.pcm_format), "<f4"))
                cb = _PCM_CB(lambda _u, off, cnt, ptr: pcm_callback(int(off), np.frombuffer(C.string_at(ptr, int(cnt) * dt.itemsize), dtype=dt)))
            stream = JoinStreamOpts(first_group or 0, cb)
        gains = None
        if part_opts is not None:
            if len(part_opts) != n:
                raise PttsError(PTTS_EINVAL, "generate_joined: parts holds %d PartOpts for %d chunks" % (len(part_opts), n))
            gains = np.ones(max(n, 1), np.float32)
            rc = lib().ptts_generate_joined_parts(self.h, reqs, n, C.byref(o), _part_list(part_opts), C.byref(stream) if stream is not None else None,
                                                  C.byref(res), parts, _fp(gains))
        elif stream is not None:
            rc = lib().ptts_generate_joined_streamed(self.h, reqs, n, C.byref(o), C.byref(stream), C.byref(res), parts)
        else:
            rc = lib().ptts_generate_joined(self.h, reqs, n, C.byref(o), C.byref(res), parts)
        records = [JoinPart(p.offset, p.n_samples, p.n_frames, p.eos_step, p.status, 0) for p in parts[:n]]
        try:
            _check(rc)
        except PttsError as e:
            lib().ptts_free_result(C.byref(res))
            e.parts = records
            raise
        fmt = int(o.pcm_format)
        field = {PCM_F32: "pcm", PCM_S16: "pcm16"}.get(fmt, "pcm8")
        addr = C.cast(getattr(res, field), C.c_void_p).value
        if res.n_samples and addr:
            pcm = np.asarray(_OwnedBuffer(addr, int(res.n_samples), _PCM_DTYPES[fmt]))   # zero-copy, back to the pool on collection
        else:
            lib().ptts_free_result(C.byref(res))
            pcm = np.zeros(0, _PCM_DTYPES[fmt])
        out = JoinedResult(pcm, int(res.n_frames), records)
        if gains is not None:
            out.gains = gains[:n]
        return out


class DeviceVoice:
    """A voice model state in HBM (ptts_voice).  offset: the keys it holds (ptts_voice_offset)."""

    def __init__(self, handle: int, offset: Optional[int] = None, info: Optional["ModelInfo"] = None):
        self.h, self.info = handle, info
        if offset is None or offset < 0:
            o = C.c_int64()
            _check(lib().ptts_voice_offset(self.h, C.byref(o)))
            offset = int(o.value)
        self.offset = offset

    def read_state(self, layer: int) -> np.ndarray:
        """Layer `layer` as the reference's cache [2, 1, offset, H, Dh] f32 (ptts_voice_read_state)."""
        out = np.empty((2, 1, self.offset, self.info.n_heads, self.info.d_model // self.info.n_heads), np.float32)
        _check(lib().ptts_voice_read_state(self.h, layer, _fp(out)))
        return out

    def state(self) -> VoiceModelState:
        """The voice as safetensors.VoiceModelState: per layer "cache" [2, 1, offset, H, Dh] and "offset" [1]."""
        return VoiceModelState({f"transformer.layers.{i}.self_attn": {"cache": self.read_state(i), "offset": np.array([self.offset], np.int64)}
                                for i in range(self.info.n_layers)})

    def to_bytes(self) -> bytes:
        """The voice as a model-state voice file, in memory (ptts_voice_write_bytes)."""
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        _check(lib().ptts_voice_write_bytes(self.h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib().ptts_free_bytes(p)

    def save(self, path: str) -> None:
        """The voice as a model-state voice file (ptts_voice_write): what Model.open_voice and load_voice_conditioning read."""
        _check(lib().ptts_voice_write(self.h, os.fsencode(path)))

    def close(self):
        if self.h:
            lib().ptts_voice_free(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


VOICE_FILE_UNKNOWN, VOICE_FILE_EMBEDDING, VOICE_FILE_MODEL_STATE = 0, 1, 2
VOICE_FILE_KIND_NAMES = {0: "unknown", 1: "embedding", 2: "model_state"}   # safetensors.VoiceFileKind (reader.go:20-26)


class VoiceFile:
    """A voice safetensors file read by the library (host only): InspectVoiceFile, LoadVoiceEmbedding, LoadVoiceModelState
    (internal/safetensors/reader.go:69-155) over ptts_voice_file_*."""

    def __init__(self, src):
        self.h = C.c_void_p()
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = bytes(src)
            _check(lib().ptts_voice_file_open_bytes(buf, len(buf), C.byref(self.h)))
        else:
            _check(lib().ptts_voice_file_open(os.fsencode(src), C.byref(self.h)))

    @property
    def kind(self) -> str:
        return VOICE_FILE_KIND_NAMES[int(lib().ptts_voice_file_kind(self.h))]

    def embedding(self) -> VoiceEmbedding:
        p, shape = _FP(), np.zeros(3, np.int64)
        _check(lib().ptts_voice_file_embedding(self.h, C.byref(p), _ip(shape)))
        n = int(shape.prod())
        data = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.float32)
        return VoiceEmbedding(data.reshape(tuple(int(x) for x in shape)), [int(x) for x in shape])

    def model_state(self) -> VoiceModelState:
        n = C.c_int32()
        _check(lib().ptts_voice_file_modules(self.h, C.byref(n)))
        mods = {}
        for i in range(n.value):
            name, cache, off = C.c_char_p(), _VoiceTensor(), _VoiceTensor()
            _check(lib().ptts_voice_file_module(self.h, i, C.byref(name), C.byref(cache), C.byref(off)))
            m = {}
            for key, t in (("cache", cache), ("offset", off)):
                if not t.data:
                    continue
                shape = tuple(int(t.shape[d]) for d in range(t.rank))
                m[key] = (np.ctypeslib.as_array(t.data, shape=(int(t.count),)).copy() if t.count else np.zeros(0, np.float32)).reshape(shape)
            mods[name.value.decode()] = m
        return VoiceModelState(mods)

    def state_arrays(self, n_layers: int, heads: int = 0, head_dim: int = 0):
        """initStateFromVoiceModelState's checks (flow_transformer.go:451-590): per layer (cache [2,1,T,H,D], T, offset)."""
        ptrs, steps, offs = (_FP * max(n_layers, 1))(), np.zeros(max(n_layers, 1), np.int64), np.zeros(max(n_layers, 1), np.int64)
        _check(lib().ptts_voice_file_state(self.h, n_layers, heads, head_dim, ptrs, _ip(steps), _ip(offs)))
        return ptrs, steps[:n_layers], offs[:n_layers]

    def close(self):
        if self.h:
            lib().ptts_voice_file_close(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def voice_state_file_bytes(caches: Sequence[np.ndarray], offset: int) -> bytes:
    """A model-state voice file from host caches (caches[l]: [2, 1, offset, H, Dh] f32; ptts_voice_state_write_bytes)."""
    cs = [_f32(c) for c in caches]
    if not cs or any(c.ndim != 5 or c.shape[:3] != (2, 1, offset) or c.shape != cs[0].shape for c in cs):
        raise PttsError(PTTS_EINVAL, f"voice caches must be [2, 1, {offset}, H, Dh], got {[list(c.shape) for c in cs]}")
    pp = (_FP * len(cs))(*[_fp(c) for c in cs])
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    _check(lib().ptts_voice_state_write_bytes(pp, offset, len(cs), cs[0].shape[3], cs[0].shape[4], C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value)
    finally:
        lib().ptts_free_bytes(p)


def load_voice_conditioning(voice_path: str) -> dict:
    """tts.loadVoiceConditioning (service.go:216-246): {} for a blank path, else the keyword RuntimeGenerateConfig takes
    (voice_model_state or voice_embedding), chosen by the file's kind; error prefixes as in the reference."""
    if not voice_path or not voice_path.strip():
        return {}
    try:
        vf = VoiceFile(voice_path)
    except PttsError as e:
        raise PttsError(e.code, f"inspect voice safetensors: {e}") from None
    try:
        if vf.kind == "model_state":
            try:
                return {"voice_model_state": vf.model_state()}
            except PttsError as e:
                raise PttsError(e.code, f"load voice model state: {e}") from None
        try:
            return {"voice_embedding": vf.embedding()}
        except PttsError as e:
            raise PttsError(e.code, f"load voice embedding: {e}") from None
    finally:
        vf.close()


def _voice_arrays(state: VoiceModelState, n_layers: int):
    caches, steps, offs = [], [], []
    for i in range(n_layers):
        name = f"transformer.layers.{i}.self_attn"  # flow_transformer.go:513-515
        mod = state.modules.get(name)
        if mod is None:
            raise PttsError(PTTS_EINVAL, f'native: voice model state missing module "{name}"')
        if "cache" not in mod:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" missing cache')
        if "offset" not in mod:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" missing offset')
        c = _f32(mod["cache"])
        if c.ndim != 5 or c.shape[0] != 2:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" cache shape {list(c.shape)}, want [2,B,T,H,D]')
        if c.shape[1] != 1:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" batch {c.shape[1]}, want 1')
        if c.shape[3] != 16 or c.shape[4] != 64:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" heads {c.shape[3]}, want 16')
        off = np.asarray(mod["offset"], np.float32).reshape(-1)
        if off.size == 0:
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" has empty offset tensor')
        if np.float32(int(off[0])) != off[0]:  # flow_transformer.go:554-566
            raise PttsError(PTTS_EINVAL, f'native: voice model state module "{name}" offset {off[0]} is not an integer')
        caches.append(c)
        steps.append(c.shape[2])
        offs.append(int(off[0]))
    ptrs = (_FP * n_layers)(*[_fp(c) for c in caches])
    return ptrs, np.array(steps, np.int64), np.array(offs, np.int64), caches


class Batch:
    """n_slots x native.FlowLMState (flow_lm.go:45-49): NewFlowState / PromptFlow / SampleNextLatentStateful."""

    def __init__(self, model: Model, n_slots: int, kv_capacity: int):
        self.model, self.n = model, n_slots
        h = C.c_void_p()
        _check(lib().ptts_batch_new(model.h, n_slots, kv_capacity, C.byref(h)))
        self.h = h.value

    def close(self):
        if self.h:
            lib().ptts_batch_free(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():   # the HIP runtime may already be gone at interpreter teardown
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def reset(self):
        _check(lib().ptts_batch_reset(self.h))

    def set_voice_state(self, slot: int, state: VoiceModelState):
        ptrs, steps, offs, arrs = _voice_arrays(state, self.model.info.n_layers)
        _check(lib().ptts_batch_set_voice_state(self.h, slot, ptrs, _ip(steps), _ip(offs)))

    def prompt(self, embs: Sequence[np.ndarray]):
        """embs[s]: [T_s, d_model] rows for slot s (voice rows first, then text rows)."""
        d = self.model.info.d_model
        rows = [_f32(e).reshape(-1, d) for e in embs]
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([r.shape[0] for r in rows])
        cat = np.concatenate(rows, 0) if offs[-1] else np.zeros((0, d), np.float32)
        cat = np.ascontiguousarray(cat)
        _check(lib().ptts_batch_prompt(self.h, _fp(cat), _ip(offs)))

    def step(self, frames_in, lsd_steps: int = 1, noise=None):
        m = self.model.info
        fi = _f32(frames_in).reshape(self.n, m.ldim)
        nz = _f32(noise).reshape(self.n, m.ldim) if noise is not None else None
        fo = np.empty((self.n, m.ldim), np.float32)
        eos = np.empty(self.n, np.float32)
        last = np.empty((self.n, m.d_model), np.float32)
        _check(lib().ptts_batch_step(self.h, _fp(fi), lsd_steps, _fp(nz), _fp(fo), _fp(eos), _fp(last)))
        return fo, eos, last

    def offsets(self) -> np.ndarray:
        o = np.zeros(self.n, np.int64)
        _check(lib().ptts_batch_offsets(self.h, _ip(o)))
        return o

    def read_kv(self, slot: int, layer: int):
        n = int(self.offsets()[slot])
        k = np.empty((self.model.info.n_heads, n, 64), np.float32)
        v = np.empty_like(k)
        _check(lib().ptts_batch_read_kv(self.h, slot, layer, _fp(k), _fp(v)))
        return k, v


class Runtime:
    """tts.Runtime (runtime.go:42-45) on one MI355X: GenerateAudio + Close (+ MimiTiming)."""

    def __init__(self, model: Model):
        self.model = model

    def generate_audio(self, tokens: Sequence[int], cfg: RuntimeGenerateConfig) -> np.ndarray:
        """GenerateAudio (runtime_native_safetensors.go:52-238): returns f32 PCM @ 24 kHz."""
        if self.model is None or self.model.h is None:
            raise PttsError(PTTS_EINVAL, "native-safetensors runtime unavailable")
        return self.model.generate_batch([tokens], [cfg])[0].pcm

    def generate(self, tokens: Sequence[int], cfg: RuntimeGenerateConfig) -> GenerateResult:
        if self.model is None or self.model.h is None:
            raise PttsError(PTTS_EINVAL, "native-safetensors runtime unavailable")
        return self.model.generate_batch([tokens], [cfg])[0]

    def mimi_timing(self) -> tuple[float, float, int]:
        """MimiTiming (runtime_native_safetensors.go:40-49): 12.5, 200, 16."""
        i = self.model.info
        return i.frame_rate, i.encoder_frame_rate, i.steps_per_latent

    def close(self):
        """Close (runtime_native_safetensors.go:240-244): nil-safe."""
        if self.model is not None:
            self.model.close()


# ----------------------------------------------------------------------------- kernel-level entry points

def op_linear(x, w, bias=None) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    out, inp = w.shape
    rows = x.size // inp
    y = np.empty(x.shape[:-1] + (out,), np.float32)
    b = _f32(bias) if bias is not None else None
    _check(lib().ptts_op_linear(_fp(x), _fp(w), _fp(b), rows, inp, out, _fp(y)))
    return y


def op_layernorm(x, w, b, eps: float) -> np.ndarray:
    x = _f32(x)
    d = x.shape[-1]
    y = np.empty_like(x)
    wa = _f32(w) if w is not None else None
    ba = _f32(b) if b is not None else None
    _check(lib().ptts_op_layernorm(_fp(x), _fp(wa), _fp(ba), eps, x.size // d, d, _fp(y)))
    return y


def op_rope(x, cos, sin, pos: int) -> np.ndarray:
    x = _f32(x).copy()
    cos, sin = _f32(cos), _f32(sin)
    seq, dim = x.shape[-2], x.shape[-1]
    _check(lib().ptts_op_rope(_fp(x), _fp(cos), _fp(sin), cos.shape[0], x.size // (seq * dim), seq, dim, pos))
    return x


def op_attention_positions(q, k, v, posq, posk, context: int) -> np.ndarray:
    q, k, v = _f32(q), _f32(k), _f32(v)
    b, h, tq, d = q.shape
    tk = k.shape[2]
    pq, pk = np.ascontiguousarray(posq, np.int64), np.ascontiguousarray(posk, np.int64)
    out = np.empty((b, h, tq, d), np.float32)
    _check(lib().ptts_op_attention_positions(_fp(q), _fp(k), _fp(v), b, h, tq, tk, d, _ip(pq), _ip(pk), context, _fp(out)))
    return out


TALL_OPS = {"rowprep": 1, "tall": 2, "both": 3}   # PTTS_TALL_*


class _TallArgs(C.Structure):   # ptts_tall_args
    _fields_ = ([(n, C.c_int32) for n in ("op", "M", "rows", "N", "K", "epi", "splitk", "form", "psplit", "want_x_out", "want_y_out")] + [("eps", C.c_float)] +
                [(n, C.c_int64) for n in ("ldx", "ldy", "lda", "ldc", "ldr", "ldp", "pstride", "zstride", "launched_cap")] +
                [(n, _FP) for n in ("x", "planes", "pbias", "ln_w", "ln_b", "W", "bias", "R", "out", "x_out", "y_out")] +
                [(n, _U16P) for n in ("ch", "cl", "yh", "yl")] +
                [("form_out", _I32P), ("grid", _I32P), ("launched", C.c_char_p)])


def debug_tall(op, x, *, M=None, K=None, w=None, bias=None, residual=None, epi=0, splitk=1, form=0, ln=None, planes=None, pbias=None, want_x_out=True,
               want_y_out=True, out_planes=False, ldy=None, lda=None, ldc=None, ldp=None, zstride=None):
    """k_rowprep and k_tall (csrc/tall.hip) on host operands (ptts_debug_tall, include/ptts_debug.h): op is a key of TALL_OPS.  x [rows, ldx] ("tall": [rows,
    lda]); the launch is told of M rows (default: all) of width K (default: ln's weight's, "tall": w's).  ln = (weight, bias, eps); planes [psplit, pstride], each plane
    holding dense [M, K] rows; w [N, K]; residual [rows, ldr].  Returns a dict of whole buffers, 0xff bytes where nothing was stored: "out" ([rows, ldc] f32, or
    the planes [splitk, zstride]; None with out_planes), "ch" / "cl" ([rows, ldp] bf16 bits, with out_planes), "x_out" / "y_out" [rows, K], "yh" / "yl" [rows, ldy]
    bf16 bits (None for "tall"), "form" (the block height launched), "grid", "launched" ({kernel: count}).  A refusal raises PttsError with the same dict as
    its `partial` attribute."""
    x = _f32(x)
    rows = int(x.shape[0])
    prep, prod = op in ("rowprep", "both"), op in ("tall", "both")
    w = _f32(w) if w is not None else None
    if K is not None:
        k = int(K)
    elif prep:
        k = int(np.asarray(ln[0]).shape[0]) if ln is not None else int(x.shape[1])
    else:
        k = int(w.shape[1]) if w is not None else int(x.shape[1])
    n = int(w.shape[0]) if w is not None else 0
    m = rows if M is None else int(M)
    s = int(splitk)
    a, keep = _TallArgs(), _Keep()
    a.op, a.M, a.rows, a.N, a.K, a.epi, a.splitk, a.form = TALL_OPS[op], m, rows, n, k, int(epi), s, int(form)
    a.want_x_out, a.want_y_out = (1 if want_x_out else 0), (1 if want_y_out else 0)
    a.launched_cap = 256
    a.x, a.W, a.bias, a.pbias = keep.f32(x), keep.f32(w), keep.f32(bias), keep.f32(pbias)
    res = {"out": None, "ch": None, "cl": None, "x_out": None, "y_out": None, "yh": None, "yl": None}
    if prep:
        a.ldx = x.shape[1]
        a.ldy = k if ldy is None else int(ldy)
        if ln is not None:
            a.ln_w, a.ln_b, a.eps = keep.f32(ln[0]), keep.f32(ln[1]), float(ln[2])
        if planes is not None:
            planes = _f32(planes)
            a.psplit, a.pstride = planes.shape[0], planes.size // max(planes.shape[0], 1)
        a.planes = keep.f32(planes)
        res["x_out"], res["y_out"] = np.empty((rows, k), np.float32), np.empty((rows, k), np.float32)
        res["yh"], res["yl"] = np.empty((rows, max(int(a.ldy), 0)), np.uint16), np.empty((rows, max(int(a.ldy), 0)), np.uint16)
        a.x_out, a.y_out, a.yh, a.yl = keep.f32(res["x_out"]), keep.f32(res["y_out"]), keep.u16(res["yh"]), keep.u16(res["yl"])
    if prod:
        a.lda = int(lda) if lda is not None else (int(a.ldy) if prep else x.shape[1])
        if residual is not None:
            residual = _f32(residual)
            a.ldr = residual.shape[1]
        a.R = keep.f32(residual)
        a.ldc, a.ldp = (n if ldc is None else int(ldc)), (n if ldp is None else int(ldp))
        a.zstride = rows * n if zstride is None else int(zstride)
        if s > 1 or not out_planes:
            res["out"] = np.empty((s, max(int(a.zstride), 0)) if s > 1 else (rows, max(int(a.ldc), 0)), np.float32)
        if out_planes:
            res["ch"], res["cl"] = np.empty((rows, max(int(a.ldp), 0)), np.uint16), np.empty((rows, max(int(a.ldp), 0)), np.uint16)
        a.out, a.ch, a.cl = keep.f32(res["out"]), keep.u16(res["ch"]), keep.u16(res["cl"])
    fo, grid, launched = (C.c_int32 * 1)(), (C.c_int32 * 3)(), C.create_string_buffer(256)
    a.form_out, a.grid, a.launched = C.cast(fo, _I32P), C.cast(grid, _I32P), C.cast(launched, C.c_char_p)
    rc = hooks().ptts_debug_tall(C.byref(a))
    res.update(form=int(fo[0]), grid=tuple(int(g) for g in grid), launched=_census_dict(launched))
    try:
        _check(rc)
    except PttsError as e:
        e.partial = res
        raise
    return res


def _bf16_bits_f32(u):
    return (np.ascontiguousarray(u, np.uint16).astype(np.uint32) << 16).view(np.float32)


def debug_tall_linear(x, w, *, bias=None, residual=None, epi=0, splitk=1, ln=None, planes=None, pbias=None, out_planes=False):
    """debug_tall in its first form: `ln` = (weight, bias, eps) sends the rows through k_rowprep (with `planes` [psplit, M, K] and `pbias` summed in first),
    then k_tall as production launches it; returns (out [splitk or 1, M, N] squeezed -- hi + lo with out_planes --, updated rows or None)."""
    x, w = _f32(x), _f32(w)
    m = x.shape[0]
    n = w.shape[0]
    s = max(1, int(splitk))
    pend = ln is not None and planes is not None
    r = debug_tall("both" if ln is not None else "tall", x, w=w, bias=bias, residual=residual, epi=epi, splitk=s, ln=ln, planes=planes if pend else None,
                   pbias=pbias if pend else None, out_planes=bool(out_planes) and s == 1)
    if out_planes and s == 1:
        out = _bf16_bits_f32(r["ch"]) + _bf16_bits_f32(r["cl"])
    else:
        out = r["out"].reshape((s, m, n) if s > 1 else (m, n))
    return out, (r["x_out"] if pend else None)


class _FlowClusterArgs(C.Structure):   # ptts_flow_cluster_args
    _fields_ = ([(n, C.c_int32) for n in ("rows", "depth", "n_launch", "in_place")] + [("tag_base0", C.c_uint32), ("reserved", C.c_int32)] +
                [(n, C.c_int64) for n in ("ldmod", "launched_cap")] +
                [(n, _FP) for n in ("fx", "ada", "ln_w", "ln_b", "b0", "b2", "eps", "w0", "w2")] +
                [("launch_rows", C.POINTER(C.c_int32)), ("out", _FP), ("fx_back", _FP), ("state", C.POINTER(C.c_uint32)), ("launched", C.c_char_p)])


FLOW_CLUSTER_TILES, FLOW_CLUSTER_TILE_ROWS = 22, 12


def debug_flow_cluster(fx, ada, ln_w, ln_b, w0, b0, w2, b2, eps, *, launch_rows=None, in_place=True, tag_base0=0, null=()):
    """k_flow_cluster (csrc/flow_cluster.hip) on host operands (ptts_debug_flow_cluster, include/ptts_debug.h): the launches `launch_rows` (default: one of
    all rows) one after another on one granule buffer and one set of tag words starting at tag_base0.  fx [rows, 512], ada [rows, ldmod], ln_w / ln_b / b0 /
    b2 [depth, 512], w0 / w2 [depth, 512, 512] f32, eps [depth].  Returns a dict: "out" [n_launch, rows, 512] (0xff bytes where nothing was stored), "fx_back"
    (out of place: the launches' input copies afterwards, else None), "tags" (the 22 tiles' tag words), "fault" (the fault word), "launched" ({kernel:
    count}).  A set fault word raises PttsError (PTTS_ENODEVICE) with the same dict as its `partial` attribute.  null: names of ptts_flow_cluster_args
    pointers to pass as NULL (the refusal tests)."""
    fx, ada, ln_w, ln_b, w0, b0, w2, b2 = [_f32(a) for a in (fx, ada, ln_w, ln_b, w0, b0, w2, b2)]
    eps = np.ascontiguousarray(np.atleast_1d(np.asarray(eps, np.float32)))
    depth = int(eps.shape[0])
    if (fx.ndim != 2 or fx.shape[1] != 512 or ada.ndim != 2 or ada.shape[0] != fx.shape[0] or eps.ndim != 1 or
            any(a.shape != (depth, 512) for a in (ln_w, ln_b, b0, b2)) or any(a.shape != (depth, 512, 512) for a in (w0, w2))):
        raise PttsError(PTTS_EINVAL, "debug_flow_cluster: operand shapes do not fit (include/ptts_debug.h ptts_flow_cluster_args)")
    rows = fx.shape[0]
    lr = np.ascontiguousarray([rows] if launch_rows is None else launch_rows, np.int32).reshape(-1)
    n = int(lr.shape[0])
    out = np.empty((n, rows, 512), np.float32)
    back = None if in_place else np.empty((n, rows, 512), np.float32)
    state = np.zeros(FLOW_CLUSTER_TILES + 1, np.uint32)
    launched = C.create_string_buffer(256)
    a, keep = _FlowClusterArgs(), _Keep()
    a.rows, a.depth, a.n_launch, a.in_place, a.tag_base0 = rows, depth, n, (1 if in_place else 0), int(tag_base0)
    a.ldmod, a.launched_cap = ada.shape[1], 256
    a.fx, a.ada, a.ln_w, a.ln_b, a.b0, a.b2, a.eps, a.w0, a.w2 = [keep.f32(x) for x in (fx, ada, ln_w, ln_b, b0, b2, eps, w0, w2)]
    a.launch_rows = keep.i32(lr)
    a.out, a.fx_back = keep.f32(out), keep.f32(back)
    a.state = C.cast(state.ctypes.data, C.POINTER(C.c_uint32))
    a.launched = C.cast(launched, C.c_char_p)
    for name in null:
        setattr(a, name, C.cast(None, dict(_FlowClusterArgs._fields_)[name]))
    rc = hooks().ptts_debug_flow_cluster(C.byref(a))
    res = {"out": out, "fx_back": back, "tags": state[:FLOW_CLUSTER_TILES].copy(), "fault": int(state[FLOW_CLUSTER_TILES]), "launched": _census_dict(launched)}
    try:
        _check(rc)
    except PttsError as e:
        e.partial = res
        raise
    return res


class _StepLinearArgs(C.Structure):   # ptts_step_linear_args
    _fields_ = ([(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldc", "wfmt", "epi", "splitk", "tail", "path", "ldg", "ln", "ldmod", "psplit", "r_in_c", "zrows",
                                          "pgate", "reserved")] +
                [("alpha", C.c_float), ("eps", C.c_float)] +
                [(n, _FP) for n in ("x", "W", "bias", "addvec", "R", "scale", "gate", "ln_w", "ln_b", "shift", "mscale", "planes", "pbias",
                                    "C", "tail_out", "x_out", "y_out", "w_eff", "w_scale")] +
                [("launches", C.POINTER(C.c_int32))])


def debug_step_linear(x, w, *, wfmt=0, bias=None, addvec=None, residual=None, inplace=False, scale=None, gate=None, alpha=1.0, epi=0, tail=False,
                      ldc=None, splitk=1, zrows=0, ln=False, ln_wb=None, eps=1e-5, shift=None, mscale=None, planes=None, pbias=None, pgate=False, path=0):
    """The step linear (csrc/skinny.hip) on host operands (ptts_debug_step_linear, include/ptts_debug.h).  x [M, lda] (K columns are multiplied: default
    lda), w [N, K] f32; wfmt 0 f32 / 1 bf16 / 2 int8; residual [M, ldc] (inplace: the kernel runs with R == C), gate [M, ldg]; ln_wb = (weight, bias);
    shift / mscale [M, ldmod]; planes [psplit, M, K]; path 0: launch_skinny, 1: launch_gemm.  Returns a dict: "out" ([M, ldc], or the planes
    [splitk, zrows or M, N]), "tail", "x_out", "y_out" (whole buffers: NaN where nothing was stored), "w_eff" / "w_scale" (int8), "k_skinny" / "launches"
    (the census of the call)."""
    x, w = _f32(x), _f32(w)
    m, lda = x.shape
    n, k = w.shape
    ldc = n if ldc is None else int(ldc)
    s = max(1, int(splitk))
    a, keep = _StepLinearArgs(), _Keep()
    ptr = keep.f32
    a.M, a.N, a.K, a.lda, a.ldc, a.wfmt, a.epi, a.splitk, a.tail, a.path = m, n, k, lda, ldc, int(wfmt), int(epi), s, 1 if tail else 0, int(path)
    a.ldg = 0 if gate is None else int(np.asarray(gate).shape[1])
    a.ln = 1 if ln else 0
    mod = shift if shift is not None else mscale
    a.ldmod = 0 if mod is None else int(np.asarray(mod).shape[1])
    a.psplit = 0 if planes is None else int(np.asarray(planes).shape[0])
    a.r_in_c, a.zrows, a.pgate = (1 if inplace else 0), int(zrows), (1 if pgate else 0)
    a.alpha, a.eps = float(alpha), float(eps)
    a.x, a.W, a.bias, a.addvec, a.R, a.scale, a.gate = ptr(x), ptr(w), ptr(bias), ptr(addvec), ptr(residual), ptr(scale), ptr(gate)
    a.ln_w, a.ln_b = (ptr(ln_wb[0]), ptr(ln_wb[1])) if ln_wb is not None else (ptr(None), ptr(None))
    a.shift, a.mscale, a.planes, a.pbias = ptr(shift), ptr(mscale), ptr(planes), ptr(pbias)
    out = np.empty((s, int(zrows) or m, n) if s > 1 else (m, ldc), np.float32)
    tl = np.empty(m, np.float32)
    fused = bool(ln or planes is not None or shift is not None or mscale is not None or ln_wb is not None or pgate)
    xo = np.empty((m, k), np.float32) if fused else None
    yo = np.empty((m, k), np.float32) if fused else None
    we = np.empty((n, k), np.float32) if int(wfmt) == 2 else None
    ws = np.empty(n, np.float32) if int(wfmt) == 2 else None
    cnt = (C.c_int32 * 2)()
    a.C, a.tail_out, a.x_out, a.y_out, a.w_eff, a.w_scale = ptr(out), ptr(tl), ptr(xo), ptr(yo), ptr(we), ptr(ws)
    a.launches = C.cast(cnt, _I32P)
    _check(hooks().ptts_debug_step_linear(C.byref(a)))
    return {"out": out, "tail": tl if tail else None, "x_out": xo, "y_out": yo, "w_eff": we, "w_scale": ws, "k_skinny": int(cnt[0]), "launches": int(cnt[1])}


STEP_EDGE_OPS = {"begin": 0, "begin_lin": 1, "finish": 2, "fin": 3, "fin_chain": 4}   # PTTS_STEP_EDGE_*
STEP_STATE_I32 = ("kv_len", "active", "step", "countdown", "n_frames", "eos_step", "max_steps", "frames_after_eos", "broke")   # kernels.h StepState, [rows] each


class _StepEdgeArgs(C.Structure):   # ptts_step_edge_args
    _fields_ = ([(n, C.c_int32) for n in ("op", "B", "rows", "S", "ldim", "d_in", "d_pj", "lin_bf16", "N", "K", "wfmt", "epi", "ldmod", "reserved")] +
                [("alpha", C.c_float), ("eps", C.c_float)] +
                [(n, C.c_int64) for n in ("lat_stride", "noise_stride", "launched_cap")] +
                [(n, _I32P) for n in STEP_STATE_I32 + ("n_active",)] +
                [(n, _FP) for n in ("eos_threshold", "latents", "noise", "bos", "eos_logit", "frame")] +
                [("w_in", C.c_void_p), ("w_pj", C.c_void_p)] +
                [(n, _FP) for n in ("b_in", "b_pj", "fx_in", "W", "bias", "shift", "mscale", "cur", "in32", "x0", "x", "fx", "w_eff", "w_scale")] +
                [("launched", C.c_char_p)])


def debug_step_edge(op, state, latents, bos, *, B=None, S=None, noise=None, eos_logit=None, frame=None, lin=None, final=None, null=()):
    """The opening and closing of an AR step on host operands (ptts_debug_step_edge, include/ptts_debug.h): ONE launcher call.  op: a key of STEP_EDGE_OPS.
    state: {name: [rows] int32 for name in STEP_STATE_I32, "eos_threshold": [rows] f32, "n_active": int}; latents [rows, lat_stride] (S frames of ldim =
    len(bos) per row: default lat_stride // ldim); noise [rows, noise_stride] or None; B rows are launched (default: all).  lin = dict(w_in [d_in, ldim],
    w_pj [d_pj, ldim], b_in, b_pj): f32 arrays, or uint16 arrays of bf16 bits.  final = dict(fx [rows, K], W [N, K], bias, shift, mscale [rows, ldmod],
    cur [rows, N], wfmt, alpha, eps, epi).  Nothing passed in is modified.  Returns a dict: "state" (as above, after the launch), "latents", "cur" (whole,
    after the launch), "in32", "x0", "x", "fx" (whole; 0xff bytes where nothing was stored), "w_eff" / "w_scale" (int8), "launched" ({kernel: count}).
    null: names of ptts_step_edge_args pointers to pass as NULL (the refusal tests)."""
    bos = _f32(bos)
    ldim = int(bos.shape[0])
    lat = np.array(latents, np.float32, order="C")
    rows = int(lat.shape[0])
    st_i = {n: np.array(state[n], np.int32, order="C").reshape(rows) for n in STEP_STATE_I32}
    thr = np.array(state["eos_threshold"], np.float32, order="C").reshape(rows)
    n_act = np.array([int(state["n_active"])], np.int32)
    a, keep = _StepEdgeArgs(), _Keep()
    a.op, a.B, a.rows, a.ldim = STEP_EDGE_OPS[op], rows if B is None else int(B), rows, ldim
    a.S = lat.shape[1] // max(ldim, 1) if S is None else int(S)
    a.lat_stride, a.launched_cap = lat.shape[1], 256
    for n in STEP_STATE_I32:
        setattr(a, n, keep.i32(st_i[n]))
    a.n_active, a.eos_threshold, a.latents, a.bos = keep.i32(n_act), keep.f32(thr), keep.f32(lat), keep.f32(bos)
    if noise is not None:
        noise = _f32(noise)
        a.noise_stride = noise.shape[1]
    a.noise, a.eos_logit, a.frame = keep.f32(noise), keep.f32(eos_logit), keep.f32(frame)
    d_in = d_pj = 0
    if lin is not None:
        ws = [np.ascontiguousarray(lin[k]) for k in ("w_in", "w_pj")]
        a.lin_bf16 = 1 if ws[0].dtype == np.uint16 else 0
        ws = [w if w.dtype == np.uint16 else _f32(w) for w in ws]
        keep.arrays += ws
        d_in, d_pj = int(ws[0].shape[0]), int(ws[1].shape[0])
        a.d_in, a.d_pj, a.w_in, a.w_pj = d_in, d_pj, ws[0].ctypes.data, ws[1].ctypes.data
        a.b_in, a.b_pj = keep.f32(lin.get("b_in")), keep.f32(lin.get("b_pj"))
    cur = we = wsc = None
    if final is not None:
        W = _f32(final["W"])
        a.N, a.K, a.wfmt, a.epi = int(W.shape[0]), int(W.shape[1]), int(final.get("wfmt", 0)), int(final.get("epi", 7))
        a.alpha, a.eps = float(final.get("alpha", 1.0)), float(final.get("eps", 1e-6))
        a.ldmod = int(np.asarray(final["shift"]).shape[1])
        cur = np.array(final["cur"], np.float32, order="C")
        if a.wfmt == 2:
            we, wsc = np.empty(W.shape, np.float32), np.empty(W.shape[0], np.float32)
        a.fx_in, a.W, a.bias, a.shift, a.mscale = keep.f32(final["fx"]), keep.f32(W), keep.f32(final.get("bias")), keep.f32(final["shift"]), keep.f32(final["mscale"])
        a.cur, a.w_eff, a.w_scale = keep.f32(cur), keep.f32(we), keep.f32(wsc)
    in32, x0 = np.empty((rows, ldim), np.float32), np.empty((rows, ldim), np.float32)
    x, fx = (np.empty((rows, d_in), np.float32), np.empty((rows, d_pj), np.float32)) if lin is not None else (None, None)
    a.in32, a.x0, a.x, a.fx = keep.f32(in32), keep.f32(x0), keep.f32(x), keep.f32(fx)
    launched = C.create_string_buffer(256)
    a.launched = C.cast(launched, C.c_char_p)
    for name in null:
        setattr(a, name, C.cast(None, dict(_StepEdgeArgs._fields_)[name]))
    _check(hooks().ptts_debug_step_edge(C.byref(a)))
    out_state = dict(st_i, eos_threshold=thr, n_active=int(n_act[0]))
    return {"state": out_state, "latents": lat, "cur": cur, "in32": in32, "x0": x0, "x": x, "fx": fx, "w_eff": we, "w_scale": wsc, "launched": _census_dict(launched)}


class _AttnStepArgs(C.Structure):   # ptts_attn_step_args
    _fields_ = ([(n, C.c_int32) for n in ("kv_bf16", "heads", "rows", "layers", "layer", "cap", "keys_now", "n_pre")] +
                [(n, C.c_int64) for n in ("qkv_ld", "out_ld", "kernel_cap")] +
                [(n, _FP) for n in ("qkv", "cos_t", "sin_t")] +
                [(n, C.POINTER(C.c_int32)) for n in ("seg_len", "active", "pre_len", "voice_of_row")] +
                [("pre_k", C.c_void_p * 4), ("pre_v", C.c_void_p * 4), ("pre_rows", C.c_int32 * 4), ("k", C.c_void_p), ("v", C.c_void_p), ("out", _FP),
                 ("kernel", C.c_char_p), ("info", C.POINTER(C.c_int32))])


def debug_attn_step(qkv, cos, sin, seg_len, k, v, *, kv_bf16, heads, layers=1, layer=0, keys_now=0, active=None, pre_len=None, voice_of_row=None, pre_k=(),
                    pre_v=(), out_ld=None):
    """The step attention (csrc/attn_step.hip) on host operands (ptts_debug_attn_step, include/ptts_debug.h): one launch_attention call with the AR step's
    arguments.  qkv [rows, qkv_ld]; cos / sin [cap, 32]; k, v [rows, heads, cap, 64] in the cache format (uint16 bf16 bits, or 4-byte elements); pre_k / pre_v:
    up to 4 prefix buffers [layers, heads, len, 64] in the same format, named per row by voice_of_row (-1: none).  Returns a dict: "out" ([rows, out_ld], NaN
    where nothing was stored), "k" / "v" (the caches after the launch, the inputs are not modified), "kernel" (launch_attention's choice), "rounds" (load
    rounds of k_attn_step, 0 for another kernel), "launches", "k_attn_step", "k_attention" (the census of the call)."""
    qkv, cos, sin = _f32(qkv), _f32(cos), _f32(sin)
    rows, qkv_ld = qkv.shape
    cap = cos.shape[0]
    es = 2 if kv_bf16 else 4
    i32 = lambda a, fill: np.ascontiguousarray(np.full(rows, fill, np.int32) if a is None else np.asarray(a, np.int32))   # noqa: E731
    seg_len, active, pre_len, voice_of_row = i32(seg_len, 0), i32(active, 1), i32(pre_len, 0), i32(voice_of_row, -1)
    k, v = np.array(k, order="C", copy=True), np.array(v, order="C", copy=True)
    pre_k, pre_v = [np.ascontiguousarray(p) for p in pre_k], [np.ascontiguousarray(p) for p in pre_v]
    if (cos.shape != (cap, 32) or sin.shape != (cap, 32) or any(a.shape != (rows,) for a in (seg_len, active, pre_len, voice_of_row)) or len(pre_k) != len(pre_v) or
            len(pre_k) > 4 or any(a.itemsize != es or a.shape != (rows, heads, cap, 64) for a in (k, v)) or
            any(a.itemsize != es or a.ndim != 4 or a.shape[:2] != (layers, heads) or a.shape[3] != 64 or a.shape != b.shape for a, b in zip(pre_k, pre_v))):
        raise PttsError(PTTS_EINVAL, "debug_attn_step: operand shapes do not fit (include/ptts_debug.h ptts_attn_step_args)")
    out_ld = heads * 64 if out_ld is None else int(out_ld)
    out = np.empty((rows, max(out_ld, 0)), np.float32)
    name = C.create_string_buffer(64)
    info = (C.c_int32 * 4)()
    a, keep = _AttnStepArgs(), _Keep()
    a.kv_bf16, a.heads, a.rows, a.layers, a.layer, a.cap, a.keys_now, a.n_pre = (1 if kv_bf16 else 0), int(heads), rows, int(layers), int(layer), cap, int(keys_now), len(pre_k)
    a.qkv_ld, a.out_ld, a.kernel_cap = qkv_ld, out_ld, 64
    a.qkv, a.cos_t, a.sin_t = keep.f32(qkv), keep.f32(cos), keep.f32(sin)
    a.seg_len, a.active, a.pre_len, a.voice_of_row = [keep.i32(x) for x in (seg_len, active, pre_len, voice_of_row)]
    for i, (pk, pv) in enumerate(zip(pre_k, pre_v)):
        a.pre_k[i], a.pre_v[i], a.pre_rows[i] = pk.ctypes.data, pv.ctypes.data, pk.shape[2]
    a.k, a.v, a.out = k.ctypes.data, v.ctypes.data, keep.f32(out)
    a.kernel = C.cast(name, C.c_char_p)
    a.info = C.cast(info, _I32P)
    _check(hooks().ptts_debug_attn_step(C.byref(a)))
    return {"out": out, "k": k, "v": v, "kernel": name.value.decode(), "rounds": int(info[0]), "launches": int(info[1]), "k_attn_step": int(info[2]),
            "k_attention": int(info[3])}


def attn_step_rounds(keys: int, kv_bf16: bool):
    """(load rounds of k_attn_step for a launch bounded by `keys`, keys per round): attn_step_rounds / attn_step_keys_per_round of csrc/attn_step.hip.  No GPU."""
    H = hooks()
    H.ptts_debug_attn_step_rounds.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    kpr = C.c_int32()
    return int(H.ptts_debug_attn_step_rounds(int(keys), 1 if kv_bf16 else 0, C.byref(kpr))), int(kpr.value)


class _AttnWindowArgs(C.Structure):   # ptts_attn_window_args
    _fields_ = ([(n, C.c_int32) for n in ("form", "ragged", "kv_bf16", "heads", "segs", "context", "T1", "t0", "CT", "cap", "rows", "reserved")] +
                [(n, C.c_int64) for n in ("ld", "out_ld", "kernel_cap", "launched_cap")] +
                [("qkv", _FP), ("k", C.c_void_p), ("v", C.c_void_p), ("rag_off", C.POINTER(C.c_int32)), ("rag_pos0", C.POINTER(C.c_int32)), ("out", _FP),
                 ("kernel", C.c_char_p), ("launched", C.c_char_p)])


ATTN_WINDOW_DISPATCH, ATTN_WINDOW_WAVE, ATTN_WINDOW_LDS = 0, 1, 2


def debug_attn_window(qkv, *, heads, context, form=0, t0=0, ct=None, k=None, v=None, rag_off=None, rag_pos0=None, kv_bf16=False, out_ld=None):
    """The window attention (csrc/attn_window.hip) on host operands (ptts_debug_attn_window, include/ptts_debug.h): one launch.  Dense: qkv [segs, T1, ld] (q | k |
    v at columns 0, D, 2 D), the chunk (t0, ct) of every segment is launched (ct default: T1 - t0).  Ragged (rag_off given): qkv is the packed query rows
    [rows, ld], k / v the caches [segs, heads, cap, 64] in the cache format (uint16 bf16 bits, or 4-byte elements), rag_off [segs + 1], rag_pos0 [segs].  form 0:
    launch_attention's dispatch, 1: k_attn_window, 2: k_attn_window_lds<4>.  Returns a dict: "out" ([rows, out_ld], 0xff bytes where nothing was stored),
    "kernel" (the dispatch's name, or the instance's), "launched" ({kernel: count})."""
    qkv = _f32(qkv)
    ragged = rag_off is not None
    a, keep = _AttnWindowArgs(), _Keep()
    if ragged:
        es = 2 if kv_bf16 else 4
        k, v = np.ascontiguousarray(k), np.ascontiguousarray(v)
        rag_off, rag_pos0 = np.ascontiguousarray(rag_off, np.int32), np.ascontiguousarray(rag_pos0, np.int32)
        segs = rag_pos0.shape[0] if rag_pos0.ndim == 1 else -1
        if (qkv.ndim != 2 or segs < 1 or rag_off.shape != (segs + 1,) or k.ndim != 4 or k.shape != v.shape or k.shape[:2] != (segs, heads) or k.shape[3] != 64 or
                k.itemsize != es or v.itemsize != es):
            raise PttsError(PTTS_EINVAL, "debug_attn_window: operand shapes do not fit (include/ptts_debug.h ptts_attn_window_args)")
        rows, ld = qkv.shape
        a.cap, a.rows = k.shape[2], rows
        a.k, a.v = k.ctypes.data, v.ctypes.data
        a.rag_off, a.rag_pos0 = keep.i32(rag_off), keep.i32(rag_pos0)
    else:
        if qkv.ndim != 3:
            raise PttsError(PTTS_EINVAL, "debug_attn_window: the dense operand is [segs, T1, ld]")
        segs, t1, ld = qkv.shape
        ct = t1 - int(t0) if ct is None else int(ct)
        a.T1, a.t0, a.CT = t1, int(t0), ct
        rows = max(segs * ct, 0)
    out_ld = heads * 64 if out_ld is None else int(out_ld)
    out = np.empty((rows, max(out_ld, 0)), np.float32)
    name, launched = C.create_string_buffer(64), C.create_string_buffer(256)
    a.form, a.ragged, a.kv_bf16, a.heads, a.segs, a.context = int(form), (1 if ragged else 0), (1 if kv_bf16 else 0), int(heads), segs, int(context)
    a.ld, a.out_ld, a.kernel_cap, a.launched_cap = ld, out_ld, 64, 256
    a.qkv, a.out = keep.f32(qkv), keep.f32(out)
    a.kernel, a.launched = C.cast(name, C.c_char_p), C.cast(launched, C.c_char_p)
    _check(hooks().ptts_debug_attn_window(C.byref(a)))
    return {"out": out, "kernel": name.value.decode(), "launched": _census_dict(launched)}


class _GemmRowsArgs(C.Structure):   # ptts_gemm_rows_args
    _fields_ = ([(n, C.c_int32) for n in ("M", "N", "K", "ldw", "w_bf16", "aop", "epi", "kernel", "cfg", "rgl", "r_in_c", "ldg", "rope_cols", "rope_hd", "rope_pos0",
                                          "rope_rows_per_seg", "n_pos", "kslice", "win_taps", "win_c")] +
                [("alpha", C.c_float), ("reserved", C.c_int32)] +
                [(n, C.c_int64) for n in ("a_elems", "a_ld", "a_rows_per_batch", "a_batch_stride", "a_off", "c_elems", "c_ld", "c_rows_per_batch", "c_batch_stride",
                                          "c_off", "zstride", "launched_cap")] +
                [(n, _FP) for n in ("A", "W", "bias", "addvec", "scale", "gate", "R", "rope_cos", "rope_sin")] +
                [("rope_row_pos", C.POINTER(C.c_int32)), ("C", _FP), ("launched", C.c_char_p), ("info", C.POINTER(C.c_int32))])


GEMM_DISPATCH, GEMM_K_GEMM, GEMM_K_GEMM2, GEMM_K_GEMM3, GEMM_K_WRES, GEMM_K_GEMM5 = 0, 1, 2, 3, 4, 5


def debug_gemm_rows(a_buf, w, M, *, amap, cmap, c_elems, kernel=0, cfg=0, rgl=0, w_bf16=True, K=None, aop=0, epi=0, alpha=1.0, bias=None, addvec=None, scale=None,
                    gate=None, residual=None, inplace=False, rope=None, rope_cols=0, rope_hd=64, rope_pos0=0, rope_rows_per_seg=0, rope_row_pos=None, kslice=0,
                    zstride=0, win_taps=0, win_c=0):
    """ONE launch of a many-row GEMM kernel on host operands (ptts_debug_gemm_rows, include/ptts_debug.h).  a_buf: A's raw buffer (flat f32); w [N, ldw] (K columns
    are multiplied: default ldw); amap / cmap = (ld, rows_per_batch, batch_stride, off) in elements; residual: a flat buffer of c_elems floats addressed like C
    (inplace: the kernel runs with R == C); gate [M, ldg]; rope = (cos, sin) tables [n_pos, rope_hd / 2]; kernel 0 dispatch / 1 k_gemm / 2 k_gemm2 / 3 k_gemm3 /
    4 k_gemm_wres / 5 k_gemm5.  Returns a dict: "out" (the whole C buffer, 0xff bytes where nothing was stored), "launched" ({kernel: count}), "cus", "rgl"."""
    a_buf, w = _f32(a_buf).reshape(-1), _f32(w)
    n, ldw = w.shape
    a, keep = _GemmRowsArgs(), _Keep()
    ptr = keep.f32
    a.M, a.N, a.K, a.ldw, a.w_bf16, a.aop, a.epi = int(M), n, ldw if K is None else int(K), ldw, 1 if w_bf16 else 0, int(aop), int(epi)
    a.kernel, a.cfg, a.rgl, a.r_in_c = int(kernel), int(cfg), int(rgl), 1 if inplace else 0
    a.ldg = 0 if gate is None else int(np.asarray(gate).shape[1])
    a.alpha = float(alpha)
    a.a_elems, a.c_elems = a_buf.size, int(c_elems)
    a.a_ld, a.a_rows_per_batch, a.a_batch_stride, a.a_off = (int(v) for v in amap)
    a.c_ld, a.c_rows_per_batch, a.c_batch_stride, a.c_off = (int(v) for v in cmap)
    a.A, a.W, a.bias, a.addvec, a.scale, a.gate = ptr(a_buf), ptr(w), ptr(bias), ptr(addvec), ptr(scale), ptr(gate)
    if residual is not None:
        residual = _f32(residual).reshape(-1)
        if residual.size != int(c_elems):
            raise ValueError("the residual is addressed like C: c_elems floats")
    a.R = ptr(residual)
    if rope is not None:
        cos, sin = _f32(rope[0]), _f32(rope[1])
        if cos.shape != sin.shape or cos.ndim != 2 or cos.shape[1] * 2 != int(rope_hd):
            raise ValueError("rope tables are [n_pos, rope_hd / 2]")
        a.rope_cos, a.rope_sin, a.n_pos = ptr(cos), ptr(sin), cos.shape[0]
        a.rope_cols, a.rope_hd, a.rope_pos0, a.rope_rows_per_seg = int(rope_cols), int(rope_hd), int(rope_pos0), int(rope_rows_per_seg)
        if rope_row_pos is not None:
            a.rope_row_pos = keep.i32(np.asarray(rope_row_pos, np.int32).reshape(int(M)))
    a.kslice, a.zstride, a.win_taps, a.win_c = int(kslice), int(zstride), int(win_taps), int(win_c)
    out = np.empty(int(c_elems), np.float32)
    a.C = ptr(out)
    name = C.create_string_buffer(512)
    a.launched, a.launched_cap = C.cast(name, C.c_char_p), 512
    info = (C.c_int32 * 2)()
    a.info = C.cast(info, _I32P)
    _check(hooks().ptts_debug_gemm_rows(C.byref(a)))
    return {"out": out, "launched": _census_dict(name), "cus": int(info[0]), "rgl": int(info[1])}


class _MimiFusedArgs(C.Structure):   # ptts_mimi_fused_args
    _fields_ = ([(n, C.c_int32) for n in ("kind", "M", "D", "F", "n_pos", "rope_cols", "pos0", "rows_per_seg", "ls_off", "reserved")] +
                [("eps", C.c_float), ("reserved_f", C.c_float)] +
                [(n, C.c_int64) for n in ("x_elems", "x_ld", "x_rows_per_batch", "x_batch_stride", "x_off", "y_elems", "y_ld", "y_rows_per_batch", "y_batch_stride",
                                          "y_off", "launched_cap")] +
                [(n, _FP) for n in ("x", "ln_w", "ln_b", "w1", "w2", "ls", "rope_cos", "rope_sin", "out")] + [("launched", C.c_char_p)])


MIMI_FFN, MIMI_ROWLIN = 0, 1


def debug_mimi_fused(kind, x_buf, M, *, xmap, ln_w, ln_b, w1, w2=None, eps=1e-5, ls=None, ls_off=0, D=None, F=None, y_elems=0, ymap=(0, 0, 0, 0), rope=None,
                     rope_cols=0, pos0=0, rows_per_seg=0):
    """ONE launch of k_mimi_ffn (kind 0) or k_mimi_rowlin (kind 1) on host operands (ptts_debug_mimi_fused, include/ptts_debug.h).  x_buf: x's raw buffer (flat
    f32); xmap / ymap = (ld, rows_per_batch, batch_stride, off) in elements; w1 [F or N, D], w2 [D, F] f32 row-major (rounded to bf16 by the packers); ls [D] or
    None; rope = (cos, sin) tables [n_pos, 32].  D / F override the widths taken from w1's shape (for refusals).  Returns a dict: "out" (kind 0: the whole x buffer
    after the in-place launch; kind 1: the whole y buffer, 0xff bytes where nothing was stored), "launched" ({kernel: count})."""
    x_buf, w1 = _f32(x_buf).reshape(-1), _f32(w1)
    a, keep = _MimiFusedArgs(), _Keep()
    ptr = keep.f32
    a.kind, a.M, a.D, a.F = int(kind), int(M), int(w1.shape[1] if D is None else D), int(w1.shape[0] if F is None else F)
    a.eps, a.ls_off = float(eps), int(ls_off)
    a.x_elems = x_buf.size
    a.x_ld, a.x_rows_per_batch, a.x_batch_stride, a.x_off = (int(v) for v in xmap)
    a.y_elems = int(y_elems)
    a.y_ld, a.y_rows_per_batch, a.y_batch_stride, a.y_off = (int(v) for v in ymap)
    a.x, a.ln_w, a.ln_b, a.w1, a.w2, a.ls = ptr(x_buf), ptr(ln_w), ptr(ln_b), ptr(w1), ptr(w2), ptr(ls)
    if rope is not None:
        cos, sin = (None if t is None else _f32(t) for t in rope)
        a.rope_cos, a.rope_sin = ptr(cos), ptr(sin)
        a.n_pos = (cos if cos is not None else sin).shape[0]
        a.rope_cols, a.pos0, a.rows_per_seg = int(rope_cols), int(pos0), int(rows_per_seg)
    out = np.empty(x_buf.size if int(kind) == 0 else max(int(y_elems), 1), np.float32)
    a.out = ptr(out)
    name = C.create_string_buffer(512)
    a.launched, a.launched_cap = C.cast(name, C.c_char_p), 512
    _check(hooks().ptts_debug_mimi_fused(C.byref(a)))
    return {"out": out, "launched": _census_dict(name)}


def debug_mimi_pack(kind, w1, w2=None):
    """The weight-image packers of csrc/ffn_fused.hip's kernels (csrc/model.h) on matrices: kind 0 w1 [F, 512] + w2 [512, F] -> uint16 [F / 32, 2, 16384] (per
    chunk the W1 image, then the W2 image); kind 1 w1 [N, 512] -> uint16 [N / 32, 16384].  No GPU."""
    w1 = _f32(w1)
    n = w1.shape[0]
    if w1.ndim != 2 or w1.shape[1] != 512 or (kind == 0 and (w2 is None or tuple(np.shape(w2)) != (512, n))):
        raise ValueError("w1 is [n, 512], w2 [512, n]")
    w2 = None if kind != 0 else _f32(w2)
    dst = np.empty(n * (1024 if kind == 0 else 512), np.uint16)
    H = hooks()
    H.ptts_debug_mimi_pack.argtypes = [C.c_int32, _FP, _FP, C.c_int32, C.c_void_p]
    _check(H.ptts_debug_mimi_pack(int(kind), _fp(w1), C.cast(None, _FP) if w2 is None else _fp(w2), n, dst.ctypes.data_as(C.c_void_p)))
    return dst.reshape((n // 32, 2, 16384) if kind == 0 else (n // 32, 16384))


class _ResblockArgs(C.Structure):   # ptts_resblock_args
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "t0", "t1", "C", "H", "pad", "slack", "w_bf16", "final_conv", "form", "grid", "fuse_up", "x_pad", "x_L", "x_slack")] +
                [(n, _FP) for n in ("u", "w1", "w2", "wf", "b1", "b2", "bf", "xin", "wup", "bup")] +
                [("rows", C.POINTER(C.c_int32)), ("uo", _FP), ("pcm", _FP), ("row_out", C.c_void_p), ("row_bytes", C.c_int64), ("launched", C.POINTER(C.c_int32))])


RES_FORM_AUTO, RES_FORM_TILE, RES_FORM_PERS = 0, 1, 2


def debug_resblock(u, w1, w2, *, L=None, pad=2, slack=0, t0=0, t1=None, w_bf16=True, wf=None, b1=None, b2=None, bf=None, rows=None, row_bytes=None,
                   form=RES_FORM_AUTO, grid=0, xin=None, wup=None, bup=None, x_pad=1, x_slack=0):
    """ONE launch of a fused SEANet block (csrc/resblock.hip, csrc/resblock_up.hip) on host operands (ptts_debug_resblock, include/ptts_debug.h).
    u [B, pad + L, C] (None with xin: the fused form makes it from xin [B, x_pad + L / 4, 128], wup [256, 256], bup [64]); w1 [H, 3 C], w2 [C, H]; wf [3 C]
    asks for the final convolution; rows: [(lim, s16)] per utterance asks for row destinations of row_bytes bytes each; form 0 automatic / 1 one tile per
    block / 2 `grid` persistent blocks.  Returns a dict: "uo" [B, pad + L + slack, C] or "pcm" [B, L] and "rows" [B, row_bytes] uint8 (whole buffers, 0xff
    bytes where nothing was stored), "plan": (waves per block, persistent, grid, tiles per utterance, new rows per tile)."""
    w1, w2 = _f32(w1), _f32(w2)
    h, c = w1.shape[0], w2.shape[0]
    a, keep = _ResblockArgs(), _Keep()
    ptr = keep.f32
    fused = xin is not None
    if fused:
        xin = _f32(xin)
        b, xl = xin.shape[0], xin.shape[1] - int(x_pad)
        L = 4 * xl if L is None else int(L)
    else:
        u = _f32(u)
        b = u.shape[0]
        L = u.shape[1] - int(pad) if L is None else int(L)
        xl = 0
    a.B, a.L, a.t0, a.t1, a.C, a.H, a.pad, a.slack = b, L, int(t0), L if t1 is None else int(t1), c, h, int(pad), int(slack)
    a.w_bf16, a.final_conv, a.form, a.grid, a.fuse_up, a.x_pad, a.x_L, a.x_slack = (1 if w_bf16 else 0), (1 if wf is not None else 0), int(form), int(grid), (1 if fused else 0), int(x_pad), xl, int(x_slack)
    a.u, a.w1, a.w2, a.wf, a.b1, a.b2, a.bf, a.xin, a.wup, a.bup = ptr(None if fused else u), ptr(w1), ptr(w2), ptr(wf), ptr(b1), ptr(b2), ptr(bf), ptr(xin), ptr(wup), ptr(bup)
    final = wf is not None
    uo = None if final else np.empty((b, int(pad) + L + int(slack), c), np.float32)
    pcm = np.empty((b, L), np.float32) if final else None
    a.uo, a.pcm = ptr(uo), ptr(pcm)
    ro = None
    if rows is not None:
        a.rows = keep.i32(np.asarray(rows, np.int32).reshape(b, 2))
        a.row_bytes = ((4 * L + 8 * 4 + 15) // 16) * 16 if row_bytes is None else int(row_bytes)
        ro = np.empty((b, max(int(a.row_bytes), 0)), np.uint8)
        a.row_out = ro.ctypes.data_as(C.c_void_p)
    cnt = (C.c_int32 * 5)()
    a.launched = C.cast(cnt, _I32P)
    _check(hooks().ptts_debug_resblock(C.byref(a)))
    return {"uo": uo, "pcm": pcm, "rows": ro, "plan": tuple(int(v) for v in cnt)}


def debug_resblock_plan(c, final_conv, w_bf16, batch, rows, cus, *, fuse_up=False, form=RES_FORM_AUTO, grid=0):
    """(waves per block, persistent, grid, tiles per utterance, new rows per tile) as resblock_plan / resblock_up_plan choose for `cus` compute units.  No GPU."""
    out = (C.c_int32 * 5)()
    H = hooks()
    H.ptts_debug_resblock_plan.argtypes = [C.c_int32] * 9 + [C.POINTER(C.c_int32)]
    _check(H.ptts_debug_resblock_plan(int(c), 1 if final_conv else 0, 1 if w_bf16 else 0, 1 if fuse_up else 0, int(batch), int(rows), int(form), int(grid), int(cus), out))
    return tuple(int(v) for v in out)


def debug_seanet_pack(kind, rm, want_lo=True):
    """The SEANet blocks' weight packers (csrc/model.h) on a matrix: kind 0 frag16 of rm [out, in], 1 the fused transposed convolution's [256, in], 2 the
    final convolution rm [in].  Returns (hi, lo) uint16 planes (lo None when not asked for).  No GPU."""
    rm = _f32(rm)
    out, inn = (16, rm.shape[0]) if kind == 2 else rm.shape
    hi = np.empty(out * inn, np.uint16)
    lo = np.empty(out * inn, np.uint16) if (want_lo or kind == 2) else None
    H = hooks()
    H.ptts_debug_seanet_pack.argtypes = [C.c_int32, _FP, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    _check(H.ptts_debug_seanet_pack(int(kind), _fp(rm), 1 if kind == 2 else out, inn, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p) if lo is not None else None))
    return hi, lo


def debug_plan_seanet_frags(plan, item):
    """What the loader packed for a plan (Model.plan): (hi, lo or None, (out, in)) of item 0-2 conv k3, 3-5 conv k1, 6 last transposed convolution, 7 final
    convolution; None when the loader made no fragment-ordered copy of it.  No GPU."""
    H = hooks()
    H.ptts_debug_plan_seanet_frags.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    n, dims = C.c_int64(0), (C.c_int32 * 3)()
    _check(H.ptts_debug_plan_seanet_frags(plan, int(item), None, None, 0, C.byref(n), dims))
    if n.value == 0:
        return None
    hi = np.empty(n.value, np.uint16)
    lo = np.empty(n.value, np.uint16) if dims[2] else None
    _check(H.ptts_debug_plan_seanet_frags(plan, int(item), hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p) if lo is not None else None, n.value, C.byref(n), dims))
    return hi, lo, (int(dims[0]), int(dims[1]))


def last_attention_kernel() -> str:
    """Which kernel this thread's last attention launch used (ptts_debug_last_attention_kernel)."""
    return hooks().ptts_debug_last_attention_kernel().decode()


def mimi_encode_frames(n_samples: int) -> int:
    """Frames the Mimi encoder makes of n samples: ceil(n / 1920) (ptts_mimi_encode_frames)."""
    L = lib()
    L.ptts_mimi_encode_frames.argtypes = [C.c_int64]
    L.ptts_mimi_encode_frames.restype = C.c_int64
    return int(L.ptts_mimi_encode_frames(int(n_samples)))


def resample_launches(reset: bool = True) -> int:
    """k_resample launches of the whole process, every thread (ptts_debug_resample_launches); reset: start counting again from 0."""
    H = hooks()
    H.ptts_debug_resample_launches.restype = C.c_int64
    H.ptts_debug_resample_launches.argtypes = [C.c_int32]
    return int(H.ptts_debug_resample_launches(1 if reset else 0))


def launch_counts(on: bool) -> dict:
    """Kernel launches noted on this thread since the previous call ({kernel: count}); switches the census on / off."""
    buf = C.create_string_buffer(4096)
    hooks().ptts_debug_launch_counts(1 if on else 0, buf, 4096)
    return _census_dict(buf)


def op_conv1d_leftpad(x, w, bias=None) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    b, cin, ln = x.shape
    cout, _, k = w.shape
    y = np.empty((b, cout, ln), np.float32)
    ba = _f32(bias) if bias is not None else None
    _check(lib().ptts_op_conv1d_leftpad(_fp(x), _fp(w), _fp(ba), b, cin, ln, cout, k, _fp(y)))
    return y


def op_convtr1d_righttrim(x, w, bias, stride: int, groups: int = 1) -> np.ndarray:
    x, w = _f32(x), _f32(w)
    b, cin, ln = x.shape
    _, opg, k = w.shape
    y = np.empty((b, opg * groups, ln * stride), np.float32)
    ba = _f32(bias) if bias is not None else None
    _check(lib().ptts_op_convtr1d_righttrim(_fp(x), _fp(w), _fp(ba), b, cin, ln, opg, k, stride, groups, _fp(y)))
    return y


def wav_header_streaming() -> bytes:
    """audio.WriteWAVHeaderStreaming (internal/audio/wav_stream.go:15-41): the 44 bytes in front of a PCM16 stream."""
    buf = (C.c_uint8 * 44)()
    lib().ptts_wav_header_streaming(buf)
    return bytes(buf)


def _pcm_format(cfg) -> int:
    g = getattr(cfg, "g711", "") or ""
    if g:
        if g not in ("ulaw", "alaw"):
            raise PttsError(PTTS_EINVAL, f'g711 must be "ulaw" or "alaw", got {g!r}')
        return PCM_ULAW if g == "ulaw" else PCM_ALAW
    return PCM_S16 if getattr(cfg, "pcm16", False) else PCM_F32


def _rates(sample_rate, n: int) -> np.ndarray:
    r = np.asarray(sample_rate, np.int32).reshape(-1)
    return np.ascontiguousarray(np.broadcast_to(r, (max(n, 1),)) if r.size == 1 else r, np.int32)


def resample_length(n_in: int, in_rate: int, out_rate: int) -> int:
    """ptts_resample_length (no GPU): ceil(n_in L / M); < 0 (-PTTS_EINVAL) for a bad rate or pair."""
    return int(lib().ptts_resample_length(int(n_in), int(in_rate), int(out_rate)))


def wav_header(sample_rate: int = 24000, pcm_format: int = PCM_S16, n_samples: int = -1) -> bytes:
    """ptts_wav_header: the WAV header of n_samples mono samples (< 0: a streaming header) in pcm_format at sample_rate."""
    buf = (C.c_uint8 * 64)()
    n = lib().ptts_wav_header(buf, 64, int(sample_rate), int(pcm_format), int(n_samples))
    if n < 0:
        raise PttsError(-n, lib().ptts_last_error().decode(errors="replace"))
    return bytes(buf[:n])


def op_pcm16(samples) -> np.ndarray:
    """audio.WritePCM16Samples on the device."""
    x = np.ascontiguousarray(samples, np.float32).reshape(-1)
    out = np.zeros(x.size, np.int16)
    L = lib()
    L.ptts_op_pcm16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    _check(L.ptts_op_pcm16(x.ctypes.data, x.size, out.ctypes.data))
    return out


class _DispatchOpts(C.Structure):
    _fields_ = [("max_batch", C.c_int32), ("window_us", C.c_int32), ("queue_cap", C.c_int32), ("continuous", C.c_int32), ("cont_kv_capacity", C.c_int32),
                ("cont_max_steps", C.c_int32), ("cont_steps_per_group", C.c_int32), ("reserved", C.c_int32 * 1)]


class _DispatchStats(C.Structure):
    _fields_ = [("requests", C.c_int64), ("batches", C.c_int64), ("cancelled_waiting", C.c_int64), ("max_queue_depth", C.c_int64),
                ("mean_batch", C.c_double), ("mean_wait_us", C.c_double), ("mean_exec_us", C.c_double), ("cont_steps", C.c_int64), ("cont_slot_steps", C.c_int64), ("flow_cluster_fallbacks", C.c_int64)]


DISPATCH_EXEC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(_Request), C.c_int32, C.POINTER(_Result), C.c_void_p, C.c_int32)


class Dispatcher:
    """The serving front of the runtime: `generate` blocks like Synthesize behind the reference's worker
    semaphore (internal/server/server.go:398-421); concurrent callers are coalesced into batched GenerateAudio passes."""

    def __init__(self, models: Sequence[Model], max_batch: int = 0, window_us: int = 2000, queue_cap: int = 0, _custom_exec=None, _workers: int = 1,
                 continuous: Optional[bool] = None, cont_kv_capacity: int = 0, cont_max_steps: int = 0, cont_steps_per_group: int = 0):
        L = lib()
        L.ptts_dispatcher_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(_DispatchOpts), C.POINTER(C.c_void_p)]
        L.ptts_dispatcher_create_custom.argtypes = [DISPATCH_EXEC, C.c_void_p, C.c_int32, C.POINTER(_DispatchOpts), C.POINTER(C.c_void_p)]
        L.ptts_dispatch_generate.argtypes = [C.c_void_p, C.POINTER(_Request), C.POINTER(_Result)]
        L.ptts_dispatcher_stats.argtypes = [C.c_void_p, C.POINTER(_DispatchStats)]
        L.ptts_dispatcher_close.argtypes = [C.c_void_p]
        o = _DispatchOpts(max_batch=max_batch, window_us=window_us, queue_cap=queue_cap, continuous=0 if continuous is None else (1 if continuous else -1), cont_kv_capacity=cont_kv_capacity,
                          cont_max_steps=cont_max_steps, cont_steps_per_group=cont_steps_per_group)
        h = C.c_void_p()
        self.models = list(models)
        if _custom_exec is not None:
            self._exec = DISPATCH_EXEC(_custom_exec)   # kept alive with the dispatcher
            _check(L.ptts_dispatcher_create_custom(self._exec, None, _workers, C.byref(o), C.byref(h)))
        else:
            arr = (C.c_void_p * len(self.models))(*[m.h for m in self.models])
            _check(L.ptts_dispatcher_create(arr, len(self.models), C.byref(o), C.byref(h)))
        self.h = h.value

    def generate(self, tokens: Sequence[int], cfg: RuntimeGenerateConfig) -> GenerateResult:
        """Blocking; safe to call from many threads (the GIL is released while waiting)."""
        req, res, keep = _Request(), _Result(), []
        m = self.models[0] if self.models else None
        if m is not None:
            m._fill_request(req, tokens, cfg, keep)
        else:   # custom executor (tests): only what the queueing logic looks at
            t = np.ascontiguousarray(tokens, np.int64)
            keep.append(t)
            req.tokens, req.n_tokens = _ip(t), t.size
            if cfg.cancel is not None:
                req.cancel = cfg.cancel.ctypes.data_as(C.POINTER(C.c_int32))
        rc = lib().ptts_dispatch_generate(self.h, C.byref(req), C.byref(res))
        try:
            _check(rc)
            if m is None:
                return GenerateResult(np.zeros(0, np.float32), int(res.n_frames), int(res.eos_step), None)
            return m._take_result(res, cfg)
        finally:
            lib().ptts_free_result(C.byref(res))

    def stats(self) -> dict:
        s = _DispatchStats()
        lib().ptts_dispatcher_stats(self.h, C.byref(s))
        return {n: getattr(s, n) for n, _ in _DispatchStats._fields_ if n != "reserved"}

    def close(self):
        if self.h:
            lib().ptts_dispatcher_close(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        self.close()


# ---- text front end (internal/text/prepare.go) ---------------------------------------------------------
def _join_in(parts):
    """A list of arrays as the parts of a join: (rows, n, their pointer array, their lengths as int64)."""
    rows = [_f32(r).reshape(-1) for r in parts]
    return rows, len(rows), _row_ptrs(rows), np.array([r.size for r in rows] or [0], np.int64)


def join_length(lengths, join: Optional[JoinOpts] = None, offsets: bool = False):
    """ptts_join_length: the joined length of parts of these lengths at 24 kHz (offsets: and where each part's first sample lies).  Host."""
    ns = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    offs = np.zeros(max(ns.size, 1), np.int64)
    o = join if join is not None else JoinOpts()
    total = int(lib().ptts_join_length(_ip(ns) if ns.size else None, ns.size, C.byref(o), _ip(offs)))
    if total < 0:
        _check(-total)
    return (total, offs[:ns.size]) if offsets else total


def dsp_windows(model, x, cuts, opts: Optional[DspOpts] = None):
    """Model.dsp_windows: the causal chain over rows in windows with carried state (the hook ptts_debug_dsp_windows)."""
    return model.dsp_windows(x, cuts, opts)


def join_stream_ready(join: Optional[JoinOpts], joined: int) -> int:
    """ptts_join_stream_ready: the samples of the joined 24 kHz audio that are final once `joined` have been joined and more parts follow.  No GPU."""
    o = join if join is not None else JoinOpts()
    rc = int(lib().ptts_join_stream_ready(C.byref(o), int(joined)))
    if rc < 0:
        _check(-rc)
    return rc


def join_parts_length(lengths, parts_opts, join: Optional[JoinOpts] = None, offsets: bool = False):
    """ptts_join_parts_length: join_length with the seam behind every part taken from its PartOpts.  Host."""
    ns = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    offs = np.zeros(max(ns.size, 1), np.int64)
    o = join if join is not None else JoinOpts()
    total = int(lib().ptts_join_parts_length(_ip(ns) if ns.size else None, ns.size, C.byref(o), _part_list(parts_opts), _ip(offs)))
    if total < 0:
        _check(-total)
    return (total, offs[:ns.size]) if offsets else total


def join_parts_stream_ready(join: Optional[JoinOpts], last: PartOpts, joined: int) -> int:
    """ptts_join_parts_stream_ready: join_stream_ready with the crossfade of the seam behind the part `last` describes.  No GPU."""
    o = join if join is not None else JoinOpts()
    rc = int(lib().ptts_join_parts_stream_ready(C.byref(o), C.byref(last), int(joined)))
    if rc < 0:
        _check(-rc)
    return rc


def join_parts(parts, parts_opts, join: Optional[JoinOpts] = None, gains: bool = False):
    """ptts_join_parts: the parts (mono f32 at 24 kHz, in order), each at its PartOpts' volume, as one utterance with the seam of its PartOpts behind
    every part.  gains: also the f32 gain of every part.  Host: the statement of what Model.join_parts_rows and a joined call with a list compute."""
    rows, n, pp, ns = _join_in(parts)
    o = join if join is not None else JoinOpts()
    total = join_parts_length(ns[:n], parts_opts, o)
    out = np.empty(max(total, 1), np.float32)
    g = np.ones(max(n, 1), np.float32)
    _check(lib().ptts_join_parts(pp, _ip(ns), n, C.byref(o), _part_list(parts_opts), _fp(out), _fp(g)))
    return (out[:total], g[:n]) if gains else out[:total]


def join(parts, join: Optional[JoinOpts] = None) -> np.ndarray:
    """ptts_join: the parts (mono f32 at 24 kHz, in order) as one utterance, with join.gap_ms of silence or join.crossfade_ms of overlap at the
    seams.  Host: the statement of what Model.join_rows and Model.generate_joined compute."""
    rows, n, pp, ns = _join_in(parts)
    o = join if join is not None else JoinOpts()
    total = join_length(ns[:n], o)
    out = np.empty(max(total, 1), np.float32)
    _check(lib().ptts_join(pp, _ip(ns), n, C.byref(o), _fp(out)))
    return out[:total]


def dsp_apply(samples, normalize: bool = False, dc_block: bool = False, fade_in_ms: float = 0.0, fade_out_ms: float = 0.0) -> np.ndarray:
    """audio.PeakNormalize / DCBlock / FadeIn / FadeOut in the CLI's order (dsp.go:12-78, synth.go:361-390); returns a new array."""
    out = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    L = lib()
    L.ptts_dsp_apply.argtypes = [_FP, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double]
    _check(L.ptts_dsp_apply(_fp(out), out.size, 1 if normalize else 0, 1 if dc_block else 0, float(fade_in_ms), float(fade_out_ms)))
    return out


def _dsp_opts(cfg) -> Optional[DspOpts]:
    """The ptts_dsp_opts of a RuntimeGenerateConfig: None when nothing is set (the request carries NULL)."""
    raw = getattr(cfg, "dsp_opts", None)
    if raw is not None:
        return raw
    nz, dc = bool(getattr(cfg, "normalize", False)), bool(getattr(cfg, "dc_block", False))
    fi, fo = float(getattr(cfg, "fade_in_ms", 0.0)), float(getattr(cfg, "fade_out_ms", 0.0))
    eq = getattr(cfg, "eq", None)
    tp = getattr(cfg, "true_peak_dbtp", None)
    cmp_ = getattr(cfg, "compressor", None)
    lim = getattr(cfg, "limiter", None)
    des = getattr(cfg, "deesser", None)
    if not (nz or dc or fi != 0.0 or fo != 0.0 or eq is not None or tp is not None or cmp_ is not None or lim is not None or des is not None):
        return None
    o = DspOpts(1 if nz else 0, 1 if dc else 0, fi, fo)
    if eq is not None:
        o.eq = eq.h
    if tp is not None or cmp_ is not None or lim is not None or des is not None:
        o._ext = DspExt(true_peak_dbtp=None if tp is None else float(tp), compressor=cmp_, limiter=lim, deesser=des)   # (kept by the struct, which the request keeps: the handle lives as long as the call)
        o.ext = o._ext.h
    return o


class DspExt:
    """Further per-request options behind ptts_dsp_opts.ext (ptts_dsp_ext): a true-peak ceiling in dBTP (-60 .. 0; None: off), a compressor
    (a CompressorOpts; None: off), a de-esser (a DeesserOpts; None: off), a limiter (a LimiterOpts; None: off) and, for joined calls alone, a trim of the parts (a TrimOpts; None: off)
    and their tempo (a TempoOpts; None: off) and pitch (a PitchOpts; None: off), with the formants kept (a FormantOpts; None: they move with the pitch).
    With none of them the handle switches nothing on.  It belongs to no
    model; keep it alive while requests that name it are running, and set its compressor, de-esser and limiter before they start."""

    def __init__(self, true_peak_dbtp: Optional[float] = None, opts: Optional[DspExtOpts] = None, compressor: Optional[CompressorOpts] = None,
                 limiter: Optional[LimiterOpts] = None, trim: Optional["TrimOpts"] = None, tempo: Optional["TempoOpts"] = None,
                 pitch: Optional["PitchOpts"] = None, formant: Optional["FormantOpts"] = None, deesser: Optional[DeesserOpts] = None):
        o = opts if opts is not None else DspExtOpts(C.sizeof(DspExtOpts), 0 if true_peak_dbtp is None else 1,
                                                     0.0 if true_peak_dbtp is None else float(true_peak_dbtp))
        L = lib()
        L.ptts_dsp_ext_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.ptts_dsp_ext_free.argtypes = [C.c_void_p]
        L.ptts_dsp_ext_free.restype = None
        h = C.c_void_p()
        self.h = None
        _check(L.ptts_dsp_ext_create(C.byref(o), C.byref(h)))
        self.h = h.value
        if compressor is not None:
            self.set_compressor(compressor)
        if limiter is not None:
            self.set_limiter(limiter)
        if deesser is not None:
            self.set_deesser(deesser)
        if trim is not None:
            self.set_trim(trim)
        if tempo is not None:
            self.set_tempo(tempo)
        if pitch is not None:
            self.set_pitch(pitch)
        if formant is not None:
            self.set_formant(formant)

    def set_compressor(self, compressor: Optional[CompressorOpts]):
        """ptts_dsp_ext_set_compressor: attaches the compressor (None: off again).  Not while requests that name the handle are running."""
        _check(lib().ptts_dsp_ext_set_compressor(self.h, None if compressor is None else C.byref(compressor)))

    def set_limiter(self, limiter: Optional[LimiterOpts]):
        """ptts_dsp_ext_set_limiter: attaches the limiter (None: off again).  Not while requests that name the handle are running."""
        _check(lib().ptts_dsp_ext_set_limiter(self.h, None if limiter is None else C.byref(limiter)))

    def set_deesser(self, deesser: Optional[DeesserOpts]):
        """ptts_dsp_ext_set_deesser: attaches the de-esser (None: off again).  Not while requests that name the handle are running."""
        _check(lib().ptts_dsp_ext_set_deesser(self.h, None if deesser is None else C.byref(deesser)))

    def set_trim(self, trim: Optional[TrimOpts]):
        """ptts_dsp_ext_set_trim: attaches the trim of a joined call's parts (None: off again).  Served by Model.generate_joined, whose JoinOpts.dsp
        names the handle; a request's own dsp and Model.dsp_rows refuse a handle that carries one."""
        _check(lib().ptts_dsp_ext_set_trim(self.h, None if trim is None else C.byref(trim)))

    def set_tempo(self, tempo: Optional[TempoOpts]):
        """ptts_dsp_ext_set_tempo: attaches the tempo of a joined call's parts (None: off again).  Served by Model.generate_joined, whose
        JoinOpts.dsp names the handle, behind the trim; a request's own dsp and Model.dsp_rows refuse a handle that carries one."""
        _check(lib().ptts_dsp_ext_set_tempo(self.h, None if tempo is None else C.byref(tempo)))

    def set_pitch(self, pitch: Optional[PitchOpts]):
        """ptts_dsp_ext_set_pitch: attaches the pitch of a joined call's parts (None: off again).  Served by Model.generate_joined, whose
        JoinOpts.dsp names the handle, between the trim and the tempo; a request's own dsp and Model.dsp_rows refuse a handle that carries one."""
        _check(lib().ptts_dsp_ext_set_pitch(self.h, None if pitch is None else C.byref(pitch)))

    def set_formant(self, formant: Optional[FormantOpts]):
        """ptts_dsp_ext_set_formant: keeps the formants around the handle's pitch (None: off again).  Served where the pitch is; without a pitch, or
        at 1000, it switches nothing on."""
        _check(lib().ptts_dsp_ext_set_formant(self.h, None if formant is None else C.byref(formant)))

    def free(self):
        if self.h:
            lib().ptts_dsp_ext_free(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        self.free()


def compress_gain(compressor: CompressorOpts, level_db: float) -> float:
    """ptts_compress_gain: the static curve at level_db, in dB, makeup gain included, through the library's own log2 and exp2.  Host code."""
    out = C.c_double(0.0)
    _check(lib().ptts_compress_gain(C.byref(compressor), float(level_db), C.byref(out)))
    return float(out.value)


def _apply_on_host(entry, opts, samples) -> np.ndarray:
    out = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    _check(entry(C.byref(opts), _fp(out), out.size))
    return out


def compress_apply(compressor: CompressorOpts, samples) -> np.ndarray:
    """ptts_compress_apply: the compressor over mono f32 samples at 24 kHz, on the host, in the device kernels' blocked form; returns a new array."""
    return _apply_on_host(lib().ptts_compress_apply, compressor, samples)


def limit_apply(limiter: LimiterOpts, samples) -> np.ndarray:
    """ptts_limit_apply: the limiter over mono f32 samples at 24 kHz, on the host, in the device kernels' blocked form; returns a new array."""
    return _apply_on_host(lib().ptts_limit_apply, limiter, samples)


def deess_apply(deesser: DeesserOpts, samples) -> np.ndarray:
    """ptts_deess_apply: the de-esser over mono f32 samples at 24 kHz, on the host, in the device kernels' blocked form; returns a new array."""
    return _apply_on_host(lib().ptts_deess_apply, deesser, samples)


def deess_band(deesser: DeesserOpts, samples) -> np.ndarray:
    """ptts_deess_band: the de-esser's side chain alone -- its high-pass section over mono f32 samples at 24 kHz, Eq.apply of that one section --
    on the host; returns a new array."""
    x = _f32(samples).reshape(-1)
    out = np.empty(x.size, np.float32)
    _check(lib().ptts_deess_band(C.byref(deesser), _fp(x), x.size, _fp(out)))
    return out


def trim_plan(trim: TrimOpts, samples) -> TrimInfo:
    """ptts_trim_plan: what the trim makes of mono f32 samples at 24 kHz -- lo, hi, n_out, cuts, speech.  Host."""
    x = _f32(samples).reshape(-1)
    info = TrimInfo()
    _check(lib().ptts_trim_plan(C.byref(trim), _fp(x), x.size, C.byref(info)))
    return info


def trim_apply(trim: TrimOpts, samples, in_place: bool = False):
    """ptts_trim_apply: (the trimmed row as a new array, its TrimInfo).  Host: the statement of what Model.trim_rows and a joined call's trim
    compute.  in_place: the library writes over its input (out == in)."""
    x = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    out = x if in_place else np.empty(x.size, np.float32)
    info = TrimInfo()
    _check(lib().ptts_trim_apply(C.byref(trim), _fp(x), x.size, _fp(out), C.byref(info)))
    return out[:int(info.n_out)].copy(), info


def _neg(got: int) -> int:   # a host function's length or speed, or -code
    if got < 0:
        _check(-got)
    return got


def pitch_speed(pitch: PitchOpts, tempo: Optional[TempoOpts] = None) -> int:
    """ptts_pitch_speed: the speed the tempo runs at behind the resample, (1000 * s + p / 2) / p.  Host."""
    return _neg(int(lib().ptts_pitch_speed(C.byref(pitch), None if tempo is None else C.byref(tempo))))


def pitch_resample_length(pitch: PitchOpts, n: int) -> int:
    """ptts_pitch_resample_length: the samples of the resampled form of a row of n samples.  Host."""
    return _neg(int(lib().ptts_pitch_resample_length(C.byref(pitch), int(n))))


def pitch_length(pitch: PitchOpts, tempo: Optional[TempoOpts], n: int) -> int:
    """ptts_pitch_length: the samples of the shifted form of a row of n samples.  Host."""
    return _neg(int(lib().ptts_pitch_length(C.byref(pitch), None if tempo is None else C.byref(tempo), int(n))))


def pitch_resample(pitch: PitchOpts, samples) -> np.ndarray:
    """ptts_pitch_resample: the resampling step alone, as a new array.  Host: the statement of what k_pitch_resample computes."""
    x = _f32(samples).reshape(-1)
    n_r = pitch_resample_length(pitch, x.size)
    out = np.empty(max(n_r, 1), np.float32)
    _check(lib().ptts_pitch_resample(C.byref(pitch), _fp(x), x.size, _fp(out)))
    return out[:n_r].copy()


def pitch_apply(pitch: PitchOpts, tempo: Optional[TempoOpts], samples) -> np.ndarray:
    """ptts_pitch_apply: the shifted row as a new array.  Host: the statement of what Model.pitch_rows and a joined call's pitch compute."""
    x = _f32(samples).reshape(-1)
    n_f = pitch_length(pitch, tempo, x.size)
    out = np.empty(max(n_f, 1), np.float32)
    _check(lib().ptts_pitch_apply(C.byref(pitch), None if tempo is None else C.byref(tempo), _fp(x), x.size, _fp(out)))
    return out[:n_f].copy()


def formant_frames(n: int) -> int:
    """ptts_formant_frames: the frames K = ceil(n / 240) of a row of n samples.  Host."""
    return _neg(int(lib().ptts_formant_frames(int(n))))


def formant_analyse(samples) -> np.ndarray:
    """ptts_formant_analyse: the row's coefficients a32[1 .. 24] per frame, [K, 24] f32.  Host: the statement of k_formant_analyse."""
    x = _f32(samples).reshape(-1)
    out = np.zeros((max(formant_frames(x.size), 1), 24), np.float32)
    _check(lib().ptts_formant_analyse(_fp(x), x.size, _fp(out)))
    return out[:formant_frames(x.size)].copy()


def formant_whiten(coeffs, samples) -> np.ndarray:
    """ptts_formant_whiten: the row's residual under the coefficients [K, 24].  Host: the statement of k_formant_whiten."""
    x = _f32(samples).reshape(-1)
    c = np.ascontiguousarray(coeffs, np.float32)
    assert c.size == formant_frames(x.size) * 24
    out = np.empty(max(x.size, 1), np.float32)
    _check(lib().ptts_formant_whiten(_fp(c), _fp(x), x.size, _fp(out)))
    return out[:x.size].copy()


def formant_shape(coeffs, n: int, pitch_permille: int, residual) -> np.ndarray:
    """ptts_formant_shape: the envelopes of the part of n samples put back on its resampled residual.  Host: the statement of k_formant_shape."""
    e = _f32(residual).reshape(-1)
    c = np.ascontiguousarray(coeffs, np.float32)
    assert c.size == formant_frames(n) * 24
    out = np.empty(max(e.size, 1), np.float32)
    _check(lib().ptts_formant_shape(_fp(c), int(n), int(pitch_permille), _fp(e), e.size, _fp(out)))
    return out[:e.size].copy()


def formant_apply(formant: FormantOpts, pitch: PitchOpts, tempo: Optional[TempoOpts], samples) -> np.ndarray:
    """ptts_formant_apply: the shifted row with its formants kept, as a new array.  Host: the statement of what Model.formant_rows and a joined call
    with the option compute."""
    x = _f32(samples).reshape(-1)
    n_f = pitch_length(pitch, tempo, x.size)
    out = np.empty(max(n_f, 1), np.float32)
    _check(lib().ptts_formant_apply(C.byref(formant), C.byref(pitch), None if tempo is None else C.byref(tempo), _fp(x), x.size, _fp(out)))
    return out[:n_f].copy()


def pitch_table():
    """ptts_pitch_table: the prototype table of the resample, (h, hd) as f32 arrays of 6828 entries each.  Host."""
    h, hd, k = _FP(), _FP(), C.c_int32(0)
    _check(lib().ptts_pitch_table(C.byref(h), C.byref(hd), C.byref(k)))
    return np.ctypeslib.as_array(h, (k.value,)).copy(), np.ctypeslib.as_array(hd, (k.value,)).copy()


def tempo_length(tempo: TempoOpts, n: int) -> int:
    """ptts_tempo_length: the samples of the time-scaled form of a row of n samples.  Host."""
    got = int(lib().ptts_tempo_length(C.byref(tempo), int(n)))
    if got < 0:
        _check(-got)
    return got


def tempo_plan(tempo: TempoOpts, samples) -> np.ndarray:
    """ptts_tempo_plan: the read positions of the hops of mono f32 samples at 24 kHz, int32 [ceil(tempo_length / 480)].  Host."""
    x = _f32(samples).reshape(-1)
    hops = (tempo_length(tempo, x.size) + 479) // 480
    p = np.zeros(max(hops, 1), np.int32)
    _check(lib().ptts_tempo_plan(C.byref(tempo), _fp(x), x.size, p.ctypes.data_as(C.POINTER(C.c_int32))))
    return p[:hops]


def tempo_apply(tempo: TempoOpts, samples) -> np.ndarray:
    """ptts_tempo_apply: the time-scaled row as a new array.  Host: the statement of what Model.tempo_rows and a joined call's tempo compute."""
    x = _f32(samples).reshape(-1)
    out = np.empty(max(tempo_length(tempo, x.size), 1), np.float32)
    _check(lib().ptts_tempo_apply(C.byref(tempo), _fp(x), x.size, _fp(out)))
    return out[:tempo_length(tempo, x.size)].copy()


def true_peak(samples) -> float:
    """ptts_true_peak: the true peak (linear, an f32) of mono f32 samples at 24 kHz, eight times oversampled.  Host code."""
    x = _f32(samples).reshape(-1)
    out = C.c_float(0.0)
    L = lib()
    L.ptts_true_peak.argtypes = [_FP, C.c_int64, C.POINTER(C.c_float)]
    _check(L.ptts_true_peak(_fp(x), x.size, C.byref(out)))
    return np.float32(out.value)


def true_peak_limit(samples, ceiling_dbtp: float):
    """ptts_true_peak_limit: (a new array scaled by ceiling / true peak where the true peak exceeds the ceiling, the true peak before).  Host code."""
    x = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    out = C.c_float(0.0)
    L = lib()
    L.ptts_true_peak_limit.argtypes = [_FP, C.c_int64, C.c_double, C.POINTER(C.c_float)]
    _check(L.ptts_true_peak_limit(_fp(x), x.size, float(ceiling_dbtp), C.byref(out)))
    return x, np.float32(out.value)


def dsp_opts_error(opts: DspOpts) -> str:
    """Test hook (ptts_debug_dsp_opts_error): the message the library refuses these options with, "" when they are fine.  No GPU."""
    buf = C.create_string_buffer(512)
    hooks().ptts_debug_dsp_opts_error(C.byref(opts), buf, len(buf))
    return buf.value.decode(errors="replace")


def true_peak_taps():
    """Test hook (ptts_debug_true_peak_taps): (the meter's f32 taps [L][K], dlo)."""
    L_, K_, dlo = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    H = hooks()
    H.ptts_debug_true_peak_taps.argtypes = [_FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    _check(H.ptts_debug_true_peak_taps(None, C.byref(L_), C.byref(K_), C.byref(dlo)))
    out = np.zeros((L_.value, K_.value), np.float32)
    _check(H.ptts_debug_true_peak_taps(_fp(out), None, None, None))
    return out, int(dlo.value)


def true_peak_oversample(samples) -> np.ndarray:
    """Test hook (ptts_debug_true_peak_oversample): the eight-fold oversampled signal true_peak() takes its maximum over, [8 n] f32.  Host code."""
    x = _f32(samples).reshape(-1)
    y = np.zeros(8 * x.size, np.float32)
    H = hooks()
    H.ptts_debug_true_peak_oversample.argtypes = [_FP, C.c_int64, _FP]
    _check(H.ptts_debug_true_peak_oversample(_fp(x), x.size, _fp(y)))
    return y


def _eq_sections(sections):
    """(type, freq_hz, gain_db, q) tuples, or EqSection structs, as a ptts_eq_section array."""
    arr = (EqSection * max(len(sections), 1))()
    for i, s in enumerate(sections):
        arr[i] = s if isinstance(s, EqSection) else EqSection(int(s[0]), 0, float(s[1]), float(s[2]), float(s[3]))
    return arr


def eq_design(section) -> np.ndarray:
    """ptts_eq_design: b0, b1, b2, a1, a2 of one RBJ cookbook section at 24 kHz (float64, normalised by a0).  Host code."""
    arr = _eq_sections([section])
    out = np.zeros(5, np.float64)
    L = lib()
    L.ptts_eq_design.argtypes = [C.POINTER(EqSection), C.POINTER(C.c_double)]
    _check(L.ptts_eq_design(arr, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def eq_response(sections, freq_hz: float) -> float:
    """ptts_eq_response: the magnitude in dB of the cascade of 1 .. 4 sections at freq_hz.  Host code."""
    arr = _eq_sections(sections)
    out = C.c_double(0.0)
    L = lib()
    L.ptts_eq_response.argtypes = [C.POINTER(EqSection), C.c_int32, C.c_double, C.POINTER(C.c_double)]
    _check(L.ptts_eq_response(arr, len(sections), float(freq_hz), C.byref(out)))
    return float(out.value)


class Eq:
    """A per-request equaliser (ptts_eq): a cascade of 1 .. 4 biquad sections, (type, freq_hz, gain_db, q) each.  It belongs to no model; keep it
    alive while requests that name it (RuntimeGenerateConfig.eq) are running."""

    def __init__(self, sections):
        self.sections = list(sections)
        arr = _eq_sections(self.sections)
        L = lib()
        L.ptts_eq_create.argtypes = [C.POINTER(EqSection), C.c_int32, C.POINTER(C.c_void_p)]
        L.ptts_eq_free.argtypes = [C.c_void_p]
        L.ptts_eq_free.restype = None
        h = C.c_void_p()
        self.h = None
        _check(L.ptts_eq_create(arr, len(self.sections), C.byref(h)))
        self.h = h.value

    def apply(self, samples) -> np.ndarray:
        """ptts_eq_apply: the cascade over mono f32 samples at 24 kHz, on the host, in the device kernels' blocked form; returns a new array."""
        out = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
        L = lib()
        L.ptts_eq_apply.argtypes = [C.c_void_p, _FP, C.c_int64]
        _check(L.ptts_eq_apply(self.h, _fp(out), out.size))
        return out

    def rows(self, model, x):
        """ptts_eq_rows: apply() on the device of `model`."""
        return model.eq_rows(x, self)

    def response(self, freq_hz: float) -> float:
        return eq_response(self.sections, freq_hz)

    def free(self):
        if self.h:
            lib().ptts_eq_free(self.h)
            self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        self.free()


def loudness(samples) -> float:
    """ptts_loudness: integrated loudness after ITU-R BS.1770-4 of mono f32 samples at 24 kHz, in LUFS (-inf: nothing above the gates).  Host code."""
    x = _f32(samples).reshape(-1)
    out = C.c_double(0.0)
    L = lib()
    L.ptts_loudness.argtypes = [_FP, C.c_int64, C.POINTER(C.c_double)]
    _check(L.ptts_loudness(_fp(x), x.size, C.byref(out)))
    return float(out.value)


def loudness_normalize(samples, target_lufs: float):
    """ptts_loudness_normalize: (a new array at the target -- never above peak 1 --, the loudness measured before).  Host code."""
    x = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    out = C.c_double(0.0)
    L = lib()
    L.ptts_loudness_normalize.argtypes = [_FP, C.c_int64, C.c_double, C.POINTER(C.c_double)]
    _check(L.ptts_loudness_normalize(_fp(x), x.size, float(target_lufs), C.byref(out)))
    return x, float(out.value)


def loudness_energies(x, model=None):
    """Test hook (libptts_hooks.so ptts_debug_loudness_energies): the sums of squares of the K-weighted samples over each whole 480-sample sub-block
    of mono f32 rows at 24 kHz -- by the device kernels with a model, by the host instantiation of their functions without."""
    single, rows, n, pp, ns = _rows_in(x)
    outs = [np.zeros(r.size // 480, np.float64) for r in rows]
    _check(hooks().ptts_debug_loudness_energies(model.h if model is not None else None, pp, _ip(ns), n, _row_ptrs(outs, _DP)))
    return outs[0] if single else outs


def kweighting(sample_rate: int) -> np.ndarray:
    """Test hook (ptts_debug_kweighting): the K-weighting sections for a sample rate, [shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2]."""
    out = np.zeros(10, np.float64)
    H = hooks()
    H.ptts_debug_kweighting.argtypes = [C.c_int32, C.POINTER(C.c_double)]
    _check(H.ptts_debug_kweighting(int(sample_rate), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def dsp_blocked_host(samples) -> np.ndarray:
    """Test hook (libptts_hooks.so ptts_debug_dsp_blocked_host): the DC block in the device kernels' blocked form, evaluated on the host."""
    x = np.array(samples, dtype=np.float32, copy=True).reshape(-1)
    H = hooks()
    H.ptts_debug_dsp_blocked_host.argtypes = [_FP, C.c_int64, _FP]
    _check(H.ptts_debug_dsp_blocked_host(_fp(x), x.size, _fp(x)))
    return x


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 of a multi-GPU start-up)."""
    buf = (C.c_uint8 * 128)()
    _check(lib().ptts_rccl_unique_id(buf))
    return bytes(buf)


def rccl_broadcast(device_ptr: int, nbytes: int, rank: int, n_ranks: int, unique_id: bytes, device: int = 0):
    """The weight-arena broadcast (root = rank 0) over RCCL / xGMI, inside the library; every rank calls it."""
    L = lib()
    L.ptts_rccl_broadcast.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
    _check(L.ptts_rccl_broadcast(C.c_void_p(device_ptr), nbytes, rank, n_ranks, unique_id, device))


class Tokenizer:
    """tokenizer.Tokenizer (internal/tokenizer/tokenizer.go) backed by the library's SentencePiece unigram encoder
    (NewSentencePieceTokenizer / NewSentencePieceTokenizerFromBytes, sentencepiece.go:19-33)."""

    def __init__(self, model):
        L = lib()
        L.ptts_tokenizer_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.ptts_tokenizer_open_bytes.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.ptts_tokenizer_free.argtypes = [C.c_void_p]
        L.ptts_tokenizer_vocab_size.argtypes = [C.c_void_p]
        L.ptts_tokenizer_vocab_size.restype = C.c_int64
        L.ptts_tokenizer_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, _IP, C.c_int64]
        L.ptts_tokenizer_encode.restype = C.c_int64
        h = C.c_void_p()
        if isinstance(model, (bytes, bytearray)):
            buf = bytes(model)
            _check(L.ptts_tokenizer_open_bytes(buf, len(buf), C.byref(h)))
        else:
            _check(L.ptts_tokenizer_open(str(model).encode(), C.byref(h)))
        self.h = h.value

    @property
    def vocab_size(self) -> int:
        return int(lib().ptts_tokenizer_vocab_size(self.h))

    def encode(self, text: str) -> list:
        raw = text.encode("utf-8")
        ids = np.zeros(max(16, len(raw) + 2), np.int64)
        n = int(lib().ptts_tokenizer_encode(self.h, raw, len(raw), _ip(ids), ids.size))
        if n < 0:
            raise PttsError(PTTS_EINVAL, lib().ptts_last_error().decode())
        if n > ids.size:
            ids = np.zeros(n, np.int64)
            n = int(lib().ptts_tokenizer_encode(self.h, raw, len(raw), _ip(ids), ids.size))
        return [int(x) for x in ids[:n]]

    __call__ = encode

    def close(self):
        if self.h:
            lib().ptts_tokenizer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def nfkc(text: str) -> str:
    """NFKC as the tokenizer applies it (ptts_text_nfkc: generated Unicode tables)."""
    raw = text.encode("utf-8")
    L = lib()
    L.ptts_text_nfkc.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    buf = C.create_string_buffer(max(16, 20 * len(raw) + 16))   # one code point can expand to 18 (U+FDFA)
    _check(L.ptts_text_nfkc(raw, len(raw), buf, len(buf), C.byref(n)))
    return buf.raw[: n.value].decode("utf-8")


class _ChunkInfo(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_int64), ("token_ids", _IP), ("n_tokens", C.c_int64), ("num_words", C.c_int32),
                ("max_frames", C.c_int32), ("frames_after_eos", C.c_int32), ("reserved", C.c_int32)]


_ENCODE_FN = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, _IP, C.c_int64)


@dataclass
class ChunkMetadata:
    """text.ChunkMetadata (prepare.go:18-24) + MaxFrames / FramesAfterEOS."""
    text: str
    token_ids: list
    num_words: int
    max_frames: int
    frames_after_eos: int

    @property
    def num_tokens(self) -> int:
        return len(self.token_ids)


def estimate_max_frames(token_count: int, frame_rate: float = 12.5) -> int:
    L = lib()
    L.ptts_text_estimate_max_frames.argtypes = [C.c_int64, C.c_double]
    return int(L.ptts_text_estimate_max_frames(token_count, frame_rate))


def frames_after_eos(num_words: int) -> int:
    L = lib()
    L.ptts_text_frames_after_eos.argtypes = [C.c_int64]
    return int(L.ptts_text_frames_after_eos(num_words))


def prepare_text(text: str) -> str:
    """text.PrepareText (prepare.go:66-100)."""
    L = lib()
    L.ptts_text_prepare.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    raw = text.encode("utf-8", "surrogatepass")
    n = C.c_int64(0)
    buf = C.create_string_buffer(len(raw) + 16)
    _check(L.ptts_text_prepare(raw, len(raw), buf, len(buf), C.byref(n)))
    return buf.raw[: n.value].decode("utf-8", "replace")


def prepare_chunks(text: str, encode: Callable[[str], Sequence[int]], max_tokens: int = 50, frame_rate: float = 12.5) -> list:
    """text.PrepareChunks (prepare.go:105-184); `encode` plays the Tokenizer interface (prepare.go:12-16)."""
    L = lib()
    L.ptts_text_chunks.argtypes = [C.c_char_p, C.c_int64, _ENCODE_FN, C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_void_p)]
    L.ptts_chunks_count.argtypes = [C.c_void_p]
    L.ptts_chunks_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_ChunkInfo)]
    L.ptts_chunks_free.argtypes = [C.c_void_p]

    def cb(_user, ptr, n, ids, cap):
        got = list(encode(C.string_at(ptr, n).decode("utf-8", "replace")))
        for i, v in enumerate(got[:cap]):
            ids[i] = int(v)
        return len(got)

    raw = text.encode("utf-8", "surrogatepass")
    h = C.c_void_p()
    if isinstance(encode, Tokenizer):   # the library's own encoder: no callback into Python (encode == NULL, user = tokenizer)
        _check(L.ptts_text_chunks(raw, len(raw), C.cast(None, _ENCODE_FN), encode.h, max_tokens, frame_rate, C.byref(h)))
    else:
        fn = _ENCODE_FN(cb)
        _check(L.ptts_text_chunks(raw, len(raw), fn, None, max_tokens, frame_rate, C.byref(h)))
    try:
        out = []
        for i in range(L.ptts_chunks_count(h)):
            ci = _ChunkInfo()
            _check(L.ptts_chunks_get(h, i, C.byref(ci)))
            out.append(ChunkMetadata(C.string_at(ci.text, ci.text_len).decode("utf-8", "replace"), [int(ci.token_ids[k]) for k in range(ci.n_tokens)],
                                     int(ci.num_words), int(ci.max_frames), int(ci.frames_after_eos)))
        return out
    finally:
        L.ptts_chunks_free(h)


# ---- tts.Service (internal/tts/service.go): text in, audio out --------------------------------------------------------------
MAX_TOKENS_PER_CHUNK = 50          # service.go:21-23
DEFAULT_MAX_STEPS = 256            # config.DefaultConfig().TTS.MaxSteps: "use the estimate" (service.go:271-278)


@dataclass
class TTSConfig:
    """The config.TTS fields generateConfig reads (service.go:255-269)."""
    temperature: float = 0.0
    eos_threshold: float = -4.0
    max_steps: int = DEFAULT_MAX_STEPS
    lsd_decode_steps: int = 1


class Service:
    """tts.Service: PrepareChunks -> one GenerateAudio per chunk -> concatenated PCM (service.go:107-153).

    The reference generates the chunks one after the other.  They are independent (each chunk starts from the voice
    state), so here ALL chunks of a text go to the runtime in one batched call (or through a Dispatcher, where they are
    coalesced with other callers' chunks): a one-minute text costs about what one 10-second chunk costs."""

    def __init__(self, model: Model, encode: Callable[[str], Sequence[int]], tts: Optional[TTSConfig] = None, dispatcher: Optional["Dispatcher"] = None):
        self.model, self.encode, self.tts, self.dispatcher = model, encode, tts or TTSConfig(), dispatcher

    def generate_config(self, chunk: "ChunkMetadata", **voice) -> RuntimeGenerateConfig:   # service.go:255-278
        frame_rate, _, spl = self.model.info.frame_rate, self.model.info.encoder_frame_rate, self.model.info.steps_per_latent
        est = estimate_max_frames(chunk.num_tokens, frame_rate)
        limit = est if est > 0 and (self.tts.max_steps <= 0 or self.tts.max_steps == DEFAULT_MAX_STEPS) else self.tts.max_steps
        return RuntimeGenerateConfig(temperature=self.tts.temperature, eos_threshold=self.tts.eos_threshold, max_steps=limit,
                                     estimated_max_steps=est, lsd_decode_steps=self.tts.lsd_decode_steps, frames_after_eos=chunk.frames_after_eos,
                                     mimi_steps_per_latent=spl, mimi_sequence_length=est * spl, **voice)

    def synthesize_chunks(self, text: str, **voice) -> list:
        """[(ChunkMetadata, GenerateResult)] in text order."""
        try:
            chunks = prepare_chunks(text, self.encode, MAX_TOKENS_PER_CHUNK, self.model.info.frame_rate)
        except PttsError as e:
            raise PttsError(e.code, f"no tokens produced from input: {e}") from None   # service.go:124-126
        cfgs = [self.generate_config(c, **voice) for c in chunks]
        if self.dispatcher is not None:
            import concurrent.futures as cf
            with cf.ThreadPoolExecutor(max_workers=len(chunks)) as ex:
                res = list(ex.map(lambda cc: self.dispatcher.generate(cc[0].token_ids, cc[1]), zip(chunks, cfgs)))
        else:
            res = self.model.generate_batch([c.token_ids for c in chunks], cfgs)
        return list(zip(chunks, res))

    def synthesize(self, text: str, **voice) -> np.ndarray:
        """Service.Synthesize (service.go:107-153): the chunks' PCM, concatenated."""
        parts = [r.pcm for _, r in self.synthesize_chunks(text, **voice)]
        return np.concatenate(parts) if parts else np.zeros(0, np.float32)

    def synthesize_joined(self, text: str, join: Optional[JoinOpts] = None, pcm_callback=None, first_group: int = 0, **voice) -> JoinedResult:
        """Service.Synthesize with the join, the post-processing over the whole text (cmd/pockettts/synth.go:361-390) and the egress on the
        device, in one call (Model.generate_joined): one result for the text, parts[i] says where chunk i lies in it.  Joined requests do not
        go through a dispatcher, which deals single requests.  pcm_callback(offset, samples): the audio is handed over group by group while the later
        groups run (Model.generate_joined), first_group parts in the first group (0: max_batch) for sooner first audio."""
        if self.dispatcher is not None:
            raise PttsError(PTTS_EINVAL, "synthesize_joined: a service with a dispatcher deals single requests; joined calls go to the model")
        try:
            chunks = prepare_chunks(text, self.encode, MAX_TOKENS_PER_CHUNK, self.model.info.frame_rate)
        except PttsError as e:
            raise PttsError(e.code, f"no tokens produced from input: {e}") from None   # service.go:124-126
        cfgs = [self.generate_config(c, **voice) for c in chunks]
        if pcm_callback is None and not first_group:
            return self.model.generate_joined([c.token_ids for c in chunks], cfgs, join)
        return self.model.generate_joined([c.token_ids for c in chunks], cfgs, join, pcm_callback=pcm_callback, first_group=first_group)
