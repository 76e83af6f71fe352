"""The Mimi encoder on the GPU -- PARITY UNPINNED: inferred architecture, no reference fixture.

The reference has no native encoder (mimi.go:14,791-794), so the yardstick is tests/_mimi_encoder_ref.py: the inferred chain restated in float64
torch on the CPU, given exactly the weights the kernels compute with (a BF16 file's values; an F32 file's, which the kernels split into bf16
hi + lo like the decoder's).  Tolerances, as tests/_parity.py's conv constants: max abs error over max(1, max|want|), and the relative error on
the elements >= 1e-2 of the largest.  Observed on MI355X over every case here (profiles/mimi_encoder_parity_observed.jsonl): abs 1.5e-5 / rel 1.2e-3
(F32 files; BF16 files 8e-6 / 5.6e-4), the same at every stage and length -- the bars are about 10x the worst case."""
import dataclasses

import numpy as np
import pytest

from _parity import parity
import _mimi_encoder_ref as R

pytestmark = pytest.mark.gpu

SR = 24000
LENGTHS = [1, 1919, 1920, 1921, 5 * SR, 30 * SR]
# (abs, rel) per stage and for the whole chain
TOL_STAGE = (1.5e-4, 1.2e-2)
TOL_LATENT = (1.5e-4, 1.2e-2)


def pcm_of(n, seed=0):
    rng = np.random.default_rng(seed + n)
    t = np.arange(n) / SR
    return (0.3 * np.sin(2 * np.pi * 180 * t) * np.sin(2 * np.pi * 3 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def _model(pkg, tmp_path_factory, size, dtype, **cfgkw):
    synth = pkg.synth
    base = synth.SynthConfig.tiny() if size == "tiny" else synth.SynthConfig.full()
    cfg = dataclasses.replace(base, encoder=True, **cfgkw)
    t = synth.make_checkpoint(cfg, seed=21)
    path = str(tmp_path_factory.mktemp("enc") / f"{size}_{dtype}.safetensors")
    synth.write_safetensors(path, t, dtype=dtype)
    t = synth.quantize_like_file(t, dtype)
    gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_F32 if dtype == "F32" else pkg.WEIGHTS_BF16)
    return cfg, t, gm


@pytest.fixture(scope="module", params=[("tiny", "F32"), ("tiny", "BF16"), ("full", "F32"), ("full", "BF16")], ids=lambda p: f"{p[0]}-{p[1]}")
def enc(request, pkg, tmp_path_factory):
    cfg, t, gm = _model(pkg, tmp_path_factory, *request.param, speaker_proj=True)
    yield request.param, cfg, R.EncoderRef(t), t, gm
    gm.close()


@pytest.mark.parametrize("n", LENGTHS)
def test_parity_unpinned_encoder_matches_the_checker(enc, n):
    (size, dtype), _, ref, _, gm = enc
    x = pcm_of(n)
    got = gm.encode_audio(x)
    want = ref.encode(x)
    assert got.shape == want.shape == (R.frames_of(n), 512)
    parity(f"parity unpinned: mimi encoder latent {size} {dtype} n={n}", got, want, TOL_LATENT, rel_floor=1e-2)


@pytest.mark.parametrize("n", [1921, 5 * SR])
def test_parity_unpinned_encoder_stages_match_the_checker(enc, n):
    (size, dtype), _, ref, _, gm = enc
    x = pcm_of(n, seed=1)
    got = gm.encode_stages(x)
    want = ref.stages(x)
    for name, g in zip(R.STAGES, got):
        parity(f"parity unpinned: mimi encoder stage {name} {size} {dtype} n={n}", g, want[name], TOL_STAGE if name != "latent" else TOL_LATENT,
               rel_floor=1e-2)
    assert np.array_equal(got[-1], gm.encode_audio(x))   # the staged run computes what the product call does


def test_clips_in_one_call_equal_each_clip_alone(enc):
    _, _, _, _, gm = enc
    clips = [pcm_of(n, seed=3) for n in (3 * SR + 17, 1, 1921, 10 * SR, 7 * 1920)]
    batched = gm.encode_audio(clips)
    for c, b in zip(clips, batched):
        assert np.array_equal(gm.encode_audio(c), b)


def test_later_samples_leave_earlier_frames_bit_identical(enc):
    _, _, _, _, gm = enc
    x = pcm_of(12 * 1920, seed=4)
    base = gm.encode_audio(x)
    for tf in (0, 5):
        y = x.copy()
        y[(tf + 1) * 1920:] = pcm_of(y.size - (tf + 1) * 1920, seed=9)   # after frame tf's receptive field
        got = gm.encode_audio(y)
        assert np.array_equal(got[:tf + 1], base[:tf + 1])
        assert not np.array_equal(got[tf + 1:], base[tf + 1:])


def test_voice_from_audio_is_speaker_project_of_encode_audio(pkg, enc):
    (size, _), cfg, _, _, gm = enc
    x = pcm_of(2 * SR + 5, seed=5)
    lat = gm.encode_audio(x)
    two_step = gm.speaker_project(lat)
    voice = gm.voice_from_audio(x)
    assert tuple(voice.shape) == (1, lat.shape[0], cfg.d_model)
    assert np.array_equal(voice.data, two_step)
    if size != "tiny":
        return
    toks = [10, 20, 30]
    rc = lambda v: pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=4, voice_embedding=v, want_latents=True)
    a = pkg.Runtime(gm).generate(toks, rc(voice))
    b = pkg.Runtime(gm).generate(toks, rc(pkg.VoiceEmbedding(two_step, (1,) + two_step.shape)))
    assert a.n_frames == b.n_frames == 4
    assert np.array_equal(a.latents, b.latents) and np.array_equal(a.pcm, b.pcm)


def test_the_encoder_kernels_ran(pkg, enc):
    (size, dtype), _, _, _, gm = enc
    pkg.runtime.launch_counts(True)
    gm.encode_audio(pcm_of(10 * SR, seed=6))
    counts = pkg.runtime.launch_counts(False)
    for k in ("k_enc_head", "k_enc_ds_partial", "k_enc_ds_reduce"):
        assert counts.get(k, 0) == 1, counts
    if size == "full":
        assert counts.get("k_resblock", 0) == 2, counts   # widths 64 and 128 (256 runs as two products)
        if dtype == "BF16":
            assert counts.get("k_gemm5", 0) >= 3 and counts.get("k_mimi_ffn", 0) == 2 and counts.get("k_mimi_rowlin+rope", 0) == 2, counts
    assert sum(v for k, v in counts.items() if k.startswith("k_attn")) == (2 if size == "full" else 1), counts


def test_invalid_clips_are_rejected(pkg, enc):
    _, _, _, _, gm = enc
    with pytest.raises(pkg.PttsError) as ei:
        gm.encode_audio(np.zeros(0, np.float32))
    assert ei.value.code == pkg.runtime.PTTS_EINVAL
    with pytest.raises(pkg.PttsError) as ei:
        gm.encode_audio(np.zeros(512 * 1920 + 1, np.float32))   # 513 frames: past the transformer's RoPE table
    assert ei.value.code == pkg.runtime.PTTS_EINVAL and "513 frames" in str(ei.value)
    assert gm.encode_audio(np.zeros(512 * 1920, np.float32)).shape == (512, 512)


# ---------------------------------------------------------------- checkpoints without the encoder / the projection

# arena bytes of these checkpoints before the encoder existed (the parent tree's ptts_plan_arena_bytes): a checkpoint without encoder keys loads the same
ARENA_BEFORE = {("tiny", "F32"): 100451328, ("tiny", "BF16"): 54656000, ("full", "BF16"): 394411264}


@pytest.mark.parametrize("size,dtype", list(ARENA_BEFORE))
def test_a_checkpoint_without_encoder_loads_as_before_and_the_calls_name_the_tensor(pkg, tmp_path, size, dtype):
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny() if size == "tiny" else synth.SynthConfig.full(), speaker_proj=True)
    path = str(tmp_path / "plain.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234), dtype=dtype)
    gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_F32 if dtype == "F32" else pkg.WEIGHTS_BF16)
    try:
        assert gm.info.arena_bytes == ARENA_BEFORE[(size, dtype)]
        for call in (lambda: gm.encode_audio(pcm_of(1920)), lambda: gm.encode_audio([pcm_of(5), pcm_of(7)]), lambda: gm.voice_from_audio(pcm_of(1920))):
            with pytest.raises(pkg.PttsError) as ei:
                call()
            assert ei.value.code == pkg.runtime.PTTS_EFORMAT and '"mimi.encoder.model.0.conv.weight" not found' in str(ei.value)
        # the decoder side is untouched
        got = pkg.Runtime(gm).generate([10, 20, 30], pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=2))
        assert got.n_frames == 2
    finally:
        gm.close()


def test_voice_from_audio_without_a_speaker_projection_names_it(pkg, tmp_path_factory):
    _, _, gm = _model(pkg, tmp_path_factory, "tiny", "F32")
    try:
        assert gm.encode_audio(pcm_of(1920)).shape == (1, 512)
        with pytest.raises(pkg.PttsError) as ei:
            gm.voice_from_audio(pcm_of(1920))
        assert ei.value.code == pkg.runtime.PTTS_EFORMAT and "speaker_proj_weight" in str(ei.value)
    finally:
        gm.close()


# ---------------------------------------------------------------- BASELINE configs[4] with the encoder in

def test_config4_cloned_voice_at_full_size_with_the_encoder(pkg, tmp_path):
    """configs[4]'s cloned-voice leg at the reference's shapes (as test_config4_streaming_at_full_size_encoder_left_out, with the encoder in):
    10 s of reference audio -> encoder -> speaker projection on the device -> a 125-frame voice embedding, then two chunks of one text in one
    batched call on int8 step weights + bf16 KV under graph replay.  The embedding is the two-step path's bit for bit, and so is the audio."""
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.full(), speaker_proj=True, encoder=True)
    path = str(tmp_path / "full_enc.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=77), dtype="BF16")
    gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_INT8, kv=1, max_batch=8, use_graph=True)
    try:
        audio = pcm_of(10 * SR, seed=8)
        voice = gm.voice_from_audio(audio)
        assert tuple(voice.shape) == (1, 125, cfg.d_model) and np.isfinite(voice.data).all()
        two = gm.speaker_project(gm.encode_audio(audio))
        assert np.array_equal(voice.data, two)
        toks = [p.tolist() for p in synth.make_prompts(2, 40, cfg.n_bins, seed=3)]
        c = lambda v: pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=24, voice_embedding=v, want_latents=True)
        a = gm.generate_batch(toks, [c(voice)] * 2)
        b = gm.generate_batch(toks, [c(pkg.VoiceEmbedding(two, (1,) + two.shape))] * 2)
        for x, y in zip(a, b):
            assert x.n_frames == 24 and x.pcm.shape == (24 * 1920,) and np.isfinite(x.pcm).all()
            assert np.array_equal(x.latents, y.latents) and np.array_equal(x.pcm, y.pcm)
    finally:
        gm.close()
