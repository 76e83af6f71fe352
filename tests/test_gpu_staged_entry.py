"""Two properties of the staged entry points' device side (csrc/staged.cpp) that the engine relies on and nothing else holds:

  * ptts_flow_direction is the independent check of the AR step's flow part, so it must not run the step's own kernels: at 1, 3 and 17 rows it
    launches neither k_skinny (where launch_gemm sends a product of at most 64 rows whose operand carries the step's fragment-ordered weight copy)
    nor k_flow_cluster (the residual blocks as one launch).  The names are the launch census's: tests/test_gpu_step_staged.py and
    tests/test_gpu_flow_cluster.py assert that the step itself launches them under these names.
  * the speaker projection is built in one place: the embedding ptts_voice_encode_audio derives from a clip has the bits of ptts_speaker_project on
    the latents ptts_mimi_encode gives for the same clip.

Tiny synthetic checkpoint with the encoder and the speaker projection, as an F32 and as a BF16 file."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP_KERNELS = ("k_skinny", "k_flow_cluster")


@pytest.fixture(scope="module", params=["F32", "BF16"])
def gm(request, pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), encoder=True, speaker_proj=True)
    path = str(tmp_path_factory.mktemp("staged") / f"tiny_{request.param}.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234), dtype=request.param)
    m = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_F32 if request.param == "F32" else pkg.WEIGHTS_BF16)
    yield m
    m.close()


@pytest.mark.parametrize("rows", [1, 3, 17])
def test_flow_direction_stays_off_the_step_kernels(pkg, gm, rows):
    rng = np.random.default_rng(rows)
    c = rng.standard_normal((rows, gm.info.d_model)).astype(np.float32)
    x = rng.standard_normal((rows, gm.info.ldim)).astype(np.float32)
    pkg.runtime.launch_counts(True)
    out = gm.flow_direction(c, 0.25, 0.5, x)
    counts = pkg.runtime.launch_counts(False)
    assert out.shape == x.shape and np.isfinite(out).all()
    assert sum(counts.values()) > 0, counts   # the census saw the call
    assert not [k for k in STEP_KERNELS if counts.get(k, 0)], counts


def test_speaker_project_has_the_bits_of_voice_encode_audio(gm):
    n = 12000   # 0.5 s
    rng = np.random.default_rng(5)
    clip = (0.3 * np.sin(2 * np.pi * 180 * np.arange(n) / 24000) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    voice = gm.voice_from_audio(clip)                       # ptts_voice_encode_audio: the projection on the latents where the encoder left them
    two_step = gm.speaker_project(gm.encode_audio(clip))    # ptts_mimi_encode, then ptts_speaker_project on the uploaded latents
    got = np.asarray(voice.data).reshape(two_step.shape)
    assert two_step.shape == (7, gm.info.d_model) and np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, two_step)
