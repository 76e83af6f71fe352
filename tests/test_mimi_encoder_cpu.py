"""The Mimi encoder without a GPU -- PARITY UNPINNED: inferred architecture, no reference fixture.

The checker's own properties (frame count, causality, its convolution against the oracle's conv KATs, its transformer layer against the oracle's
decoder transformer), the ABI the product library exports, the frame count the library reports, the synthetic checkpoint's encoder tensors and
the loader's shape checks (planning needs no device)."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
import _mimi_encoder_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tiny(pkg):
    cfg = dataclasses.replace(pkg.synth.SynthConfig.tiny(), encoder=True)
    return cfg, pkg.synth.make_checkpoint(cfg, seed=5)


# ---------------------------------------------------------------- the checker

@pytest.mark.parametrize("n", [1, 1919, 1920, 1921, 3840, 5000])
def test_parity_unpinned_checker_frame_count_is_ceil_n_over_1920(tiny, n):
    _, t = tiny
    ref = R.EncoderRef(t)
    assert ref.hop == 1920
    lat = ref.encode(np.random.default_rng(n).standard_normal(n) * 0.3)
    assert lat.shape == (-(-n // 1920), 512) == (R.frames_of(n), 512)


def test_parity_unpinned_checker_stages_have_the_chain_shapes(tiny):
    cfg, t = tiny
    st = R.EncoderRef(t).stages(np.random.default_rng(1).standard_normal(1921) * 0.3)
    f = cfg.n_filters
    want = [(3840, f), (3840, f), (960, 2 * f), (960, 2 * f), (192, 4 * f), (192, 4 * f), (32, 8 * f), (32, 512), (32, 512), (2, 512)]
    assert [st[k].shape for k in R.STAGES] == want


def test_parity_unpinned_checker_is_causal(tiny):
    _, t = tiny
    ref = R.EncoderRef(t)
    x = np.random.default_rng(2).standard_normal(5 * 1920) * 0.3
    base = ref.encode(x)
    for tf in (0, 2):
        y = x.copy()
        y[(tf + 1) * 1920:] = np.random.default_rng(3).standard_normal(y.size - (tf + 1) * 1920)   # after frame tf's receptive field
        got = ref.encode(y)
        np.testing.assert_allclose(got[:tf + 1], base[:tf + 1], rtol=0, atol=1e-12)
        assert np.abs(got[tf + 1:] - base[tf + 1:]).max() > 1e-6   # (and the later frames do see it)


def test_parity_unpinned_checker_conv_matches_the_oracle_conv_kats():
    with open(os.path.join(HERE, "golden", "reference_kat.json")) as f:
        kat = {c["name"]: c for c in json.load(f)["cases"]}
    c = kat["conv1d_ones"]   # runtime/ops/conv1d_test.go:9-22, stride 1
    got = R.conv1d(np.array(c["x"], np.float64).reshape(c["x_shape"])[0], np.array(c["w"], np.float64).reshape(c["w_shape"]), None)
    assert got.numpy().ravel().tolist() == c["want"]
    # the causal stride-1 form equals the oracle's left-padded conv (conv1d.go:95: leftPad k - 1) on random data
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 6, 50)).astype(np.float32)
    w = rng.standard_normal((5, 6, 3)).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    want = O.conv1d(x, w, b, 1, 2)[0]
    np.testing.assert_allclose(R.causal_conv(x[0], w, b).numpy(), want, rtol=0, atol=2e-5)
    # and a stride-s conv with k - s zeros of history equals the oracle's with lpad = k - s
    w8 = rng.standard_normal((5, 6, 8)).astype(np.float32)
    np.testing.assert_allclose(R.causal_conv(x[0, :, :48], w8, b, stride=4).numpy(), O.conv1d(x[:, :, :48], w8, b, 4, 4)[0], rtol=0, atol=2e-5)


def test_parity_unpinned_checker_layer_matches_the_oracle_decoder_transformer(pkg):
    """The checker's transformer layer is the decoder transformer's: run on the decoder's weights it equals the oracle's staged
    upsample + decoder transformer (mimi.go:733-748) -- 30 frames, so 480 rows and a window that slides (250 keys)."""
    cfg = pkg.synth.SynthConfig.tiny()
    t = pkg.synth.make_checkpoint(cfg, seed=9)
    om = O.OracleModel(t)
    x = (np.random.default_rng(6).standard_normal((512, 30)) * 0.5).astype(np.float32)
    want = om.mimi_transformer(x)
    om.close()
    w = t["mimi.upsample.convtr.convtr.weight"][:, 0, :].astype(np.float64)   # depthwise, k = 32, stride 16, right-trimmed
    xs = x.T.astype(np.float64)
    prev = np.vstack([np.zeros((1, 512)), xs[:-1]])
    up = (xs[:, None, :] * w[:, :16].T[None] + prev[:, None, :] * w[:, 16:].T[None]).reshape(480, 512)   # row 16 t + r
    rows = torch.as_tensor(up)
    p = "mimi.decoder_transformer.transformer.layers."
    for i in range(cfg.mimi_layers):
        rows = R.transformer_layer(rows, {k[len(p) + len(str(i)) + 1:]: v for k, v in t.items() if k.startswith(f"{p}{i}.")}, 8, 250)
    np.testing.assert_allclose(rows.numpy(), want, rtol=0, atol=5e-5 * max(1.0, float(np.abs(want).max())))


# ---------------------------------------------------------------- the library

def test_product_library_exports_the_encoder_abi(pkg):
    lib = ctypes.CDLL(pkg.runtime.LIB_PATH)
    for s in ("ptts_mimi_encode", "ptts_mimi_encode_frames", "ptts_voice_encode_audio"):
        assert hasattr(lib, s), s
    assert not hasattr(lib, "ptts_debug_encode_stages")
    assert hasattr(ctypes.CDLL(pkg.runtime.HOOKS_PATH), "ptts_debug_encode_stages")


@pytest.mark.parametrize("n,want", [(1, 1), (1919, 1), (1920, 1), (1921, 2), (0, 0), (30 * 24000, 375)])
def test_mimi_encode_frames(pkg, n, want):
    assert pkg.runtime.mimi_encode_frames(n) == want


def test_mimi_encode_frames_rejects_a_negative_count(pkg):
    assert pkg.runtime.mimi_encode_frames(-1) == -pkg.runtime.PTTS_EINVAL


# ---------------------------------------------------------------- synthetic checkpoints and the loader

@pytest.mark.parametrize("which", ["tiny", "full"])
def test_synth_encoder_tensors_come_from_their_own_stream(pkg, which):
    base = getattr(pkg.synth.SynthConfig, which)()
    a = pkg.synth.make_checkpoint(base, seed=3)
    b = pkg.synth.make_checkpoint(dataclasses.replace(base, encoder=True), seed=3)
    assert set(a) < set(b)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    f, M = base.n_filters, base.mimi_dim
    e = "mimi.encoder.model."
    want = {e + "0.conv.weight": (f, 1, 7), e + "1.block.1.conv.weight": (f // 2, f, 3), e + "1.block.3.conv.weight": (f, f // 2, 1),
            e + "3.conv.weight": (2 * f, f, 8), e + "4.block.1.conv.weight": (f, 2 * f, 3), e + "6.conv.weight": (4 * f, 2 * f, 10),
            e + "7.block.3.conv.weight": (4 * f, 2 * f, 1), e + "9.conv.weight": (8 * f, 4 * f, 12), e + "11.conv.weight": (M, 8 * f, 3),
            "mimi.downsample.conv.conv.weight": (M, M, 32)}
    assert {k: b[k].shape for k in want} == want
    assert "mimi.downsample.conv.conv.bias" not in b
    assert sum(k.startswith("mimi.encoder_transformer.transformer.layers.") and k.endswith("norm1.weight") for k in b) == base.mimi_layers


def _plan(pkg, path, **kw):
    p, n = pkg.Model.plan(path, **kw)
    pkg.runtime.lib().ptts_plan_free(p)
    return n


@pytest.mark.parametrize("weights", ["f32", "bf16"])
def test_encoder_weights_add_to_the_arena_only_when_present(pkg, tmp_path, weights):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    w = pkg.WEIGHTS_F32 if weights == "f32" else pkg.WEIGHTS_BF16
    plain, enc = str(tmp_path / "plain.safetensors"), str(tmp_path / "enc.safetensors")
    synth.write_safetensors(plain, synth.make_checkpoint(cfg, seed=3))
    synth.write_safetensors(enc, synth.make_checkpoint(dataclasses.replace(cfg, encoder=True), seed=3))
    a, b = _plan(pkg, plain, weights=w), _plan(pkg, enc, weights=w)
    assert b > a


@pytest.mark.parametrize("key,shape,msg", [
    ("mimi.encoder.model.3.conv.weight", (32, 16, 7), "kernel 7"),
    ("mimi.encoder.model.6.conv.weight", (64, 24, 10), "down conv 2 input channels"),
    ("mimi.encoder.model.11.conv.weight", (256, 128, 3), "tail conv"),
    ("mimi.downsample.conv.conv.weight", (512, 512, 30), "hop"),
])
def test_encoder_shapes_are_checked_against_the_chain(pkg, tmp_path, key, shape, msg):
    synth = pkg.synth
    t = synth.make_checkpoint(dataclasses.replace(synth.SynthConfig.tiny(), encoder=True), seed=3)
    t[key] = np.zeros(shape, np.float32)
    path = str(tmp_path / "bad.safetensors")
    synth.write_safetensors(path, t)
    with pytest.raises(pkg.PttsError) as ei:
        pkg.Model.plan(path)
    assert ei.value.code == pkg.runtime.PTTS_EFORMAT and msg in str(ei.value), str(ei.value)


def test_a_missing_encoder_tensor_is_named(pkg, tmp_path):
    synth = pkg.synth
    t = synth.make_checkpoint(dataclasses.replace(synth.SynthConfig.tiny(), encoder=True), seed=3)
    del t["mimi.encoder.model.4.block.3.conv.weight"]
    path = str(tmp_path / "bad.safetensors")
    synth.write_safetensors(path, t)
    with pytest.raises(pkg.PttsError) as ei:
        pkg.Model.plan(path)
    assert 'mimi.encoder.model.4.block.3.conv.weight" not found' in str(ei.value)


# arena bytes of these checkpoints before the encoder existed (the parent tree's ptts_plan_arena_bytes): without encoder keys nothing changes
ARENA_BEFORE = {("tiny", "F32"): 100451328, ("tiny", "BF16"): 54656000, ("full", "BF16"): 394411264}


@pytest.mark.parametrize("size,dtype", list(ARENA_BEFORE))
def test_a_checkpoint_without_encoder_keys_plans_the_same_arena(pkg, tmp_path, size, dtype):
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny() if size == "tiny" else synth.SynthConfig.full(), speaker_proj=True)
    path = str(tmp_path / "plain.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234), dtype=dtype)
    assert _plan(pkg, path, weights=pkg.WEIGHTS_F32 if dtype == "F32" else pkg.WEIGHTS_BF16) == ARENA_BEFORE[(size, dtype)]
