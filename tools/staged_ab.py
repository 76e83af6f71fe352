"""A/B of two builds of the library through the staged and kernel-level entry points: one line per call with the SHA-256 of every output and the
launch census.  Needs a GPU and no reference tree.  Run it once per build and diff the printouts: same bits, same kernels, same counts.

    python tools/staged_ab.py > a.txt          (this tree's build; another tree's build: run its own copy of this file from that tree)
    diff a.txt b.txt

The checkpoint is the tests' synthetic one (SynthConfig.tiny with the encoder and the speaker projection, seed 1234), as an F32 and as a BF16 file; every
input comes from a fixed seed."""
import dataclasses
import hashlib
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ptts_amd

pkg = ptts_amd.load()
R = pkg.runtime


def sha(a) -> str:
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def call(name, fn):
    """fn() -> an array or a sequence of arrays; prints their digests and the launches the call made"""
    R.launch_counts(True)
    out = fn()
    counts = R.launch_counts(False)
    outs = out if isinstance(out, (list, tuple)) else [out]
    census = " ".join(f"{k}={v}" for k, v in sorted(counts.items())) or "-"
    print(f"{name}\t{' '.join(sha(o) for o in outs)}\t{census}", flush=True)
    return out


def model_calls(tag, gm, cfg):
    info = gm.info
    rng = np.random.default_rng(7)
    for n in (1, 17):
        call(f"{tag} text_embeddings n={n}", lambda: gm.text_embeddings(rng.integers(0, cfg.n_bins, n)))
    for slots in (1, 3):
        for noisy in (False, True):
            toks = [rng.integers(0, cfg.n_bins, 3 + 2 * i) for i in range(slots)]
            b = gm.new_batch(slots, 64)
            embs = [gm.text_embeddings(t) for t in toks]
            call(f"{tag} batch.prompt slots={slots}", lambda: (b.prompt(embs), b.offsets())[1])
            frames = np.full((slots, info.ldim), np.nan, np.float32)
            for step in range(3):
                noise = rng.standard_normal((slots, info.ldim)).astype(np.float32) if noisy else None
                out = call(f"{tag} batch.step slots={slots} noise={int(noisy)} step={step}", lambda: b.step(frames, noise=noise))
                frames = out[0]
            call(f"{tag} batch.read_kv slots={slots} noise={int(noisy)}", lambda: [a for sl in range(slots) for a in b.read_kv(sl, info.n_layers - 1)])
            b.close()
    for n, fr in ((1, 2), (3, 5)):
        lat = (rng.standard_normal((n, fr, info.ldim)) * 0.5).astype(np.float32)
        call(f"{tag} decode_latents {n}x{fr}", lambda: gm.decode_latents(lat))
        call(f"{tag} decode_latents {n}x{fr} mimi_latent", lambda: gm.decode_latents(lat, want_mimi_latent=True))
    for fr in (1, 9):
        x = (rng.standard_normal((fr, info.mimi_dim)) * 0.3).astype(np.float32)
        call(f"{tag} speaker_project frames={fr}", lambda: gm.speaker_project(x))
    clip = (0.3 * np.sin(2 * np.pi * 180 * np.arange(12000) / 24000) + 0.1 * rng.standard_normal(12000)).astype(np.float32)
    call(f"{tag} voice_from_audio 0.5s", lambda: gm.voice_from_audio(clip).data)
    call(f"{tag} encode_audio 0.5s", lambda: gm.encode_audio(clip))
    call(f"{tag} noise_rows seed=7 t=0.7 rows=5", lambda: gm.noise_rows(7, 0.7, 5))
    for n in (1, 3, 17):
        c = rng.standard_normal((n, info.d_model)).astype(np.float32)
        x = rng.standard_normal((n, info.ldim)).astype(np.float32)
        call(f"{tag} flow_direction rows={n}", lambda: gm.flow_direction(c, 0.25, 0.5, x))
    rows = [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in (700, 1923)]
    call(f"{tag} resample 24000->8000", lambda: gm.resample(rows, 24000, 8000))
    call(f"{tag} resample 48000->24000", lambda: gm.resample(rows, 48000, 24000))
    for fmt in (pkg.PCM_F32, pkg.PCM_S16, pkg.PCM_ULAW, pkg.PCM_ALAW):
        call(f"{tag} pcm_encode fmt={fmt}", lambda: gm.pcm_encode(rows[1], fmt))


def op_calls():
    rng = np.random.default_rng(11)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    call("op_linear 3x32->1024", lambda: R.op_linear(f32(3, 32), f32(1024, 32), f32(1024)))
    call("op_linear 70x100->37", lambda: R.op_linear(f32(70, 100), f32(37, 100), f32(37)))
    call("op_layernorm 7x512", lambda: R.op_layernorm(f32(7, 512), f32(512), f32(512), 1e-6))
    ang = rng.uniform(0, 6.28, (40, 32))
    call("op_rope 2x16x5x64 pos=17", lambda: R.op_rope(f32(2, 16, 5, 64), np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32), 17))
    for tq, tk, ctx in ((40, 40, -1), (64, 64, 7)):
        posq = np.arange(tk - tq, tk)
        call(f"op_attention_positions tq={tq} tk={tk} ctx={ctx}", lambda: R.op_attention_positions(f32(2, 3, tq, 64), f32(2, 3, tk, 64), f32(2, 3, tk, 64), posq, np.arange(tk), ctx))
    call("op_conv1d_leftpad 16->8 k=3 len=33", lambda: R.op_conv1d_leftpad(f32(2, 16, 33), f32(8, 16, 3), f32(8)))
    call("op_convtr1d_righttrim 16->8 stride=4 len=77", lambda: R.op_convtr1d_righttrim(f32(2, 16, 77), f32(16, 8, 8), f32(8), 4, 1))
    call("op_convtr1d_righttrim depthwise 512 stride=16 len=5", lambda: R.op_convtr1d_righttrim(f32(2, 512, 5), f32(512, 1, 32), None, 16, 512))
    call("op_pcm16 n=9", lambda: R.op_pcm16(f32(9) * 0.7))


def main():
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), encoder=True, speaker_proj=True)
    tensors = synth.make_checkpoint(cfg, seed=1234)
    with tempfile.TemporaryDirectory() as td:
        for dtype, weights in (("F32", pkg.WEIGHTS_F32), ("BF16", pkg.WEIGHTS_BF16)):
            path = os.path.join(td, f"tiny_{dtype}.safetensors")
            synth.write_safetensors(path, tensors, dtype=dtype)
            gm = pkg.Model.open(path, device=0, weights=weights)
            model_calls(dtype, gm, cfg)
            gm.close()
    op_calls()


if __name__ == "__main__":
    main()
