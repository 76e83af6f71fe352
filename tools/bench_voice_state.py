"""Cloned voice given as an embedding (prefilled again by every request) versus as a device voice built once (ptts_voice_from_embeddings), and
the cost of ptts_voice_from_audio.  Full-size synthetic checkpoint with the encoder and speaker projection, bf16 weights and bf16 KV, graph replay:
- one 64-request batch of 10 s (125 frames, 25-token prompts) with a 125-frame voice, as voice_embedding vs as device_voice;
- ptts_voice_from_audio for 1 and for 8 ten-second clips (encoder + projection + one model-state build; PARITY UNPINNED encoder).
HIP-synchronous host timing of whole calls; prints one JSON line (--out also writes it).

    python3 tools/bench_voice_state.py [--iters 7] [--warmup 2] [--out profiles/voice_state_bench.json]
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(float(ts.min()), 3), "ms_max": round(float(ts.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ptts_amd
    pkg = ptts_amd.load()
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.full(), encoder=True, speaker_proj=True)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "full_enc.safetensors")
        synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1), dtype="BF16")
        gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_BF16, kv=pkg.KV_BF16, max_batch=64, use_graph=True)
    rng = np.random.default_rng(0)
    clip = lambda: (0.2 * rng.standard_normal(10 * 24000)).astype(np.float32)
    ref_clip = clip()
    emb = gm.voice_from_audio(ref_clip)                    # [1, 125, 1024]
    dv = gm.voice_from_embedding(emb)
    frames = 125
    toks = [p.tolist() for p in synth.make_prompts(64, 25, 4000, seed=42)]
    base = dict(temperature=0.0, eos_threshold=float("inf"), max_steps=frames, lsd_decode_steps=1, frames_after_eos=3)
    as_emb = [pkg.RuntimeGenerateConfig(voice_embedding=emb, **base) for _ in toks]
    as_dev = [pkg.RuntimeGenerateConfig(device_voice=dv, **base) for _ in toks]
    res = {"metric": "cloned_voice_ms_per_call", "weights": "bf16", "kv": "bf16", "use_graph": True, "iters": a.iters, "voice_frames": int(emb.shape[1]),
           "batch": 64, "frames": frames}
    # interleaved, so that drift affects both alike
    e_ts, d_ts = [], []
    for _ in range(a.warmup):
        gm.generate_batch(toks, as_emb)
        gm.generate_batch(toks, as_dev)
    for _ in range(a.iters):
        e_ts.append(timed(lambda: gm.generate_batch(toks, as_emb), 1, 0)["ms_median"])
        d_ts.append(timed(lambda: gm.generate_batch(toks, as_dev), 1, 0)["ms_median"])
    sm = lambda ts: {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(float(np.min(ts)), 3), "ms_max": round(float(np.max(ts)), 3)}
    res["b64_10s_voice_embedding"] = sm(e_ts)
    res["b64_10s_device_voice"] = sm(d_ts)
    res["device_voice_speedup"] = round(float(np.median(e_ts)) / float(np.median(d_ts)), 4)
    one = [ref_clip]
    eight = [clip() for _ in range(8)]
    free_all = lambda vs: [v.close() for v in vs]
    res["voice_from_audio_1x10s"] = timed(lambda: free_all(gm.voice_state_from_audio(one)), a.iters, a.warmup)
    res["voice_from_audio_8x10s"] = timed(lambda: free_all(gm.voice_state_from_audio(eight)), a.iters, a.warmup)
    res["voice_from_embedding_1x125"] = timed(lambda: gm.voice_from_embedding(emb).close(), a.iters, a.warmup)
    dv.close()
    gm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
