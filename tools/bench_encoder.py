"""Micro-benchmark of the Mimi encoder (PARITY UNPINNED: inferred architecture): ms per clip for 10-s and 30-s clips and for
one call of 8 x 10 s, full-size synthetic checkpoint (f = 64, 2 transformer layers), bf16 weights, HIP-synchronous host timing around
Model.encode_audio (host -> device PCM and device -> host latents included).  Prints one JSON line; --out also writes it to a file.

    python3 tools/bench_encoder.py [--iters 20] [--warmup 3] [--out bench_encoder.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ptts_amd
    pkg = ptts_amd.load()
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.full(), encoder=True)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "full_enc.safetensors")
        synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1), dtype="BF16" if a.weights == "bf16" else "F32")
        gm = pkg.Model.open(path, device=0, weights=pkg.WEIGHTS_BF16 if a.weights == "bf16" else pkg.WEIGHTS_F32)
    rng = np.random.default_rng(0)
    clip = lambda s: (0.2 * rng.standard_normal(s * 24000)).astype(np.float32)
    cases = {"10s": [clip(10)], "30s": [clip(30)], "8x10s": [clip(10) for _ in range(8)]}
    res = {"metric": "mimi_encoder_ms_per_clip", "weights": a.weights, "iters": a.iters, "parity": "unpinned (inferred architecture)"}
    for name, clips in cases.items():
        arg = clips if len(clips) > 1 else clips[0]
        for _ in range(a.warmup):
            gm.encode_audio(arg)
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            gm.encode_audio(arg)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        res[name] = {"ms_per_call_median": round(float(np.median(ts)), 3), "ms_per_call_min": round(float(ts.min()), 3),
                     "ms_per_clip_median": round(float(np.median(ts)) / len(clips), 3), "clips": len(clips)}
    gm.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
