"""Rate and format egress (k_resample) on the headline workload: 64 x 10 s, bf16, graph step, one device voice, run as
native f32 and as 48 kHz f32, 44.1 kHz PCM16, 16 kHz PCM16 and 8 kHz mu-law; whole-call median of --runs calls after --warmup.  Also
ptts_resample of 8 x 10 s from 48 kHz to 24 kHz.  Writes profiles/resample_bench.json.  k_resample's device time per launch comes from a
separate run under `rocprofv3 --kernel-trace --stats` (--trace-only: the converted passes alone, a few calls)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ptts_amd  # noqa: E402

CASES = [("native_f32", dict()), ("48k_f32", dict(sample_rate=48000)), ("44k1_pcm16", dict(sample_rate=44100, pcm16=True)),
         ("16k_pcm16", dict(sample_rate=16000, pcm16=True)), ("8k_ulaw", dict(sample_rate=8000, g711="ulaw")),
         # a mixed group: 32 native f32 rows beside 32 rows of 8 kHz mu-law.  One converting row turns the decoder's direct store off for the
         # group, so the native rows take the device buffer and a copy (same bits): this case measures what that costs
         ("mixed_f32_8k_ulaw", None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(wl["batch"], 25, 4000, seed=42)]
    runs, warmup = (3, 1) if a.trace_only else (a.runs, a.warmup)
    out = {"workload": "b64_10s_bf16", "runs": runs, "warmup": warmup, "calls_ms": {}}
    for name, kw in CASES:
        if a.trace_only and name == "native_f32":
            continue
        if kw is None:
            half = len(toks) // 2
            cfgs = bench.gen_cfgs(pkg, wl, half, voice) + bench.gen_cfgs(pkg, wl, len(toks) - half, voice, sample_rate=8000, g711="ulaw")
        else:
            cfgs = bench.gen_cfgs(pkg, wl, len(toks), voice, **kw)
        for _ in range(warmup):
            res = model.generate_batch(toks, cfgs)
        lat = []
        for _ in range(runs):
            t0 = time.perf_counter()
            res = model.generate_batch(toks, cfgs)
            lat.append(1e3 * (time.perf_counter() - t0))
        for r, c in zip(res, cfgs):
            assert r.pcm.size == wl["frames"] * 8 * (c.sample_rate or 24000) // 100
        out["calls_ms"][name] = {"median": statistics.median(lat), "min": min(lat), "max": max(lat),
                                 "bytes_to_host": int(sum(r.pcm.nbytes for r in res))}
        print(f"{name:12s} median {statistics.median(lat):8.2f} ms  min {min(lat):8.2f}  max {max(lat):8.2f}", flush=True)
        del res
    x = [np.random.default_rng(i).standard_normal(480000).astype(np.float32) * 0.1 for i in range(8)]
    model.resample(x, 48000, 24000)
    lat = []
    for _ in range(runs):
        t0 = time.perf_counter()
        model.resample(x, 48000, 24000)
        lat.append(1e3 * (time.perf_counter() - t0))
    out["resample_8x10s_48k_to_24k_ms"] = {"median": statistics.median(lat), "min": min(lat)}
    print(f"ptts_resample 8 x 10 s 48k->24k: median {statistics.median(lat):.2f} ms", flush=True)
    if not a.trace_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
