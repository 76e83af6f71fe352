"""The true-peak ceiling on the device (true_peak.hip k_tp_peak / k_tp_scale) on the headline workload: 64 x 10 s, bf16, graph
step, one device voice.  Legs, run interleaved in one process, whole-call median of --runs rounds after --warmup: (a) no post-processing; (b) loudness
-16 LUFS and a ceiling of -1 dBTP, native f32; (c) the same as 8 kHz mu-law; (d) leg (a) followed by ptts_true_peak_limit on the host over the 64
results, one thread -- what the device stage replaces; (e) ptts_true_peak_rows on 64 x 10 s host rows.  Writes profiles/true_peak_bench.json
(PTTS_OUT_DIR: elsewhere).  --trace-only: a few calls of leg (b) alone, for a run under `rocprofv3 --kernel-trace --stats` (the per-kernel times of
profiles/true_peak_by_kernel.txt)."""
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

LOUDNESS, CEILING = -1600, -1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "true_peak_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(wl["batch"], 25, 4000, seed=42)]
    n = len(toks)
    legs = {"a_plain": bench.gen_cfgs(pkg, wl, n, voice),
            "b_loudness_ceiling_f32": bench.gen_cfgs(pkg, wl, n, voice, loudness=LOUDNESS, true_peak_dbtp=CEILING),
            "c_loudness_ceiling_8k_ulaw": bench.gen_cfgs(pkg, wl, n, voice, sample_rate=8000, g711="ulaw", loudness=LOUDNESS, true_peak_dbtp=CEILING)}
    if a.trace_only:
        for _ in range(3):
            model.generate_batch(toks, legs["b_loudness_ceiling_f32"])
        voice.close()
        model.close()
        return
    lat = {k: [] for k in list(legs) + ["d_plain_then_host_limit", "d_host_limit_alone", "e_true_peak_rows_64x10s"]}
    rows = None
    for it in range(a.warmup + a.runs):
        for name, cfgs in legs.items():
            t0 = time.perf_counter()
            res = model.generate_batch(toks, cfgs)
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del res
        t0 = time.perf_counter()
        res = model.generate_batch(toks, legs["a_plain"])
        t1 = time.perf_counter()
        post = [rt.true_peak_limit(r.pcm, CEILING)[0] for r in res]
        t2 = time.perf_counter()
        if rows is None:
            rows = [np.array(r.pcm, copy=True) for r in res]
        del res, post
        t3 = time.perf_counter()
        model.true_peak_rows(rows)
        t4 = time.perf_counter()
        if it >= a.warmup:
            lat["d_plain_then_host_limit"].append(1e3 * (t2 - t0))
            lat["d_host_limit_alone"].append(1e3 * (t2 - t1))
            lat["e_true_peak_rows_64x10s"].append(1e3 * (t4 - t3))
    out = {"workload": "b64_10s_bf16", "runs": a.runs, "warmup": a.warmup, "loudness": LOUDNESS, "ceiling_dbtp": CEILING, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{k:28s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["b_minus_a_ms"] = out["calls_ms"]["b_loudness_ceiling_f32"]["median"] - out["calls_ms"]["a_plain"]["median"]
    out["c_minus_a_ms"] = out["calls_ms"]["c_loudness_ceiling_8k_ulaw"]["median"] - out["calls_ms"]["a_plain"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
