"""The per-request limiter on the device (limiter.hip k_lim_*) on the headline workload: 64 x 10 s, bf16, graph step, one
device voice.  Legs, run interleaved in one process, whole-call median of --runs rounds after --warmup: (a) no post-processing; (b) a limiter
per request (ceiling 6 dB under the first result's peak, 1.5 ms ahead, 80 ms release), native f32; (c) a limiter at -6 dBFS behind loudness -16 LUFS as
8 kHz mu-law; (d) leg (a) followed by ptts_limit_apply on the host over the 64 results, one thread -- what the device stage replaces; (e)
ptts_limit_rows on 64 x 10 s host rows (the results of leg (a), each scaled to a peak of 0.9; ceiling -6 dB, so the limiter works on most
crests); (f) ptts_compress_rows on the same rows -- the same kind of passes, the yardstick.  Writes profiles/limiter_bench.json (PTTS_OUT_DIR:
elsewhere).  --trace-only: one plain call, then a few calls of legs (e) and (f) alone, for a run under `rocprofv3 --kernel-trace --stats` (the
per-kernel times of profiles/limiter_by_kernel.txt)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ptts_amd  # noqa: E402

LOUDNESS = -1600


def _rows(res):
    """The results as host rows for legs (e) and (f), each scaled to a peak of 0.9: whatever the checkpoint's level, the crests are well above
    the limiter's ceiling and the compressor's threshold."""
    return [(np.float32(0.9) / np.float32(max(float(np.abs(r.pcm).max()), 1e-9)) * r.pcm).astype(np.float32) for r in res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "limiter_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(wl["batch"], 25, 4000, seed=42)]
    n = len(toks)
    plain = bench.gen_cfgs(pkg, wl, n, voice)
    first = model.generate_batch(toks, plain)
    peak = max(float(np.abs(r.pcm).max()) for r in first)
    lim = rt.LimiterOpts(ceiling_db=min(max(20.0 * math.log10(max(peak, 1e-9)) - 6.0, -60.0), 0.0), lookahead_ms=1.5, release_ms=80.0)
    lim_rows = rt.LimiterOpts(ceiling_db=-6.0, lookahead_ms=1.5, release_ms=80.0)
    comp = rt.CompressorOpts(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0)
    rows = _rows(first)
    del first
    legs = {"a_plain": plain,
            "b_limiter_f32": bench.gen_cfgs(pkg, wl, n, voice, limiter=lim),
            "c_loudness_limiter_8k_ulaw": bench.gen_cfgs(pkg, wl, n, voice, sample_rate=8000, g711="ulaw", loudness=LOUDNESS, limiter=lim_rows)}
    if a.trace_only:
        for _ in range(3):
            model.limit_rows(rows, lim_rows)
            model.compress_rows(rows, comp)
        voice.close()
        model.close()
        return
    lat = {k: [] for k in list(legs) + ["d_plain_then_host_limit", "d_host_limit_alone", "e_limit_rows_64x10s", "f_compress_rows_64x10s"]}
    said = False
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
        post = [rt.limit_apply(lim, r.pcm) for r in res]
        t2 = time.perf_counter()
        if not said:
            moved = float(np.mean([float((p != r.pcm).mean()) for p, r in zip(post, res)]))
            row_moved = float(np.mean([float((rt.limit_apply(lim_rows, x) != x).mean()) for x in rows[:4]]))
            print(f"results: {len(res)} x {res[0].pcm.size} samples, peak {peak:.3f}; the request's limiter changes {100 * moved:.1f} % of the samples, "
                  f"the rows' limiter {100 * row_moved:.1f} %", flush=True)
            said = True
        del res, post
        t3 = time.perf_counter()
        model.limit_rows(rows, lim_rows)
        t4 = time.perf_counter()
        model.compress_rows(rows, comp)
        t5 = time.perf_counter()
        if it >= a.warmup:
            lat["d_plain_then_host_limit"].append(1e3 * (t2 - t0))
            lat["d_host_limit_alone"].append(1e3 * (t2 - t1))
            lat["e_limit_rows_64x10s"].append(1e3 * (t4 - t3))
            lat["f_compress_rows_64x10s"].append(1e3 * (t5 - t4))
    out = {"workload": "b64_10s_bf16", "runs": a.runs, "warmup": a.warmup, "loudness": LOUDNESS, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{k:30s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["b_minus_a_ms"] = out["calls_ms"]["b_limiter_f32"]["median"] - out["calls_ms"]["a_plain"]["median"]
    out["c_minus_a_ms"] = out["calls_ms"]["c_loudness_limiter_8k_ulaw"]["median"] - out["calls_ms"]["a_plain"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
