"""The per-request compressor on the device (compressor.hip k_cmp_*) on the headline workload: 64 x 10 s, bf16, graph step,
one device voice.  Legs, run interleaved in one process, whole-call median of --runs rounds after --warmup: (a) no post-processing; (b) a
compressor per request (-24 dB, ratio 4, 6 dB knee, 5 / 120 ms), native f32; (c) the compressor in front of loudness -16 LUFS as 8 kHz mu-law;
(d) leg (a) followed by ptts_compress_apply on the host over the 64 results, one thread -- what the device stage replaces; (e)
ptts_compress_rows on 64 x 10 s host rows (the results of leg (a), each scaled to a peak of 0.9); (f) ptts_eq_rows with a four-section equaliser on the same rows -- the same kind of passes, the
yardstick.  Writes profiles/compressor_bench.json (PTTS_OUT_DIR: elsewhere).  --trace-only: one plain call, then a few calls of legs (e) and (f)
alone, for a run under `rocprofv3 --kernel-trace --stats` (the per-kernel times of profiles/compressor_bench.txt)."""
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

LOUDNESS = -1600
EQ = [(2, 80.0, 0.0, 0.7071), (5, 400.0, -4.0, 2.0), (5, 3000.0, 6.0, 1.0), (4, 8000.0, 3.0, 0.7071)]   # high-pass, two peaks, a high shelf


def _rows(res):
    """The results as host rows for legs (e) and (f), each scaled to a peak of 0.9: whatever the checkpoint's level, the detector is well above
    the threshold and the curve is evaluated on most samples."""
    return [(np.float32(0.9) / np.float32(max(float(np.abs(r.pcm).max()), 1e-9)) * r.pcm).astype(np.float32) for r in res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "compressor_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(wl["batch"], 25, 4000, seed=42)]
    n = len(toks)
    comp = rt.CompressorOpts(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0)
    eq = rt.Eq(EQ)
    legs = {"a_plain": bench.gen_cfgs(pkg, wl, n, voice),
            "b_compressor_f32": bench.gen_cfgs(pkg, wl, n, voice, compressor=comp),
            "c_compressor_loudness_8k_ulaw": bench.gen_cfgs(pkg, wl, n, voice, sample_rate=8000, g711="ulaw", loudness=LOUDNESS, compressor=comp)}
    if a.trace_only:
        rows = _rows(model.generate_batch(toks, legs["a_plain"]))
        for _ in range(3):
            model.compress_rows(rows, comp)
            model.eq_rows(rows, eq)
        voice.close()
        model.close()
        return
    lat = {k: [] for k in list(legs) + ["d_plain_then_host_compress", "d_host_compress_alone", "e_compress_rows_64x10s", "f_eq_rows_64x10s"]}
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
        post = [rt.compress_apply(comp, r.pcm) for r in res]
        t2 = time.perf_counter()
        if rows is None:
            moved = max(float(np.abs(p - r.pcm).max()) for p, r in zip(post, res))
            print(f"results: {len(res)} x {res[0].pcm.size} samples, peak {max(float(np.abs(r.pcm).max()) for r in res):.3f}, the compressor moves them by {moved:.3e}", flush=True)
            rows = _rows(res)
        del res, post
        t3 = time.perf_counter()
        model.compress_rows(rows, comp)
        t4 = time.perf_counter()
        model.eq_rows(rows, eq)
        t5 = time.perf_counter()
        if it >= a.warmup:
            lat["d_plain_then_host_compress"].append(1e3 * (t2 - t0))
            lat["d_host_compress_alone"].append(1e3 * (t2 - t1))
            lat["e_compress_rows_64x10s"].append(1e3 * (t4 - t3))
            lat["f_eq_rows_64x10s"].append(1e3 * (t5 - t4))
    out = {"workload": "b64_10s_bf16", "runs": a.runs, "warmup": a.warmup, "loudness": LOUDNESS, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{k:30s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["b_minus_a_ms"] = out["calls_ms"]["b_compressor_f32"]["median"] - out["calls_ms"]["a_plain"]["median"]
    out["c_minus_a_ms"] = out["calls_ms"]["c_compressor_loudness_8k_ulaw"]["median"] - out["calls_ms"]["a_plain"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    eq.free()
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
