"""The per-request de-esser on the device (deesser.hip k_de_*) against its yardstick, the compressor: one call of
ptts_deess_rows and one of ptts_compress_rows on the same 64 host rows of 10 s (a 200 Hz tone with bursts of high-passed noise, peak 0.9, so that
both stages work on most of the row), interleaved in one process, whole-call median of --runs rounds after --warmup.  The rows need no checkpoint's
audio, so the tiny synthetic model carries the call.  Writes profiles/deesser_bench.json (PTTS_OUT_DIR: elsewhere).  --trace-only: a few calls of
each alone, for a run under `rocprofv3 --kernel-trace --stats` (the per-kernel times)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ptts_amd  # noqa: E402

ROWS, SECONDS, RATE = 64, 10, 24000


def _rows(rt):
    n = SECONDS * RATE
    t = np.arange(n) / RATE
    hp = rt.Eq([(2, 6000.0, 0.0, 0.7071)])
    out = []
    for i in range(ROWS):
        rng = np.random.default_rng(100 + i)
        hiss = hp.apply(rng.standard_normal(n).astype(np.float32)).astype(np.float64)
        hiss *= 0.45 / float(np.abs(hiss).max())
        on = (np.arange(n) + 531 * i) % 4800 < 1440
        x = 0.45 * np.sin(2 * np.pi * (180.0 + i) * t) + np.where(on, hiss, 0.0)
        out.append((0.9 / float(np.abs(x).max()) * x).astype(np.float32))
    hp.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "deesser_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    synth = pkg.synth
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "tiny.safetensors")
        synth.write_safetensors(path, synth.make_checkpoint(synth.SynthConfig.tiny(), seed=1234))
        model = pkg.Model.open(path, device=0)
        try:
            measure(a, rt, model)
        finally:
            model.close()


def measure(a, rt, model):
    rows = _rows(rt)
    de = rt.DeesserOpts(freq_hz=5000.0, q=0.7071, threshold_db=-30.0, ratio=4.0, knee_db=6.0, attack_ms=1.0, release_ms=60.0, max_reduction_db=12.0)
    comp = rt.CompressorOpts(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0)
    if a.trace_only:
        for _ in range(3):
            model.deess_rows(rows, de)
            model.compress_rows(rows, comp)
        return
    moved = float(np.mean([float((rt.deess_apply(de, x) != x).mean()) for x in rows[:4]]))
    squeezed = float(np.mean([float((rt.compress_apply(comp, x) != x).mean()) for x in rows[:4]]))
    print(f"rows: {len(rows)} x {rows[0].size} samples; the de-esser changes {100 * moved:.1f} % of the samples, the compressor {100 * squeezed:.1f} %", flush=True)
    lat = {"deess_rows_64x10s": [], "compress_rows_64x10s": []}
    for it in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        model.deess_rows(rows, de)
        t1 = time.perf_counter()
        model.compress_rows(rows, comp)
        t2 = time.perf_counter()
        if it >= a.warmup:
            lat["deess_rows_64x10s"].append(1e3 * (t1 - t0))
            lat["compress_rows_64x10s"].append(1e3 * (t2 - t1))
    out = {"rows": ROWS, "seconds": SECONDS, "runs": a.runs, "warmup": a.warmup, "deesser_moves": moved, "compressor_moves": squeezed, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{k:24s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["ratio"] = out["calls_ms"]["deess_rows_64x10s"]["median"] / out["calls_ms"]["compress_rows_64x10s"]["median"]
    print(f"de-esser / compressor = {out['ratio']:.2f}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
