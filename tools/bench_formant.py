"""Keep the formants around the pitch of a joined call's parts (formant.hip k_formant_analyse, k_formant_whiten, k_formant_shape around pitch.hip
k_pitch_resample).  The kernels depend on no weight, so the model is the tiny synthetic checkpoint and the rows are
synthetic: 64 x 10 s of a pulse train through three resonators plus noise, peak 0.5.  Legs, run interleaved in one process, whole-call wall clock
(upload, kernels, the tempo at the effective speed, the rows back; the call ends in a stream wait), median of --runs rounds after --warmup:
(a) ptts_pitch_rows at pitch 1250; (b) ptts_formant_rows at pitch 1250 with the option.  No gate: the figures are recorded as seen.  Writes
profiles/formant_bench.json (PTTS_OUT_DIR: elsewhere).
--trace-only: a few calls of (a) and (b) alone, for a run under `rocprofv3 --kernel-trace --output-format csv` (a run of its own).
--kernels-from DIR: no GPU work; reads the kernel trace below DIR and adds the times of the three formant kernels, k_pitch_resample and the tempo's
kernels (median, min, max over the dispatches of each grid) to the JSON.
--bench-runs FILE: no GPU work; adds the JSON lines of alternating bench.py runs (one line per run, {"tree": "parent" | "this", ...bench.py's
result}) with each tree's median and spread."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, SAMPLES = 64, 240000
TRACE_CALLS = 5
NAMES = ("k_formant_analyse", "k_formant_whiten", "k_formant_shape", "k_pitch_resample", "k_tempo_plan", "k_tempo_store")


def kernels_from(trace_dir):
    """{kernel: {"workgroups x by y": {median_us, min_us, max_us, dispatches}}} of the dispatches of NAMES in rocprofv3's kernel trace"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = next((k for k in NAMES if k in row["Kernel_Name"]), None)
                if name is None:
                    continue
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                wg = [int(row[f"Grid_Size_{d}"]) // max(int(row[f"Workgroup_Size_{d}"]), 1) for d in "XY"]
                out.setdefault(name, {}).setdefault(f"{wg[1]} rows x {wg[0]} workgroups", []).append(us)
    return {k: {g: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)} for g, v in sorted(gs.items())}
            for k, gs in sorted(out.items())}


def make_rows():
    """ROWS rows of SAMPLES samples: a pulse train (f0 from 90 to 250 Hz) through three two-pole resonators, plus a little noise, peak 0.5"""
    rng = np.random.default_rng(7)
    rows = []
    for i in range(ROWS):
        f0 = 90.0 + 2.5 * i
        x = np.zeros(SAMPLES)
        x[(np.arange(0.0, SAMPLES, 24000.0 / f0)).astype(np.int64)] = 1.0
        x += 0.01 * rng.standard_normal(SAMPLES)
        spec = np.fft.rfft(x)
        z = np.exp(-2j * np.pi * np.arange(spec.size) / SAMPLES)
        for hz, bw in ((500.0 + 5 * i, 80.0), (1500.0, 100.0), (2600.0, 140.0)):
            r = np.exp(-np.pi * bw / 24000.0)
            spec = spec / (1.0 - 2.0 * r * np.cos(2.0 * np.pi * hz / 24000.0) * z + r * r * z * z)
        y = np.fft.irfft(spec, SAMPLES)
        rows.append((y * (0.5 / np.abs(y).max())).astype(np.float32))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernels-from", default=None)
    ap.add_argument("--bench-runs", default=None)
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "formant_bench.json"))
    a = ap.parse_args()
    if a.kernels_from or a.bench_runs:
        if not os.path.exists(a.out):
            sys.exit(f"{a.out} is missing: run the timing legs first (no --kernels-from / --bench-runs), which write it")
        with open(a.out) as f:
            out = json.load(f)
        if a.kernels_from:
            out["kernels"] = kernels_from(a.kernels_from)
            print(json.dumps(out["kernels"], indent=1))
        if a.bench_runs:
            with open(a.bench_runs) as f:
                runs = [json.loads(line) for line in f if line.strip().startswith("{")]
            out["bench_py"] = {}
            for tree in ("parent", "this"):
                v = [r["value"] for r in runs if r.get("tree") == tree]
                if v:
                    out["bench_py"][tree] = {"values": v, "median": statistics.median(v), "min": min(v), "max": max(v), "unit": runs[0].get("unit")}
            print(json.dumps(out["bench_py"], indent=1))
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        return
    import ptts_amd
    pkg = ptts_amd.load()
    rt = pkg.runtime
    synth = pkg.synth
    td = tempfile.TemporaryDirectory()   # (the checkpoint stays while the model is open)
    path = os.path.join(td.name, "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(synth.SynthConfig.tiny(), seed=1234))
    model = pkg.Model.open(path, device=0)
    rows = make_rows()
    keep, high = rt.FormantOpts(1), rt.PitchOpts(1250)
    print(f"rows: {len(rows)} x {rows[0].size} samples at peak 0.5; pitch 1250, effective speed {rt.pitch_speed(high)}", flush=True)
    legs = {"a_pitch_rows_64x10s_1250": lambda: model.pitch_rows(rows, high), "b_formant_rows_64x10s_1250": lambda: model.formant_rows(rows, keep, high)}
    if a.trace_only:
        for leg in legs.values():
            for _ in range(TRACE_CALLS):
                leg()
        model.close()
        return
    lat = {k: [] for k in legs}
    for it in range(a.warmup + a.runs):
        for name, leg in legs.items():
            t0 = time.perf_counter()
            y = leg()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    out = {"workload": f"rows: {len(rows)} x 10 s synthetic vowels, pitch 1250, tempo at {rt.pitch_speed(high)}", "runs": a.runs, "warmup": a.warmup, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:34s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["b_minus_a_ms"] = out["calls_ms"]["b_formant_rows_64x10s_1250"]["median"] - out["calls_ms"]["a_pitch_rows_64x10s_1250"]["median"]
    print(f"rows: with the option - without = {out['b_minus_a_ms']:+.2f} ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    model.close()


if __name__ == "__main__":
    main()
