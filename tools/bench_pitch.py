"""The pitch of a joined call's parts (pitch.hip k_pitch_resample, generate.cpp generate_joined), full-size synthetic
checkpoint, bf16, graph step, one device voice.  Legs, run interleaved in one process, whole-call wall clock, median of --runs rounds after
--warmup: (a) / (b) ptts_pitch_rows on 64 x 10 s host rows (the results of one plain batch, each scaled to a peak of 0.9) at pitch 800 and
1250 -- upload, k_pitch_resample, the tempo at the effective speed, the rows back; (c) / (d) the yardstick: ptts_resample in f32 on the same rows
for 24000 -> 30000 and 24000 -> 19200, the two ratios (step 0.8 and 1.25) that k_resample's per-pair tap tables can express too; (e) one
generate_joined call of a text of 12 chunks of 10 s without a pitch; (f) the same call at pitch 1100; legs alternate.  No gate: the figures are
recorded as seen.  Writes profiles/pitch_bench.json (PTTS_OUT_DIR: elsewhere).
--trace-only: a few calls of (a) to (d) alone, for a run under `rocprofv3 --kernel-trace --output-format csv` (a run of its own).
--kernels-from DIR: no GPU work; reads the kernel trace below DIR and adds the times of k_pitch_resample and k_resample (median, min, max over
the dispatches of each grid) and their ratio to the JSON.
--bench-runs FILE: no GPU work; adds the JSON lines of alternating bench.py runs (one line per run, {"tree": "parent" | "this", ...bench.py's
result}) with each tree's median and spread."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = 12
TRACE_CALLS = 5
NAMES = ("k_pitch_resample", "k_resample")


def kernels_from(trace_dir):
    """{kernel: {"rows x tiles": {median_us, min_us, max_us, dispatches}}} of the dispatches of NAMES in rocprofv3's kernel trace"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = next((k for k in NAMES if k in row["Kernel_Name"]), None)   # (neither name is part of the other)
                if name is None:
                    continue
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                wg = [int(row[f"Grid_Size_{d}"]) // max(int(row[f"Workgroup_Size_{d}"]), 1) for d in "XY"]
                out.setdefault(name, {}).setdefault(f"{wg[1]} rows x {wg[0]} output tiles", []).append(us)
    return {k: {g: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)} for g, v in sorted(gs.items())}
            for k, gs in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernels-from", default=None)
    ap.add_argument("--bench-runs", default=None)
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "pitch_bench.json"))
    a = ap.parse_args()
    if a.kernels_from or a.bench_runs:
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
    import bench
    import ptts_amd
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(wl["batch"], 25, 4000, seed=42)]
    n = len(toks)
    cfgs = bench.gen_cfgs(pkg, wl, n, voice)
    raw = [np.array(r.pcm, np.float32) for r in model.generate_batch(toks, cfgs)]
    # the rows of legs (a) to (d): each result scaled to a peak of 0.9 (as tools/bench_tempo.py does): the tempo's search works on audio inside full scale
    rows = [(np.float32(0.9) / np.float32(max(float(np.abs(x).max()), 1e-9)) * x).astype(np.float32) for x in raw]
    del raw
    low, high = rt.PitchOpts(800), rt.PitchOpts(1250)
    print(f"rows: {n} x {rows[0].size} samples at peak 0.9; effective speeds {rt.pitch_speed(low)} and {rt.pitch_speed(high)}", flush=True)

    def joined_opts(pitch):
        ext = rt.DspExt(pitch=pitch)
        dsp = rt.DspOpts()
        dsp.ext = ext.h
        o = rt.JoinOpts(dsp=dsp)
        o._keep = (ext, dsp)
        return o

    plain_join, pitch_join = rt.JoinOpts(), joined_opts(rt.PitchOpts(1100))
    jt, jc = toks[:CHUNKS], cfgs[:CHUNKS]
    rows_legs = {"a_pitch_rows_64x10s_800": lambda: model.pitch_rows(rows, low), "b_pitch_rows_64x10s_1250": lambda: model.pitch_rows(rows, high),
                 "c_resample_64x10s_24000_30000": lambda: model.resample(rows, 24000, 30000), "d_resample_64x10s_24000_19200": lambda: model.resample(rows, 24000, 19200)}
    if a.trace_only:
        for leg in rows_legs.values():
            for _ in range(TRACE_CALLS):
                leg()
        voice.close()
        model.close()
        return
    legs = dict(rows_legs)
    legs["e_generate_joined_plain"] = lambda: model.generate_joined(jt, jc, plain_join)
    legs["f_generate_joined_pitch_1100"] = lambda: model.generate_joined(jt, jc, pitch_join)
    lat = {k: [] for k in legs}
    for it in range(a.warmup + a.runs):
        for name, leg in legs.items():
            t0 = time.perf_counter()
            y = leg()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    out = {"workload": f"rows: {n} x 10 s; joined: {CHUNKS} chunks x 10 s, bf16, graph step", "runs": a.runs, "warmup": a.warmup, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:34s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["f_minus_e_ms"] = out["calls_ms"]["f_generate_joined_pitch_1100"]["median"] - out["calls_ms"]["e_generate_joined_plain"]["median"]
    print(f"joined: pitch 1100 - plain = {out['f_minus_e_ms']:+.2f} ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
