"""Per-part prosody in a joined call (join.hip k_join_gain, dsp_device.cpp level_launch, generate.cpp generate_joined) on the
text of tools/bench_join.py: 12 chunks of 10 s, full-size synthetic checkpoint, bf16, graph step, one device voice, f32 at 24 kHz and no chain.  Leg
(a): generate_joined without a list (k_join).  Leg (b): a list with a fixed gain on every part (k_join_gain).  Leg (c): a list with a level on every
part (the loudness rows' measuring launches, then k_join_gain reading their words).  Every call ends in a device synchronise; the legs alternate after
--warmup rounds, --runs rounds are timed (wall clock).  Writes profiles/join_parts_bench.json (PTTS_OUT_DIR: elsewhere).
--trace-only: a few calls of each leg alone, for a run under `rocprofv3 --kernel-trace --output-format csv` (a run of its own).
--summarise DIR: the dispatches of the join and measuring kernels in that run's trace, into the same file."""
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

CHUNKS, LEVEL, TRACE_CALLS = 12, -1600, 3
NAMES = ("k_join_gain", "k_join", "k_dsp_peak", "k_loud_summary", "k_loud_carry", "k_loud_energy", "k_loud_gate")


def kernels_from(trace_dir):
    """{kernel: {"rows x workgroups": {median_us, min_us, max_us, dispatches}}} of the dispatches of NAMES in rocprofv3's kernel trace"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = next((k for k in NAMES if k + "E" in row["Kernel_Name"] or k + "(" in row["Kernel_Name"]), None)
                if name is None:
                    continue
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                wg = [int(row[f"Grid_Size_{d}"]) // max(int(row[f"Workgroup_Size_{d}"]), 1) for d in "XY"]
                out.setdefault(name, {}).setdefault(f"{wg[1]} rows x {wg[0]} workgroups", []).append(us)
    return {k: {g: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)} for g, v in sorted(gs.items())}
            for k, gs in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "join_parts_bench.json"))
    a = ap.parse_args()
    if a.summarise:
        out = json.load(open(a.out)) if os.path.exists(a.out) else {}
        out["kernels_us"] = kernels_from(a.summarise)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
        print(json.dumps(out["kernels_us"], indent=1))
        return
    import bench
    import ptts_amd
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(CHUNKS, 25, 4000, seed=42)]
    cfgs = bench.gen_cfgs(pkg, wl, CHUNKS, voice)
    join = rt.JoinOpts(gap_ms=37.5)
    gains = [rt.PartOpts(gain_db=(-6.0 if i % 2 else 3.0)) for i in range(CHUNKS)]
    levels = [rt.PartOpts(level=LEVEL) for _ in range(CHUNKS)]
    legs = {"a_no_list": lambda: model.generate_joined(toks, cfgs, join), "b_fixed_gains": lambda: model.generate_joined(toks, cfgs, join, parts=gains),
            "c_levels": lambda: model.generate_joined(toks, cfgs, join, parts=levels)}
    first = {k: f() for k, f in legs.items()}
    g = first["c_levels"].gains
    print(f"text: {CHUNKS} chunks, {first['a_no_list'].pcm.size / 24000:.1f} s; level gains {float(g.min()):.4f} .. {float(g.max()):.4f}; "
          f"lengths equal: {len({r.pcm.size for r in first.values()}) == 1}", flush=True)
    if a.trace_only:
        for _ in range(TRACE_CALLS):
            for f in legs.values():
                f()
        voice.close()
        model.close()
        return
    lat = {k: [] for k in legs}
    for it in range(a.warmup + a.runs):
        for name, f in legs.items():
            t0 = time.perf_counter()
            y = f()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    out = {"workload": f"{CHUNKS} chunks x 10 s, bf16, graph step, gap 37.5 ms, f32 at 24 kHz, no chain; (b) +3 / -6 dB alternating, (c) level {LEVEL / 100.0} LUFS",
           "runs": a.runs, "warmup": a.warmup, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:16s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
