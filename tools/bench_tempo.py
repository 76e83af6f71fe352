"""The speaking rate of a joined call's parts (tempo.hip k_tempo_plan / k_tempo_store, generate.cpp generate_joined),
full-size synthetic checkpoint, bf16, graph step, one device voice.  Legs, run interleaved in one process, whole-call wall clock, median of
--runs rounds after --warmup: (a) / (b) ptts_tempo_rows on 64 x 10 s host rows (the results of one plain batch, each scaled to a peak of 0.9)
at speed 800 and 1250 -- upload, the two kernels, the time-scaled rows back; (c) one generate_joined call of a text of 12 chunks of 10 s without a
tempo -- the call tools/bench_trim.py measures; (d) the same call from a handle whose tempo was set and cleared; (e) the same call at speed 1250.
e - c is what the tempo costs a joined call, less what the shorter joined row saves behind it.  The Mimi decode of that one group is read from
the model's phase profile in a call of its own.  No gate: the figures are recorded as seen.  Writes profiles/tempo_bench.json (PTTS_OUT_DIR:
elsewhere).
--trace-only: a few calls of (a), (b) and (e) alone, for a run under `rocprofv3 --kernel-trace --output-format csv` (a run of its own).
--kernels-from DIR: no GPU work; reads the kernel trace below DIR and adds the tempo kernels' times (median, min, max over the dispatches of each
grid) to the JSON."""
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


def kernels_from(trace_dir):
    """{kernel: {"rows x ...": {median_us, min_us, max_us, dispatches}}} of the k_tempo_* dispatches in rocprofv3's kernel trace"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = sorted((r for r in csv.DictReader(f) if "k_tempo_" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        plan_us = None
        for row in rows:   # a launch sequence is k_tempo_plan, then k_tempo_store, whose grid says how long the output is: it names both
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            if "k_tempo_plan" in row["Kernel_Name"]:
                plan_us = us
                continue
            wg = [int(row[f"Grid_Size_{d}"]) // max(int(row[f"Workgroup_Size_{d}"]), 1) for d in "XY"]
            key = f"{wg[1]} rows x {wg[0]} output tiles"
            out.setdefault("k_tempo_store", {}).setdefault(key, []).append(us)
            if plan_us is not None:
                out.setdefault("k_tempo_plan", {}).setdefault(key, []).append(plan_us)
            plan_us = None
    return {k: {g: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)} for g, v in sorted(gs.items())}
            for k, gs in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernels-from", default=None)
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "tempo_bench.json"))
    a = ap.parse_args()
    if a.kernels_from:
        with open(a.out) as f:
            out = json.load(f)
        out["kernels"] = kernels_from(a.kernels_from)
        print(json.dumps(out["kernels"], indent=1))
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
    # the rows of legs (a) and (b): each result scaled to a peak of 0.9 (as tools/bench_trim.py does): the search works on audio inside full scale
    rows = [(np.float32(0.9) / np.float32(max(float(np.abs(x).max()), 1e-9)) * x).astype(np.float32) for x in raw]
    del raw
    slow, fast = rt.TempoOpts(800), rt.TempoOpts(1250)
    spliced = {s: sum(int((np.diff(rt.tempo_plan(rt.TempoOpts(s), x).astype(np.int64)) != 480).sum()) for x in rows[:4]) for s in (800, 1250)}
    hops = {s: sum((rt.tempo_length(rt.TempoOpts(s), x.size) + 479) // 480 for x in rows[:4]) for s in (800, 1250)}
    print(f"rows: {n} x {rows[0].size} samples at peak 0.9; of the first four rows' hops {spliced[800]} / {hops[800]} splice at 800, {spliced[1250]} / {hops[1250]} at 1250", flush=True)

    def joined_opts(tempo, clear=False):
        ext = rt.DspExt(tempo=tempo)
        if clear:
            ext.set_tempo(None)
        dsp = rt.DspOpts()
        dsp.ext = ext.h
        o = rt.JoinOpts(dsp=dsp)
        o._keep = (ext, dsp)
        return o

    plain_join, cleared_join, fast_join = rt.JoinOpts(), joined_opts(fast, clear=True), joined_opts(fast)
    jt, jc = toks[:CHUNKS], cfgs[:CHUNKS]
    if a.trace_only:
        for _ in range(TRACE_CALLS):
            model.tempo_rows(rows, slow)
        for _ in range(TRACE_CALLS):
            model.tempo_rows(rows, fast)
        for _ in range(TRACE_CALLS):
            model.generate_joined(jt, jc, fast_join)
        voice.close()
        model.close()
        return
    legs = {"a_tempo_rows_64x10s_800": lambda: model.tempo_rows(rows, slow), "b_tempo_rows_64x10s_1250": lambda: model.tempo_rows(rows, fast),
            "c_generate_joined_plain": lambda: model.generate_joined(jt, jc, plain_join),
            "d_generate_joined_tempo_cleared": lambda: model.generate_joined(jt, jc, cleared_join),
            "e_generate_joined_tempo_1250": lambda: model.generate_joined(jt, jc, fast_join)}
    lat = {k: [] for k in legs}
    for it in range(a.warmup + a.runs):
        for name, leg in legs.items():
            t0 = time.perf_counter()
            y = leg()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    model.profile_enable(2)   # phases only: the decode of the one group of the joined call
    model.generate_joined(jt, jc, fast_join)
    mimi_ms = model.profile_read()["mimi_ms"]
    model.profile_enable(0)
    out = {"workload": f"rows: {n} x 10 s; joined: {CHUNKS} chunks x 10 s, bf16, graph step", "runs": a.runs, "warmup": a.warmup,
           "spliced_hops_of_first_four_rows": {str(s): [spliced[s], hops[s]] for s in spliced}, "joined_group_mimi_decode_ms": mimi_ms, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:34s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["e_minus_c_ms"] = out["calls_ms"]["e_generate_joined_tempo_1250"]["median"] - out["calls_ms"]["c_generate_joined_plain"]["median"]
    out["d_minus_c_ms"] = out["calls_ms"]["d_generate_joined_tempo_cleared"]["median"] - out["calls_ms"]["c_generate_joined_plain"]["median"]
    print(f"joined: tempo 1250 - plain = {out['e_minus_c_ms']:+.2f} ms; cleared - plain = {out['d_minus_c_ms']:+.2f} ms; the group's Mimi decode {mimi_ms:.2f} ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
