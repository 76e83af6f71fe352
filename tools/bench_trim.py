"""Silence control of a joined call's parts (trim.hip k_trim_mark / k_trim_carry / k_trim_store, generate.cpp generate_joined; DESIGN.md section 8
N3), full-size synthetic checkpoint, bf16, graph step, one device voice.  Legs, run interleaved in one process, whole-call wall clock, median of
--runs rounds after --warmup: (a) ptts_trim_rows on 64 x 10 s host rows (the results of one plain batch, each scaled to a peak of 0.9; upload,
the three kernels, the records back, the kept samples back); (b) ptts_limit_rows on the same rows -- the same kind of round trip with four
kernels, the yardstick; (c) one generate_joined call of a text of 12 chunks of 10 s without a trim -- what profiles/join_bench.json measured
with a chain behind it; (d) the same call with a trim attached (edges and pauses, the threshold at the 99.9th percentile of the audio's own
|x|, capped at 0 dB: the synthetic checkpoint's audio may lie above it, and then all three kernels run over every sample and keep them all).
d - c is what the trim costs a joined call: three launches, one page-locked copy of the records and one stream wait per group, less what the
shorter joined row saves behind it.  No gate: the figures are recorded as seen.  Writes profiles/trim_bench.json (PTTS_OUT_DIR: elsewhere).  --trace-only: a few
calls of leg (a) alone, for a run under `rocprofv3 --kernel-trace --stats` (the per-kernel times)."""
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

CHUNKS = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "trim_bench.json"))
    a = ap.parse_args()
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

    def level_db(xs, q):
        return min(max(20.0 * math.log10(max(float(np.quantile(np.abs(np.concatenate(xs)), q)), 1e-6)), -120.0), 0.0)

    # the rows of legs (a) and (b): each result scaled to a peak of 0.9 (as tools/bench_limiter.py does), so that whatever the checkpoint's level a
    # threshold at the rows' 99.9th percentile lies under 0 dB and the trim has edges and pauses to cut
    rows = [(np.float32(0.9) / np.float32(max(float(np.abs(x).max()), 1e-9)) * x).astype(np.float32) for x in raw]
    db = level_db(rows[:4], 0.999)
    trim = rt.TrimOpts(edges=1, threshold_db=db, pad_ms=30.0, max_pause_ms=20.0)
    # the joined call's parts are the model's own audio: the synthetic checkpoint's level may lie above 0 dB, and then the threshold is capped there
    db_joined = level_db(raw[:4], 0.999)
    trim_joined = rt.TrimOpts(edges=1, threshold_db=db_joined, pad_ms=30.0, max_pause_ms=20.0)
    kept_joined = sum(rt.trim_plan(trim_joined, x).n_out for x in raw[:CHUNKS]) / float(sum(x.size for x in raw[:CHUNKS]))
    del raw
    lim = rt.LimiterOpts(ceiling_db=-6.0, lookahead_ms=1.5, release_ms=80.0)
    ext = rt.DspExt(trim=trim_joined)
    dsp = rt.DspOpts()
    dsp.ext = ext.h
    plain_join, trim_join = rt.JoinOpts(), rt.JoinOpts(dsp=dsp)
    _, recs = model.trim_rows(rows, trim)
    kept = sum(r.n_out for r in recs) / float(sum(x.size for x in rows))
    print(f"rows: {n} x {rows[0].size} samples at peak 0.9; threshold {db:.1f} dB; the trim keeps {100 * kept:.1f} % of the samples, {sum(r.cuts for r in recs)} cuts", flush=True)
    print(f"joined: {CHUNKS} parts; threshold {db_joined:.1f} dB; the trim keeps {100 * kept_joined:.1f} % of the samples", flush=True)
    if a.trace_only:
        for _ in range(3):
            model.trim_rows(rows, trim)
        ext.free()
        voice.close()
        model.close()
        return
    jt, jc = toks[:CHUNKS], cfgs[:CHUNKS]
    legs = {"a_trim_rows_64x10s": lambda: model.trim_rows(rows, trim), "b_limit_rows_64x10s": lambda: model.limit_rows(rows, lim),
            "c_generate_joined_plain": lambda: model.generate_joined(jt, jc, plain_join), "d_generate_joined_trim": lambda: model.generate_joined(jt, jc, trim_join)}
    lat = {k: [] for k in legs}
    for it in range(a.warmup + a.runs):
        for name, leg in legs.items():
            t0 = time.perf_counter()
            y = leg()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    out = {"workload": f"rows: {n} x 10 s; joined: {CHUNKS} chunks x 10 s, bf16, graph step", "runs": a.runs, "warmup": a.warmup, "rows_threshold_db": db,
           "rows_kept_fraction": kept, "rows_cuts": int(sum(r.cuts for r in recs)), "joined_threshold_db": db_joined, "joined_kept_fraction": kept_joined, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:28s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    out["d_minus_c_ms"] = out["calls_ms"]["d_generate_joined_trim"]["median"] - out["calls_ms"]["c_generate_joined_plain"]["median"]
    out["a_minus_b_ms"] = out["calls_ms"]["a_trim_rows_64x10s"]["median"] - out["calls_ms"]["b_limit_rows_64x10s"]["median"]
    print(f"joined: trim - plain = {out['d_minus_c_ms']:+.2f} ms; rows: trim - limiter = {out['a_minus_b_ms']:+.2f} ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ext.free()
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
