"""Joined synthesis (join.hip k_join, generate.cpp generate_joined) against the route a host had before it, for the same
bytes: one text of 12 chunks of 10 s, full-size synthetic checkpoint, bf16, graph step, one device voice; loudness -16 LUFS, a limiter at -6 dBFS,
8 kHz mu-law.  Route A: generate_batch of the chunks, the concatenation on the host, ptts_loudness_normalize_rows and ptts_dsp_rows (the limiter) on
it, ptts_resample, ptts_pcm_encode -- four round trips of the text over PCIe behind the first.  Route B: one generate_joined call.  Every call
ends in a device synchronise; the routes alternate after --warmup rounds, --runs rounds are timed (wall clock), and the two results are compared
byte for byte once.  Writes profiles/join_bench.json (PTTS_OUT_DIR: elsewhere).  --trace-only: a few calls of each route alone, for a run under
`rocprofv3 --kernel-trace --stats`."""
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

LOUDNESS, CHUNKS, RATE = -1600, 12, 8000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "join_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(CHUNKS, 25, 4000, seed=42)]
    cfgs = bench.gen_cfgs(pkg, wl, CHUNKS, voice)
    lim = rt.LimiterOpts(ceiling_db=-6.0, lookahead_ms=1.5, release_ms=80.0)
    ext = rt.DspExt(limiter=lim)
    dsp = rt.DspOpts()
    dsp.ext = ext.h
    join = rt.JoinOpts(loudness=LOUDNESS, dsp=dsp, sample_rate=RATE, pcm_format=pkg.PCM_ULAW)

    def route_a():
        whole = np.concatenate([r.pcm for r in model.generate_batch(toks, cfgs)])
        whole, _ = model.loudness_normalize_rows(whole, LOUDNESS / 100.0)
        whole = model.dsp_rows(whole, opts=dsp)
        return model.pcm_encode(model.resample(whole, 24000, RATE), pkg.PCM_ULAW)

    def route_b():
        return model.generate_joined(toks, cfgs, join).pcm

    ya, yb = route_a(), route_b()
    same = ya.dtype == yb.dtype and ya.size == yb.size and bool(np.array_equal(ya, yb))
    print(f"text: {CHUNKS} chunks x {wl['frames']} frames = {yb.size / RATE:.1f} s as {yb.size} mu-law bytes; the two routes give the same bytes: {same}", flush=True)
    if a.trace_only:
        for _ in range(3):
            route_a()
            route_b()
        ext.free()
        voice.close()
        model.close()
        return
    lat = {"a_batch_host_concat_rows": [], "b_generate_joined": []}
    for it in range(a.warmup + a.runs):
        for name, route in (("a_batch_host_concat_rows", route_a), ("b_generate_joined", route_b)):
            t0 = time.perf_counter()
            y = route()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= a.warmup:
                lat[name].append(dt)
            del y
    out = {"workload": f"{CHUNKS} chunks x 10 s, bf16, graph step, loudness {LOUDNESS / 100.0} LUFS + limiter -6 dBFS + {RATE} Hz mu-law", "runs": a.runs,
           "warmup": a.warmup, "same_bytes": same, "calls_ms": {}}
    for k, v in lat.items():
        out["calls_ms"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
        print(f"{k:28s} median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}", flush=True)
    ma, mb = out["calls_ms"]["a_batch_host_concat_rows"], out["calls_ms"]["b_generate_joined"]
    out["a_spread_ms"] = ma["max"] - ma["min"]
    out["b_minus_a_ms"] = mb["median"] - ma["median"]
    out["b_not_above_a_by_more_than_its_spread"] = bool(out["b_minus_a_ms"] <= out["a_spread_ms"])
    print(f"B - A = {out['b_minus_a_ms']:+.2f} ms (A's spread: {out['a_spread_ms']:.2f} ms)", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ext.free()
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
