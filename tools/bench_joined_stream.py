"""Streamed joined synthesis (generate.cpp generate_joined, JoinStream; include/ptts.h ptts_generate_joined_streamed): the
time to first audio and the total time of one text of three full groups (3 x max_batch chunks), full-size synthetic checkpoint, bf16, graph
step, one device voice, the header's telephony chain -- compressor, DC block, a 300-3400 Hz equaliser, fades, 8 kHz mu-law.  Per call: the wall
time from the call's start until the first pcm_callback returns, and until the call returns, for first_group 0 (max_batch), 4 and 1; and the
total time of ptts_generate_joined on the same text, which hands nothing over until the end.  The calls alternate after --warmup rounds, --runs
rounds are timed; the streamed bytes are compared with the joined call's once.  Writes profiles/joined_stream_bench.json (PTTS_OUT_DIR:
elsewhere)."""
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

RATE = 8000
FIRST_GROUPS = (0, 4, 1)


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "joined_stream_bench.json"))
    a = ap.parse_args()
    pkg = ptts_amd.load()
    rt = pkg.runtime
    wl = bench.WORKLOADS["b64_10s_bf16"]
    path = bench.checkpoint_path(pkg, wl["file"], 0, lambda: None)
    model, _ = bench.open_model(pkg, path, wl, 0, 1, 0)
    voice = model.upload_voice(pkg.VoiceModelState(bench.voice_modules(pkg, pkg.synth.SynthConfig.full())))
    chunks = a.groups * wl["batch"]
    toks = [np.ascontiguousarray(p, np.int64) for p in pkg.synth.make_prompts(chunks, 25, 4000, seed=42)]
    cfgs = bench.gen_cfgs(pkg, wl, chunks, voice)
    eq = rt.Eq([(rt.EQ_HIGHPASS, 300.0, 0.0, 0.707), (rt.EQ_LOWPASS, 3400.0, 0.0, 0.707)])
    dsp = rt._dsp_opts(pkg.RuntimeGenerateConfig(compressor=rt.CompressorOpts(), dc_block=True, eq=eq, fade_in_ms=20.0, fade_out_ms=80.0))
    join = rt.JoinOpts(gap_ms=100.0, dsp=dsp, sample_rate=RATE, pcm_format=pkg.PCM_ULAW)

    def joined():
        t0 = time.perf_counter()
        y = model.generate_joined(toks, cfgs, join).pcm
        return y, None, 1e3 * (time.perf_counter() - t0)

    def streamed(first_group):
        first, n = [], [0]

        def cb(off, x):
            n[0] += 1
            if not first:
                first.append(time.perf_counter())

        t0 = time.perf_counter()
        y = model.generate_joined(toks, cfgs, join, pcm_callback=cb, first_group=first_group).pcm
        t1 = time.perf_counter()
        return y, 1e3 * (first[0] - t0), 1e3 * (t1 - t0), n[0]

    ref = joined()[0]
    same = {}
    for fg in FIRST_GROUPS:
        y = streamed(fg)[0]
        # (another first group is another grouping of the batches: the bytes are those of the joined call only for first_group 0)
        same[str(fg)] = bool(y.dtype == ref.dtype and y.size == ref.size and np.array_equal(y, ref))
    print(f"text: {chunks} chunks x {wl['frames']} frames = {ref.size / RATE:.1f} s as {ref.size} mu-law bytes; same bytes as the joined call: {same}", flush=True)
    total = {"joined": []}
    first = {}
    hand_overs = {}
    for fg in FIRST_GROUPS:
        total[f"streamed_first_group_{fg}"] = []
        first[f"streamed_first_group_{fg}"] = []
    for it in range(a.warmup + a.runs):
        _, _, dt = joined()
        if it >= a.warmup:
            total["joined"].append(dt)
        for fg in FIRST_GROUPS:
            _, t_first, dt, n = streamed(fg)
            hand_overs[f"streamed_first_group_{fg}"] = n
            if it >= a.warmup:
                total[f"streamed_first_group_{fg}"].append(dt)
                first[f"streamed_first_group_{fg}"].append(t_first)
    out = {"workload": f"{chunks} chunks x 10 s in groups of {wl['batch']}, bf16, graph step, compressor + DC block + 300-3400 Hz equaliser + fades, gap 100 ms, "
                       f"{RATE} Hz mu-law", "runs": a.runs, "warmup": a.warmup, "same_bytes_as_joined": same, "hand_overs": hand_overs,
           "total_ms": {k: _stats(v) for k, v in total.items()}, "first_audio_ms": {k: _stats(v) for k, v in first.items()}}
    for k, v in out["total_ms"].items():
        f = out["first_audio_ms"].get(k)
        print(f"{k:28s} total median {v['median']:9.2f} ms (spread {v['spread']:7.2f})" +
              (f"   first audio median {f['median']:9.2f} ms (spread {f['spread']:7.2f})" if f else ""), flush=True)
    j = out["total_ms"]["joined"]
    out["streamed_0_minus_joined_ms"] = out["total_ms"]["streamed_first_group_0"]["median"] - j["median"]
    out["joined_spread_ms"] = j["spread"]
    print(f"streamed (first_group 0) - joined = {out['streamed_0_minus_joined_ms']:+.2f} ms (the joined call's own spread: {j['spread']:.2f} ms)", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    eq.free()
    voice.close()
    model.close()


if __name__ == "__main__":
    main()
