"""The deviations of the host statements of "keep the formants" (ptts_formant_analyse, ptts_formant_whiten, ptts_formant_shape) from the float64 numpy
restatement of tests/_formant_ref.py, case by case, on the rows of tests/test_formant_cpu.py: one JSON line per (stage, row kind, n[, pitch]) with the
worst deviation (coefficients absolute; samples relative to the row's peak), and a last line with the worst per stage -- the figures the bounds of
that test are 8 x of.  No GPU.  Writes profiles/formant_parity_observed.jsonl (PTTS_OUT_DIR: elsewhere)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _formant_ref as F   # noqa: E402

PITCHES = (800, 1250, 1500)


def _peak(x):
    fin = np.isfinite(x)
    return max(float(np.abs(x[fin]).max(initial=0.0)), 1e-30)


def _deviation(got, want, scale):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float(np.abs(got.astype(np.float64)[fin] - want[fin]).max(initial=0.0)) / scale


def main():
    import ptts_amd
    rt = ptts_amd.load().runtime
    lines, worst = [], {"coeffs": 0.0, "whiten": 0.0, "shape": 0.0}

    def note(stage, d, **case):
        lines.append(dict(stage=stage, deviation=d, **case))
        worst[stage] = max(worst[stage], d)

    for n in F.LENGTHS:
        for name, x in F.parity_rows(n).items():
            c = rt.formant_analyse(x)
            note("coeffs", _deviation(c, F.analyse(x), 1.0), row=name, n=n)
            e = rt.formant_whiten(c, x)
            note("whiten", _deviation(e, F.whiten(c, x), _peak(x)), row=name, n=n)
            for p in PITCHES:
                er = rt.pitch_resample(rt.PitchOpts(p), e)
                want = F.shape(c, n, p, er)
                note("shape", _deviation(rt.formant_shape(c, n, p, er), want, _peak(want)), row=name, n=n, pitch_permille=p)
    lines.append({"worst": worst, "unit": "coeffs: absolute; whiten, shape: of the row's peak"})
    out = os.path.join(os.environ.get("PTTS_OUT_DIR", os.path.join(ROOT, "profiles")), "formant_parity_observed.jsonl")
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    print(json.dumps(lines[-1]))


if __name__ == "__main__":
    main()
