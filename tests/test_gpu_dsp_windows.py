"""The causal stages of the chain in windows with carried state (go-pocket-tts_amd/csrc/dsp.hip, compressor.hip, dsp_tile.h; dsp_device.cpp
dsp_launch's windowed jobs; include/ptts_debug.h ptts_debug_dsp_windows): wherever rows are cut on the grid of 1920
samples, the windows give the bits of the one-shot chain (ptts_dsp_rows on the same rows and options) -- for the compressor, the DC block, a 1-
and a 4-section equaliser, a fade in inside the first window and one across a window boundary, and all of them with a fade out.  The input
makes every stage move the samples and makes carried state matter: both are checked with the host statements before the device is trusted."""
import numpy as np
import pytest

import _chain_ref as R

pytestmark = pytest.mark.gpu

TILE = 1920
LENGTHS = [0, 1, 29, 30, 1919, 1920, 1921, 3840, 5 * 1920 + 77, 66 * 1920 + 31]   # the last one crosses the carry's 64-tile batch
EQ1 = [(5, 1000.0, 6.0, 0.9)]                                                       # (type, Hz, dB, Q): one peaking section
EQ4 = [(2, 300.0, 0.0, 0.707), (1, 3400.0, 0.0, 0.707), (5, 1000.0, 4.0, 1.0), (4, 6000.0, -3.0, 0.7)]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    path = str(tmp_path_factory.mktemp("windows") / "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(synth.SynthConfig.tiny(), seed=1234))
    gm = pkg.Model.open(path, device=0, max_batch=4)
    yield gm
    gm.close()


@pytest.fixture(scope="module")
def rows():
    """Seeded noise plus a 0.1 DC offset plus a 200 Hz tone at 0.5: computed once, never written to."""
    rng = np.random.default_rng(20)
    out = []
    for n in LENGTHS:
        t = np.arange(n, dtype=np.float64)
        x = (0.1 * rng.standard_normal(n) + 0.1 + 0.5 * np.sin(2.0 * np.pi * 200.0 * t / 24000.0)).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return out


def _patterns():
    every = [TILE * k for k in range(1, LENGTHS[-1] // TILE + 1)]
    rng = np.random.default_rng(7)
    some = sorted(int(c) for c in rng.choice(every, size=9, replace=False))
    return {"none": [], "every": every, "one": [TILE], "batch": [63 * TILE, 64 * TILE, 65 * TILE], "random": some}


PATTERNS = _patterns()


def _stages(pkg):
    cmp_ = pkg.runtime.CompressorOpts(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=120.0)
    return {
        "compressor": dict(compressor=cmp_),
        "dc": dict(dc_block=True),
        "eq1": dict(eq=EQ1),
        "eq4": dict(eq=EQ4),
        "fade_in_50": dict(fade_in_ms=50.0),
        "fade_in_100": dict(fade_in_ms=100.0),                                      # 2400 samples: across the boundary at 1920
        "all": dict(compressor=cmp_, dc_block=True, eq=EQ4, fade_in_ms=100.0, fade_out_ms=80.0),
    }


STAGE_NAMES = ["compressor", "dc", "eq1", "eq4", "fade_in_50", "fade_in_100", "all"]


@pytest.fixture(scope="module")
def one_shot(pkg, tiny, rows):
    """stage -> (the chain, ptts_dsp_rows over the rows): the reference, computed once."""
    out = {}
    for name, kw in _stages(pkg).items():
        chain = R.Chain(pkg, **kw)
        ref = tiny.dsp_rows(rows, opts=chain.opts)
        for r in ref:
            r.setflags(write=False)
        out[name] = (chain, ref)
    return out


@pytest.mark.parametrize("stage", STAGE_NAMES)
def test_the_input_makes_the_comparison_bite(pkg, rows, one_shot, stage):
    """On the host: the stage moves the samples, and windows without carried state would give other samples.  Also: the device's one-shot chain is
    the host statement, so what the windows are compared with is the documented result."""
    chain, ref = one_shot[stage]
    x = rows[8]                                                                     # 5 * 1920 + 77
    cuts = R.legal_cuts([TILE * k for k in range(1, 6)], [x.size], chain.fade_out_ms)
    assert len(cuts) >= 4
    whole = chain.host(x)
    assert not np.array_equal(_u32(whole), _u32(x)), stage
    assert not np.array_equal(_u32(whole), _u32(chain.stateless(x, cuts))), stage
    for i in (1, 4, 6, 8):
        assert np.array_equal(_u32(ref[i]), _u32(chain.host(rows[i]))), (stage, LENGTHS[i])


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("stage", STAGE_NAMES)
def test_windows_give_the_one_shot_bits(pkg, tiny, rows, one_shot, stage, pattern):
    chain, ref = one_shot[stage]
    cuts = R.legal_cuts(PATTERNS[pattern], LENGTHS, chain.fade_out_ms)
    if stage == "all" and pattern == "one":
        cuts = [2 * TILE]                                                           # (1920 lies in the fade out of the row of 1921 samples)
    assert bool(cuts) == (pattern != "none") and (chain.fade_out_ms > 0 or cuts == PATTERNS[pattern])
    got = tiny.dsp_windows(rows, cuts, chain.opts)
    for i, (g, w) in enumerate(zip(got, ref)):
        assert g.size == w.size == LENGTHS[i]
        bad = np.flatnonzero(_u32(g) != _u32(w))
        assert bad.size == 0, (stage, pattern, LENGTHS[i], int(bad.size), int(bad[0]))


def test_the_launches_of_a_window(pkg, tiny, rows):
    """Without a cut the hook launches what ptts_dsp_rows launches; an open window's summaries cover its last tile, also when it is its only one."""
    rt = pkg.runtime
    chain = R.Chain(pkg, **_stages(pkg)["all"])
    rt.launch_counts(True)
    tiny.dsp_rows(rows, opts=chain.opts)
    want = rt.launch_counts(False)
    rt.launch_counts(True)
    tiny.dsp_windows(rows, [], chain.opts)
    assert rt.launch_counts(False) == want and want.get("k_cmp_apply") == 1 and want.get("k_eq_apply") == 1, want
    one = [rows[7]]                                                                 # 3840 samples: windows of one tile each, the first open
    rt.launch_counts(True)
    got = tiny.dsp_windows(one, [TILE], chain.opts)
    counts = rt.launch_counts(False)
    assert np.array_equal(_u32(got[0]), _u32(tiny.dsp_rows(one, opts=chain.opts)[0]))
    assert counts.get("k_dsp_summary") == 1 and counts.get("k_eq_summary") == 1 and counts.get("k_cmp_summary_p") == 1 and counts.get("k_cmp_apply") == 2, counts


def test_refusals_name_what_is_wrong_and_launch_nothing(pkg, tiny, rows):
    rt = pkg.runtime

    def refused(cuts, opts, xs=rows):
        rt.launch_counts(True)
        with pytest.raises(pkg.PttsError) as ei:
            tiny.dsp_windows(xs, cuts, opts)
        counts = rt.launch_counts(False)
        assert ei.value.code == rt.PTTS_EINVAL and not counts, (str(ei.value), counts)
        return str(ei.value)

    # a cut inside a row's fade out: row 6 has 1921 samples, the last 1920 of them fade
    msg = refused([TILE], rt.DspOpts(0, 0, 0.0, 80.0))
    assert "cut 0" in msg and "row 6" in msg and "fade out" in msg, msg
    # cuts off the grid, not ascending, at 0
    for cuts in ([1000], [TILE, TILE], [2 * TILE, TILE], [0]):
        assert "cut" in refused(cuts, rt.DspOpts(0, 1, 0.0, 0.0)), cuts
    # the stages that are not causal, as the streamed joined call words them
    lim = rt.LimiterOpts(ceiling_db=-12.0, lookahead_ms=1.5, release_ms=80.0, drive_db=12.0)
    for cfg, word in ((dict(normalize=True), "normalize"), (dict(true_peak_dbtp=-1.0), "true_peak"), (dict(limiter=lim), "limiter")):
        msg = refused([TILE], rt._dsp_opts(pkg.RuntimeGenerateConfig(**cfg)))
        assert word in msg and "pcm_callback" in msg, (word, msg)
    # the model serves on
    assert np.array_equal(_u32(tiny.dsp_windows([rows[7]], [TILE], rt.DspOpts(0, 1, 0.0, 0.0))[0]), _u32(tiny.dsp_rows([rows[7]], dc_block=True)[0]))
