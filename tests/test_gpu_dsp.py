"""Post-processing on the GPU (go-pocket-tts_amd/csrc/dsp.hip): ptts_dsp_rows and a request's `dsp` are ptts_dsp_apply's chain
-- normalise and fades bit for bit, the DC block to one f32 step at the row's peak -- on the request's own 24 kHz audio, in front of its egress; batching
changes no bit; requests without it are what they are without a DSP request beside them."""
import ctypes as C
import dataclasses
import json
import os
import threading

import numpy as np
import pytest

import _dsp_ref as D
import _resample_ref as R

pytestmark = pytest.mark.gpu

FORMATS = ["f32", "s16", "ulaw", "alaw"]
RATES = [0, 8000, 16000, 44100]
ALL4 = dict(normalize=True, dc_block=True, fade_in_ms=50.0, fade_out_ms=80.0)
EXACT = [dict(normalize=True), dict(fade_in_ms=50.0), dict(fade_out_ms=80.0), dict(fade_in_ms=1e5, fade_out_ms=1e5), dict(normalize=True, fade_in_ms=12.5, fade_out_ms=33.0)]
# dc_block with a rate change: the largest |gpu - host chain| / peak observed on MI355X per case is in profiles/dsp_parity_observed.jsonl; the bound is
# 4 x the largest of them (margin for other lengths and seeds), and never above 1e-5 of the peak (a lost state or a wrong coefficient shows at 1e-3)
RATE_DC_OBSERVED = 4.61e-8   # generate f32 44100 Hz, 7 frames
RATE_DC_BOUND = min(4 * RATE_DC_OBSERVED, 1e-5)


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    synth = pkg.synth
    cfg = synth.SynthConfig.tiny()
    path = str(tmp_path_factory.mktemp("dsp") / "tiny.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234))
    gm = pkg.Model.open(path, device=0, max_batch=4)
    yield cfg, gm
    gm.close()


def _cfg(pkg, steps, fmt="f32", rate=0, **kw):
    kw.setdefault("temperature", 0.0)
    return pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=steps, pcm16=fmt == "s16", g711=fmt if fmt in ("ulaw", "alaw") else "",
                                     sample_rate=rate, **kw)


def _convert(pkg, gm, pcm24, fmt, rate):   # the specification of egress (tests/test_gpu_resample.py): ptts_resample, then the device format conversion
    y = gm.resample(pcm24, 24000, rate) if rate not in (0, 24000) else pcm24
    return y if fmt == "f32" else gm.pcm_encode(y, {"s16": pkg.PCM_S16, "ulaw": pkg.PCM_ULAW, "alaw": pkg.PCM_ALAW}[fmt])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _host(pkg, x, sw):
    return pkg.runtime.dsp_apply(x, **sw)


def _record(case, value):
    out = os.environ.get("PTTS_DSP_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": case, "max_abs_diff_over_peak": value}) + "\n")


def _check_dc(pkg, gm, got, host24, fmt, rate, tag):
    """`got`: the device result in (fmt, rate); host24: ptts_dsp_apply of the same 24 kHz audio.  The bounds of DESIGN.md section 8 (N3)."""
    peak = float(np.abs(host24).max())
    assert peak > 0
    if rate in (0, 24000):
        if fmt == "f32":
            err = float(np.abs(got.astype(np.float64) - host24.astype(np.float64)).max())
            print(f"{tag}: max |gpu - host| {err:.3e}, bound {D.dc_bound(host24):.3e}")
            assert err <= D.dc_bound(host24), (tag, err)
            return
        s16 = R.pcm16(host24).astype(np.int64)
    else:
        y = gm.resample(host24, 24000, rate)
        if fmt == "f32":
            err = float(np.abs(got.astype(np.float64) - y.astype(np.float64)).max()) / peak
            print(f"{tag}: max |gpu - host chain| / peak {err:.3e}, bound {RATE_DC_BOUND:.3e}")
            _record(tag, err)
            assert err <= RATE_DC_BOUND, (tag, err)
            return
        s16 = R.pcm16(y).astype(np.int64)
    if fmt == "s16":
        d = int(np.abs(got.astype(np.int64) - s16).max())
        print(f"{tag}: max PCM16 difference {d}")
        assert d <= 1, (tag, d)
        return
    enc = R.ulaw_encode if fmt == "ulaw" else R.alaw_encode
    ok = np.zeros(got.size, bool)
    for dlt in (-1, 0, 1):
        ok |= got == enc(np.clip(s16 + dlt, -32768, 32767))
    print(f"{tag}: G.711 bytes outside the byte of the host sample +- 1: {int((~ok).sum())}")
    assert ok.all(), (tag, int((~ok).sum()))


def test_rows_are_the_host_chain_at_ragged_lengths(pkg, tiny):
    _, gm = tiny
    rows = [D.signal(n, seed=1) for n in D.LENGTHS] + [np.zeros(5000, np.float32), np.zeros(0, np.float32)]
    for sw in EXACT:
        got = gm.dsp_rows(rows, **sw)
        for x, y in zip(rows, got):
            want = _host(pkg, x, sw)
            assert y.size == x.size and np.array_equal(y.view(np.uint32), want.view(np.uint32)), (x.size, sw)
            ref = D.apply(x, normalize=sw.get("normalize", False), fade_in_ms=sw.get("fade_in_ms", 0.0), fade_out_ms=sw.get("fade_out_ms", 0.0))
            assert np.array_equal(y.view(np.uint32), ref.view(np.uint32)), (x.size, sw)
    for sw in (dict(dc_block=True), dict(normalize=True, dc_block=True), ALL4):
        got = gm.dsp_rows(rows, **sw)
        for x, y in zip(rows, got):
            want = _host(pkg, x, sw)
            if x.size == 0 or not x.any():
                assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
                continue
            err = float(np.abs(y.astype(np.float64) - want.astype(np.float64)).max())
            print(f"rows n={x.size} {sw}: max |gpu - host| {err:.3e}, bound {D.dc_bound(want):.3e}")
            assert err <= D.dc_bound(want), (x.size, sw, err)
            if x.size >= 48000 and not sw.get("normalize"):
                assert abs(float(y[x.size // 2: x.size - 4000].mean())) < 0.02     # the offset (0.3) is gone: the filter ran
            # the device computes the blocked form: its bits are the host instantiation's
            if sw == dict(dc_block=True):
                assert np.array_equal(y.view(np.uint32), pkg.runtime.dsp_blocked_host(x).view(np.uint32)), x.size
    same = gm.dsp_rows(rows)                                # nothing switched on: a copy
    for x, y in zip(rows, same):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    same = gm.dsp_rows(rows, opts=pkg.runtime.DspOpts())
    for x, y in zip(rows, same):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_batching_changes_no_bit(pkg, tiny):
    cfg, gm = tiny
    rows = [D.signal(n, seed=2) for n in (240000, 1921, 48000, 29, 1920 * 7)]
    for sw in (ALL4, dict(dc_block=True), dict(normalize=True)):
        batched = gm.dsp_rows(rows, **sw)
        for x, y in zip(rows, batched):
            assert np.array_equal(gm.dsp_rows(x, **sw).view(np.uint32), y.view(np.uint32)), (x.size, sw)
        rev = gm.dsp_rows(rows[::-1], **sw)[::-1]
        for a, b in zip(rev, batched):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and a generated request's row in its group is the row alone
    steps = [7, 3, 9, 5]
    toks = [[3 + i, 7, 11 + i] for i in range(4)]
    base = gm.generate_batch(toks, [_cfg(pkg, s) for s in steps])
    got = gm.generate_batch(toks, [_cfg(pkg, s, **ALL4) for s in steps])
    for b, g, s in zip(base, got, steps):
        assert g.n_frames == b.n_frames == s and g.pcm.size == s * 1920
        assert np.array_equal(g.pcm.view(np.uint32), gm.dsp_rows(b.pcm, **ALL4).view(np.uint32)), s


@pytest.mark.parametrize("rate", RATES)
def test_generated_requests_are_the_egress_of_the_host_chain(pkg, tiny, rate):
    """One-shot ptts_generate, ragged lengths, more requests than max_batch (4): the result with `dsp` is the egress of ptts_dsp_apply of the same
    request's plain 24 kHz f32 audio."""
    cfg, gm = tiny
    steps = [7, 3, 9, 5, 12, 4]
    toks = [[3 + i, 7, 11 + i] for i in range(len(steps))]
    base = gm.generate_batch(toks, [_cfg(pkg, s) for s in steps])
    # the yardstick bites: the decoded audio has low-frequency content the filter removes, far above every bound below
    moved = max(float(np.abs(_host(pkg, b.pcm, dict(dc_block=True)) - b.pcm).max() / np.abs(b.pcm).max()) for b in base)
    print(f"dc_block moves the tiny model's audio by {moved:.3e} of its peak")
    assert moved > 1e-3
    for fmt in FORMATS:
        for sw in EXACT:
            got = gm.generate_batch(toks, [_cfg(pkg, s, fmt, rate, **sw) for s in steps])
            for b, g in zip(base, got):
                want = _convert(pkg, gm, _host(pkg, b.pcm, sw), fmt, rate)
                assert g.n_frames == b.n_frames and g.pcm.dtype == want.dtype and np.array_equal(_bits(g.pcm), _bits(want)), (fmt, rate, sw, b.n_frames)
        for sw in (dict(dc_block=True), ALL4):
            got = gm.generate_batch(toks, [_cfg(pkg, s, fmt, rate, **sw) for s in steps])
            for b, g in zip(base, got):
                assert g.pcm.size == b.n_frames * 8 * (rate or 24000) // 100
                _check_dc(pkg, gm, g.pcm, _host(pkg, b.pcm, sw), fmt, rate, f"generate {fmt} {rate or 24000} Hz frames={b.n_frames} {'all4' if sw is ALL4 else 'dc'}")


def _run_dispatcher(pkg, gm, toks, cfgs, continuous):
    d = pkg.Dispatcher([gm], max_batch=4, window_us=50000, continuous=continuous, cont_kv_capacity=64, cont_max_steps=32, cont_steps_per_group=3)
    n = len(toks)
    got, errs = [None] * n, [None] * n

    def client(i):
        try:
            got[i] = d.generate(toks[i], cfgs[i])
        except Exception as e:  # noqa: BLE001
            errs[i] = e
    try:
        ts = [threading.Thread(target=client, args=(i,)) for i in range(n)]
        [t.start() for t in ts]
        [t.join(300) for t in ts]
        assert not any(errs), errs
        st = d.stats()
        assert (st["cont_steps"] > 0) == bool(continuous) and st["flow_cluster_fallbacks"] == 0, st
    finally:
        d.close()
    return got


SETS = [[(7, "f32", 0, ALL4), (3, "ulaw", 8000, ALL4), (9, "f32", 0, None), (5, "s16", 16000, None)],
        [(4, "alaw", 0, dict(dc_block=True)), (8, "f32", 44100, dict(fade_in_ms=50.0)), (5, "s16", 0, dict(normalize=True, fade_out_ms=80.0)), (6, "f32", 0, None)]]


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_dispatcher_serves_dsp_and_plain_requests_mixed(pkg, tiny, continuous, which):
    """Four callers at once (one batch / one admission of the engine): DSP and plain requests mixed.  The yardstick of each request is the same four
    requests served the same way with every DSP switch off; the plain ones keep their bits."""
    cfg, gm = tiny
    specs = SETS[which]
    toks = [[3 + i, 7, 11 + i] for i in range(len(specs))]
    cfgs = [_cfg(pkg, s, f, r, **(sw or {})) for s, f, r, sw in specs]
    got = _run_dispatcher(pkg, gm, toks, cfgs, continuous)
    off = _run_dispatcher(pkg, gm, toks, [_cfg(pkg, s, f, r) for s, f, r, _ in specs], continuous)       # no DSP request among them
    own = _run_dispatcher(pkg, gm, toks, [_cfg(pkg, s) for s, _, _, _ in specs], continuous)             # ... and their 24 kHz f32 audio
    for i, (s, f, r, sw) in enumerate(specs):
        assert got[i].n_frames == s
        if sw is None:
            assert np.array_equal(_bits(got[i].pcm), _bits(off[i].pcm)), i
            continue
        host = _host(pkg, own[i].pcm, sw)
        if sw.get("dc_block"):
            _check_dc(pkg, gm, got[i].pcm, host, f, r, f"dispatcher continuous={continuous} [{which}.{i}] {f} {r or 24000} Hz")
        else:
            assert np.array_equal(_bits(got[i].pcm), _bits(_convert(pkg, gm, host, f, r))), (i, f, r, sw)


def _raw_generate(pkg, gm, toks, cfgs):
    rt = pkg.runtime
    n = len(toks)
    reqs, ress, keep = (rt._Request * n)(), (rt._Result * n)(), []
    for i in range(n):
        gm._fill_request(reqs[i], toks[i], cfgs[i], keep)
    rc = rt.lib().ptts_generate(gm.h, reqs, n, ress)
    msg = rt.lib().ptts_last_error().decode(errors="replace")
    out = []
    for i in range(n):
        pcm = np.ctypeslib.as_array(ress[i].pcm, (int(ress[i].n_samples),)).copy() if ress[i].pcm and ress[i].n_samples else None
        out.append((int(ress[i].status), pcm))
        rt.lib().ptts_free_result(C.byref(ress[i]))
    return rc, msg, out


def test_refusals_name_the_field_and_the_others_run(pkg, tiny):
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [6, 9, 14]]
    good = gm.generate_batch([toks[1]], [_cfg(pkg, 4)])[0].pcm
    res4 = rt.DspOpts(1, 0, 0.0, 0.0)
    res4.reserved[2] = 7
    cb = lambda off, x: None  # noqa: E731
    bad = [(dict(fade_in_ms=-1.0), "fade_in_ms"), (dict(fade_out_ms=float("nan")), "fade_out_ms"), (dict(fade_in_ms=float("nan")), "fade_in_ms"),
           (dict(fade_out_ms=-0.5), "fade_out_ms"), (dict(dsp_opts=res4), "reserved"),
           (dict(normalize=True, pcm_callback=cb), "normalize"), (dict(fade_out_ms=10.0, pcm_callback=cb), "fade_out_ms"),
           (dict(dc_block=True, pcm_callback=cb), "dc_block"), (dict(fade_in_ms=10.0, pcm_callback=cb), "fade_in_ms")]
    for kw, field in bad:
        rc, msg, out = _raw_generate(pkg, gm, toks, [_cfg(pkg, 4, **kw), _cfg(pkg, 4)])
        assert rc == rt.PTTS_EINVAL and out[0][0] == rt.PTTS_EINVAL and field in msg and "dsp" in msg, (kw, rc, msg)
        assert out[1][0] == rt.PTTS_OK and np.array_equal(out[1][1].view(np.uint32), good.view(np.uint32)), kw
        with pytest.raises(pkg.PttsError) as ei:
            gm.dsp_rows(np.ones(10, np.float32), opts=rt.DspOpts(0, 0, -1.0, 0.0))
        assert ei.value.code == rt.PTTS_EINVAL and "fade_in_ms" in str(ei.value)
    d = pkg.Dispatcher([gm], max_batch=4, window_us=500, continuous=True, cont_kv_capacity=64, cont_max_steps=32)
    try:
        with pytest.raises(pkg.PttsError) as ei:
            d.generate(toks[0], _cfg(pkg, 4, fade_out_ms=-3.0))
        assert ei.value.code == rt.PTTS_EINVAL and "fade_out_ms" in str(ei.value)
    finally:
        d.close()


def test_null_and_all_off_opts_take_the_plain_path(pkg, tiny):
    """dsp = NULL and a struct with nothing switched on: the bits and the launches of a plain request (no DSP kernel, no k_resample, the decoder's
    direct store), also beside each other in one call."""
    cfg, gm = tiny
    rt = pkg.runtime
    toks = [[5, 9, 13], [5, 9, 13], [5, 9, 13]]
    for fmt in ("f32", "s16"):
        plain = gm.generate_batch(toks[:1], [_cfg(pkg, 6, fmt)])[0].pcm
        rt.launch_counts(True)
        got = gm.generate_batch(toks, [_cfg(pkg, 6, fmt), _cfg(pkg, 6, fmt, dsp_opts=rt.DspOpts()), _cfg(pkg, 6, fmt, dsp_opts=rt.DspOpts(0, 0, 0.0, 0.0))])
        counts = rt.launch_counts(False)
        assert not [k for k in counts if k.startswith("k_dsp") or k == "k_resample"], counts
        for g in got:
            assert np.array_equal(_bits(g.pcm), _bits(plain))
    rt.launch_counts(True)
    gm.generate_batch(toks[:2], [_cfg(pkg, 6, **ALL4), _cfg(pkg, 6, fade_in_ms=5.0)])
    counts = rt.launch_counts(False)
    assert counts.get("k_dsp_peak") == 1 and counts.get("k_dsp_summary") == 1 and counts.get("k_dsp_carry") == 1 and counts.get("k_dsp_apply") == 1, counts
    assert counts.get("k_resample") == 1, counts
