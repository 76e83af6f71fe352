"""Cloned voices as model states on the GPU (ptts_voice_from_embeddings / ptts_voice_from_audio, include/ptts.h): a voice embedding
prefilled once, alone from position 0, and kept as a device voice (what runtime_native_safetensors.go:104-119 prepends to every prompt,
and what the reference's `export-voice --format model-state` stores).  Its KV is pinned against the oracle's prefill of the same
embedding; generation with it against generation with the prepended embedding; its voice file round trip is exact."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import oracle as O
from _parity import parity

pytestmark = pytest.mark.gpu

FLOW_TOL = (2e-4, 5e-3)             # the per-layer K/V prefill test's (test_gpu_model.py)
BF16KV_TOL = (3e-2, None)           # bf16 cache: 8-bit mantissa keys/values, max-norm bound only (test_gpu_model.py)
MULTI_LAT_TOL = (2.5e-4, 5e-2)      # test_voice_embedding_is_prepended
MULTI_PCM_TOL = (3e-4, 1e-1)
CONT_LAT_TOL, CONT_PCM_TOL = (1e-4, 5e-3), (1e-4, 5e-2)   # test_gpu_continuous.py
SR = 24000


def _ckpt(pkg, tmp_path_factory, size, **kw):
    synth = pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny() if size == "tiny" else synth.SynthConfig.full(), **kw)
    path = str(tmp_path_factory.mktemp("vsb") / f"{size}.safetensors")
    synth.write_safetensors(path, synth.make_checkpoint(cfg, seed=1234))
    return cfg, path


@pytest.fixture(scope="module")
def tiny(pkg, tmp_path_factory):
    cfg, path = _ckpt(pkg, tmp_path_factory, "tiny")
    om = O.OracleModel.from_file(path)
    gm = pkg.Model.open(path, device=0, max_batch=8)
    yield cfg, path, om, gm
    gm.close()


@pytest.fixture(scope="module", params=[("tiny", "f32"), ("tiny", "bf16"), ("full", "f32"), ("full", "bf16")], ids=lambda p: f"{p[0]}-{p[1]}")
def model(request, pkg, tmp_path_factory):
    size, kv = request.param
    cfg, path = _ckpt(pkg, tmp_path_factory, size)
    om = O.OracleModel.from_file(path)
    gm = pkg.Model.open(path, device=0, kv=pkg.KV_F32 if kv == "f32" else pkg.KV_BF16)
    yield cfg, kv, om, gm
    gm.close()


def _emb(cfg, frames, seed=11):
    return np.random.default_rng(seed + frames).standard_normal((frames, cfg.d_model)).astype(np.float32)


def _kv(v, layer):   # [2,1,T,H,Dh] -> K, V as [H, T, Dh] (ptts_batch_read_kv / OracleState.kv)
    c = v.read_state(layer)
    return c[0, 0].transpose(1, 0, 2), c[1, 0].transpose(1, 0, 2)


@pytest.mark.parametrize("frames", [7, 125])
def test_kv_matches_the_oracle_prefill(pkg, model, frames):
    cfg, kv, om, gm = model
    e = _emb(cfg, frames)
    v = gm.voice_from_embedding(e)
    try:
        assert v.offset == frames
        st = om.new_state()
        om.prompt(st, e)
        tol = FLOW_TOL if kv == "f32" else BF16KV_TOL
        # full size: the relative error is taken on elements of at least 1 % of the scale (observed on MI355X: max rel 5.02e-3 on an
        # element at 1e-3 of the scale whose abs error, 2.6e-5, is 8x under the abs bar -- the prefill's own rounding, which this
        # path shares bit for bit: test_same_path_same_bits_and_batching)
        floor = 1e-3 if cfg.d_model < 1024 else 1e-2
        for layer in range(om.n_layers):
            ko, vo = st.kv(layer)
            kg, vg = _kv(v, layer)
            parity(f"voice build K {kv} T={frames} layer {layer}", kg, ko, tol, rel_floor=floor)
            parity(f"voice build V {kv} T={frames} layer {layer}", vg, vo, tol, rel_floor=floor)
    finally:
        v.close()


def test_same_path_same_bits_and_batching(pkg, model):
    cfg, kv, om, gm = model
    lens = [1, 7, 64, 125, 300]
    embs = [_emb(cfg, t) for t in lens]
    alone = []
    for e in embs:
        v = gm.voice_from_embedding(e)
        b = gm.new_batch(1, e.shape[0])
        b.prompt([e])
        for layer in range(gm.info.n_layers):
            kb, vb = b.read_kv(0, layer)
            kg, vg = _kv(v, layer)
            assert np.array_equal(kg, kb) and np.array_equal(vg, vb), (e.shape[0], layer)
        b.close()
        alone.append(v)
    many = gm.voice_from_embedding(embs)
    assert [v.offset for v in many] == lens
    tol = FLOW_TOL if kv == "f32" else BF16KV_TOL
    for t, a, m in zip(lens, alone, many):
        for layer in range(gm.info.n_layers):
            for x, y, w in zip(_kv(m, layer), _kv(a, layer), "KV"):
                parity(f"voice build batched {w} {kv} T={t} layer {layer}", x, y, tol)
    for v in alone + many:
        v.close()


def test_generation_matches_the_prepended_embedding(pkg, tiny):
    cfg, _, om, gm = tiny
    rt = pkg.Runtime(gm)
    ve = pkg.synth.make_voice_embedding(cfg, frames=7)["audio_prompt"]
    dv = gm.voice_from_embedding(pkg.VoiceEmbedding(ve, list(ve.shape)))
    for toks in ([7, 8, 9], [3, 14, 15, 9, 26]):
        ref = om.generate(toks, max_steps=6, eos_threshold=1e30, frames_after_eos=3, voice_emb=ve[0])
        got = rt.generate(toks, pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=6, want_latents=True, device_voice=dv))
        assert got.n_frames == ref["n_frames"] == 6 and got.eos_step == ref["eos_step"]
        parity("latents (cloned device voice)", got.latents, ref["latents"], MULTI_LAT_TOL)
        parity("pcm (cloned device voice)", got.pcm, ref["pcm"], MULTI_PCM_TOL)
        emb = rt.generate(toks, pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=6, want_latents=True,
                                                          voice_embedding=pkg.VoiceEmbedding(ve, list(ve.shape))))
        parity("latents (cloned device voice vs prepended)", got.latents, emb.latents, MULTI_LAT_TOL)
    dv.close()


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_voice_file_round_trip_is_exact(pkg, tiny, tmp_path, kv):
    cfg, path, om, _ = tiny
    gm = pkg.Model.open(path, device=0, kv=pkg.KV_F32 if kv == "f32" else pkg.KV_BF16)
    try:
        e = _emb(cfg, 23)
        dv = gm.voice_from_embedding(e)
        f = str(tmp_path / f"clone_{kv}.safetensors")
        dv.save(f)
        assert open(f, "rb").read() == dv.to_bytes()
        back = gm.open_voice(f)
        assert back.offset == 23
        for layer in range(gm.info.n_layers):
            assert np.array_equal(back.read_state(layer), dv.read_state(layer))
        st = dv.state()
        assert sorted(st.modules) == [f"transformer.layers.{i}.self_attn" for i in range(gm.info.n_layers)]
        rt = pkg.Runtime(gm)
        c = lambda **kw: pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=5, want_latents=True, **kw)
        a = rt.generate([5, 6, 7], c(device_voice=dv))
        b = rt.generate([5, 6, 7], c(device_voice=back))
        assert a.n_frames == b.n_frames == 5
        assert np.array_equal(a.latents, b.latents) and np.array_equal(a.pcm, b.pcm)
        # the saved file is an ordinary voice file: load_voice_conditioning -> host voice state, the oracle reads it too
        cond = pkg.load_voice_conditioning(f)
        h = rt.generate([5, 6, 7], c(**cond))
        parity(f"latents (saved voice as host state, {kv})", h.latents, a.latents, MULTI_LAT_TOL)
        if kv == "f32":
            ref = om.generate([5, 6, 7], max_steps=5, eos_threshold=1e30, frames_after_eos=3, voice_state=O.load_voice_model_state(O.Store.open(f)))
            parity("latents (saved voice, oracle)", a.latents, ref["latents"], MULTI_LAT_TOL)
        dv.close()
        back.close()
    finally:
        gm.close()


def _pcm(n, seed=0):
    rng = np.random.default_rng(seed + n)
    t = np.arange(n) / SR
    return (0.3 * np.sin(2 * np.pi * 180 * t) * np.sin(2 * np.pi * 3 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def test_state_from_audio(pkg, tmp_path_factory, tiny):
    cfg, path = _ckpt(pkg, tmp_path_factory, "tiny", speaker_proj=True, encoder=True)
    gm = pkg.Model.open(path, device=0)
    try:
        clips = [_pcm(SR // 2, 1), _pcm(3 * SR, 2)]
        vs = gm.voice_state_from_audio(clips)   # one build of both (the packed prefill's tiling follows the batch: not bit for bit)
        for clip, v in zip(clips, vs):
            emb = gm.voice_from_audio(clip)
            w = gm.voice_from_embedding(emb)
            one = gm.voice_state_from_audio(clip)
            assert v.offset == w.offset == one.offset == emb.shape[1]
            for layer in range(gm.info.n_layers):
                assert np.array_equal(one.read_state(layer), w.read_state(layer))
                parity(f"state from audio batched layer {layer}", v.read_state(layer), w.read_state(layer), FLOW_TOL)
            w.close()
            one.close()
        rt = pkg.Runtime(gm)
        emb = gm.voice_from_audio(clips[0])
        c = lambda **kw: pkg.RuntimeGenerateConfig(eos_threshold=float("inf"), max_steps=6, want_latents=True, **kw)
        a = rt.generate([4, 5, 6], c(device_voice=vs[0]))
        b = rt.generate([4, 5, 6], c(voice_embedding=emb))
        assert a.n_frames == b.n_frames == 6 and a.eos_step == b.eos_step
        parity("latents (state from audio vs prepended embedding)", a.latents, b.latents, MULTI_LAT_TOL)
        parity("pcm (state from audio vs prepended embedding)", a.pcm, b.pcm, MULTI_PCM_TOL)
        for v in vs:
            v.close()
    finally:
        gm.close()
    _, _, _, plain = tiny   # no encoder weights
    with pytest.raises(pkg.PttsError, match="mimi.encoder.model.0.conv.weight") as ei:
        plain.voice_state_from_audio(_pcm(SR, 3))
    assert ei.value.code == pkg.runtime.PTTS_EFORMAT


def test_serving_one_cloned_voice_to_32_requests(pkg, tiny):
    cfg, _, om, gm = tiny
    dv = gm.voice_from_embedding(_emb(cfg, 9))
    rng = np.random.default_rng(41)
    n = 32
    prompts = [rng.integers(1, cfg.n_bins, size=int(rng.integers(3, 9))).astype(np.int64) for _ in range(n)]
    steps = [int(rng.integers(2, 12)) for _ in range(n)]
    cfgs = [pkg.RuntimeGenerateConfig(max_steps=steps[i], eos_threshold=1e30, want_latents=True, device_voice=dv) for i in range(n)]
    rt = pkg.Runtime(gm)
    want = [rt.generate(prompts[i], cfgs[i]) for i in range(n)]
    import threading
    d = pkg.Dispatcher([gm], max_batch=4, window_us=2000, continuous=True, cont_kv_capacity=64, cont_max_steps=32, cont_steps_per_group=3)
    got, errs = [None] * n, [None] * n

    def client(i):
        try:
            got[i] = d.generate(prompts[i], cfgs[i])
        except Exception as e:  # noqa: BLE001
            errs[i] = e
    try:
        ts = [threading.Thread(target=client, args=(i,)) for i in range(n)]
        [t.start() for t in ts]
        [t.join(180) for t in ts]
        assert not any(errs), errs
        for i in range(n):
            assert got[i].n_frames == want[i].n_frames == steps[i]
            parity(f"cloned voice served latents[{i}]", got[i].latents, want[i].latents, CONT_LAT_TOL)
            parity(f"cloned voice served pcm[{i}]", got[i].pcm, want[i].pcm, CONT_PCM_TOL)
    finally:
        d.close()
    sh = gm.share()   # a voice built on one engine serves a ptts_model_share engine
    try:
        s = pkg.Runtime(sh).generate(prompts[0], cfgs[0])
        assert s.n_frames == steps[0]
        parity("cloned voice on a shared engine", s.latents, want[0].latents, CONT_LAT_TOL)
    finally:
        sh.close()
    dv.close()


def test_errors_and_no_leaks(pkg, tiny):
    cfg, _, _, gm = tiny
    L = pkg.runtime.lib()
    e = _emb(cfg, 5)
    hs = (C.c_void_p * 2)()
    pp = (pkg.runtime._FP * 1)(pkg.runtime._fp(e))
    fr = np.array([5], np.int64)

    def call(emb, frames, width, n, out):
        rc = L.ptts_voice_from_embeddings(gm.h, emb, frames, width, n, out)
        return rc, L.ptts_last_error().decode()
    rc, msg = call(pp, pkg.runtime._ip(fr), cfg.d_model + 1, 1, hs)
    assert rc == pkg.runtime.PTTS_EINVAL and str(cfg.d_model + 1) in msg and str(cfg.d_model) in msg
    z = np.array([0], np.int64)
    rc, msg = call(pp, pkg.runtime._ip(z), cfg.d_model, 1, hs)
    assert rc == pkg.runtime.PTTS_EINVAL and "frames" in msg
    for n in (0, -1):
        rc, msg = call(pp, pkg.runtime._ip(fr), cfg.d_model, n, hs)
        assert rc == pkg.runtime.PTTS_EINVAL and msg
    rc, msg = call(None, pkg.runtime._ip(fr), cfg.d_model, 1, hs)
    assert rc == pkg.runtime.PTTS_EINVAL and msg
    rc, msg = call(pp, None, cfg.d_model, 1, hs)
    assert rc == pkg.runtime.PTTS_EINVAL and msg
    rc, msg = call(pp, pkg.runtime._ip(fr), cfg.d_model, 1, None)
    assert rc == pkg.runtime.PTTS_EINVAL and msg
    nul = (pkg.runtime._FP * 2)(pkg.runtime._fp(e), None)
    fr2 = np.array([5, 5], np.int64)
    rc, msg = call(nul, pkg.runtime._ip(fr2), cfg.d_model, 2, hs)
    assert rc == pkg.runtime.PTTS_EINVAL and "null" in msg
    with pytest.raises(pkg.PttsError):
        gm.voice_from_embedding(np.zeros((3, cfg.d_model + 1), np.float32))
    # nothing leaks: device memory is the same after 100 build / free cycles (after one to size the workspaces)
    import torch
    embs = [_emb(cfg, 40), _emb(cfg, 3)]
    for v in gm.voice_from_embedding(embs):
        v.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(100):
        for v in gm.voice_from_embedding(embs):
            v.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    per_cycle = 2 * gm.info.n_layers * 2 * 43 * cfg.d_model * 4
    assert free0 - free1 < 8 * per_cycle, (free0, free1, per_cycle)   # a leak would hold 100 cycles' voices
