"""Voice-file writer and the cloned-voice ABI, host side: what ptts_voice_embedding_write / ptts_voice_state_write_bytes write reads back
through the library's reader (ptts_voice_file_*) and through the oracle's independent restatement of the reference reader
(internal/safetensors/reader.go:69-155,219-308), with the safetensors layout every reader accepts."""
import ctypes as C
import json
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

NEW_SYMBOLS = {"ptts_voice_from_embeddings", "ptts_voice_from_audio", "ptts_voice_offset", "ptts_voice_read_state", "ptts_voice_write",
               "ptts_voice_write_bytes", "ptts_voice_state_write_bytes", "ptts_voice_embedding_write", "ptts_free_bytes"}


@pytest.fixture(scope="module")
def rt(pkg):
    return pkg.runtime


def _header(data: bytes):
    (hl,) = struct.unpack("<Q", data[:8])
    raw = data[8:8 + hl]
    return hl, raw, json.loads(raw)


def _check_layout(data: bytes):
    hl, raw, hdr = _header(data)
    assert (8 + hl) % 8 == 0, "data section must start 8-byte aligned"
    assert raw == raw.rstrip(b" ") + b" " * (len(raw) - len(raw.rstrip(b" "))), "header padding must be spaces"
    assert raw.rstrip(b" ").endswith(b"}")
    names = [n for n in hdr if n != "__metadata__"]
    assert names == sorted(names), "tensor names in sorted order"
    end = 0
    for n in names:   # contiguous, in header order, covering the whole data section
        o0, o1 = hdr[n]["data_offsets"]
        assert o0 == end, (n, o0, end)
        end = o1
    assert 8 + hl + end == len(data)
    return hdr


def _caches(n_layers, offset, heads=16, hd=64, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((2, 1, offset, heads, hd)).astype(np.float32) for _ in range(n_layers)]


def test_embedding_file_round_trip(rt, tmp_path):
    emb = np.random.default_rng(1).standard_normal((13, 1024)).astype(np.float32)
    emb[0, 0] = -0.0
    path = str(tmp_path / "clone.safetensors")
    rt.VoiceEmbedding(emb[None], [1, 13, 1024]).save(path)
    data = open(path, "rb").read()
    hdr = _check_layout(data)
    assert list(hdr) == ["audio_prompt"] and hdr["audio_prompt"]["dtype"] == "F32" and hdr["audio_prompt"]["shape"] == [1, 13, 1024]
    vf = rt.VoiceFile(path)
    assert vf.kind == "embedding"
    got = vf.embedding()
    assert list(got.shape) == [1, 13, 1024]
    assert got.data.view(np.uint32).tobytes() == emb[None].view(np.uint32).tobytes()
    st = O.Store.open(path)
    ref = O.load_voice_embedding(st)
    assert ref.shape == (1, 13, 1024) and ref.view(np.uint32).tobytes() == emb[None].view(np.uint32).tobytes()
    assert rt.load_voice_conditioning(path)["voice_embedding"].data.tobytes() == emb[None].tobytes()


@pytest.mark.parametrize("n_layers,offset", [(1, 1), (2, 7), (12, 125)])
def test_model_state_file_round_trip(rt, n_layers, offset):
    caches = _caches(n_layers, offset)
    data = rt.voice_state_file_bytes(caches, offset)
    hdr = _check_layout(data)
    want = sorted([f"transformer.layers.{l}.self_attn/{k}" for l in range(n_layers) for k in ("cache", "offset")])
    assert list(hdr) == want
    for l in range(n_layers):
        c, o = hdr[f"transformer.layers.{l}.self_attn/cache"], hdr[f"transformer.layers.{l}.self_attn/offset"]
        assert c["dtype"] == "F32" and c["shape"] == [2, 1, offset, 16, 64]   # T = offset: no padding rows
        assert o["dtype"] == "I64" and o["shape"] == [1]
    vf = rt.VoiceFile(data)
    assert vf.kind == "model_state"
    ptrs, steps, offs = vf.state_arrays(n_layers, 16, 64)
    assert list(steps) == [offset] * n_layers and list(offs) == [offset] * n_layers
    for l in range(n_layers):
        got = np.ctypeslib.as_array(ptrs[l], shape=(caches[l].size,))
        assert got.view(np.uint32).tobytes() == caches[l].view(np.uint32).tobytes()
    # the oracle's own reader
    mods = O.load_voice_model_state(O.Store(data))
    oc, osteps, ooffs = O.voice_state_layers(mods, n_layers, 16, 64)
    assert list(osteps) == [offset] * n_layers and list(ooffs) == [offset] * n_layers
    for l in range(n_layers):
        assert np.asarray(oc[l], np.float32).tobytes() == caches[l].tobytes()
    st = rt.VoiceFile(data).model_state()
    assert rt.VoiceModelState(st.modules).modules.keys() == mods.keys()


def test_model_state_file_through_load_voice_conditioning(rt, tmp_path):
    caches = _caches(2, 9)
    path = tmp_path / "state.safetensors"
    path.write_bytes(rt.voice_state_file_bytes(caches, 9))
    got = rt.load_voice_conditioning(str(path))["voice_model_state"]
    ptrs, steps, offs, _ = rt._voice_arrays(got, 2)
    assert list(offs) == [9, 9] and list(steps) == [9, 9]
    assert got.modules["transformer.layers.1.self_attn"]["cache"].tobytes() == caches[1].tobytes()


def test_writers_reject_bad_arguments(rt, tmp_path):
    L = rt.lib()
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert L.ptts_voice_state_write_bytes(None, 3, 2, 16, 64, C.byref(p), C.byref(n)) == rt.PTTS_EINVAL
    assert L.ptts_voice_state_write_bytes(None, 3, 0, 16, 64, C.byref(p), C.byref(n)) == rt.PTTS_EINVAL
    assert L.ptts_voice_embedding_write(None, 3, 1024, str(tmp_path / "x").encode()) == rt.PTTS_EINVAL
    e = np.zeros((2, 4), np.float32)
    assert L.ptts_voice_embedding_write(rt._fp(e), 0, 4, str(tmp_path / "x").encode()) == rt.PTTS_EINVAL
    assert L.ptts_voice_embedding_write(rt._fp(e), 2, 4, str(tmp_path / "no" / "such" / "dir").encode()) == rt.PTTS_EIO
    assert "create" in L.ptts_last_error().decode()
    with pytest.raises(rt.PttsError):
        rt.voice_state_file_bytes([np.zeros((2, 1, 3, 16, 64), np.float32)], 4)


def test_device_entry_points_reject_null_without_a_gpu(rt):
    L = rt.lib()
    o = C.c_int64()
    assert L.ptts_voice_offset(None, C.byref(o)) == rt.PTTS_EINVAL
    assert L.ptts_voice_read_state(None, 0, None) == rt.PTTS_EINVAL
    assert L.ptts_voice_write(None, b"/dev/null") == rt.PTTS_EINVAL
    hs = (C.c_void_p * 1)()
    assert L.ptts_voice_from_embeddings(None, None, None, 1024, 1, hs) == rt.PTTS_EINVAL
    assert L.ptts_voice_from_audio(None, None, None, 1, hs) == rt.PTTS_EINVAL


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptts_")}


def test_symbols(rt):
    prod = _exports(rt.LIB_PATH)
    assert NEW_SYMBOLS <= prod
    assert prod == set(rt.ABI_SYMBOLS), (prod ^ set(rt.ABI_SYMBOLS))
    assert not (prod & set(rt.HOOK_SYMBOLS))
    hooks = _exports(rt.HOOKS_PATH)
    assert hooks == set(rt.HOOK_SYMBOLS) and not (hooks & NEW_SYMBOLS)
