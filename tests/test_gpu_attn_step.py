"""The AR step's attention (csrc/attn_step.hip: k_attn_step, and k_attention behind it for caches beyond one burst) stand-alone, value by value, against f64
numpy on the same operands -- every instantiation (KV format x load rounds NI = 1..16), every slot this step's own key can take, every prefix boundary.

What it replaces: StreamingMultiheadAttention's one-token step (attention.go:402-484): RoPE of q and k at the cache offset (rope.go:81-105), append of k and v,
softmax(q K^T / 8) V over the keys 0..offset.  The hook (ptts_debug_attn_step) fills AttnArgs as the step does (step.cpp step_core), calls launch_attention --
so the dispatch is under test too -- and returns the output (pre-filled with 0xff bytes) and both caches whole.  It refuses, before anything is uploaded, every
operand that could make the kernel leave the hook's buffers (test_refusals_before_any_launch).

Reference (reference() below): f64.  q and k are rotated with the table row at `pos` (pairs 2t, 2t + 1); keys j < pre are decoded from the prefix buffer of the
row's voice at `layer`, keys pre <= j < pos from the row's own cache, key `pos` is this step's own k and v in the cache format (bf16: round to nearest even).
For the own KEY the reference takes the row the kernel stored, after that row has passed its own check against the f64 rotation (below): the f32 rotation
and the f64 one may round to different bf16 neighbours (about 6e-5 of all elements do), one bf16 ulp in a key of weight 1/2 moves the output by 1e-3, and
which neighbour is stored is not an attention error -- every later step reads the stored one.  The no-GPU tests use the emulation's stored row the same way.

Cache rows the kernel must not use hold 0xff bytes (a NaN in either format) or canonical NaNs: own rows j < pre (the prefix is read from the voice, not from
the slot's copy), every row j >= pos.  A prefix buffer holds exactly `pre` rows per (layer, head), so an over-read lands in the next head's data.

Tolerance, per output element e, with u = 2^-24, A = max_j sum_e |q_e k_je| and V_e = max_j |v_je|:
  score: q's rotation, then 64 products summed 4 or 8 per lane and over 4 or 3 DPP steps: at most 13 roundings, |ds| <= 0.125 * 13 u A;
  weight: p_j = __expf(s_j - mx): the subtraction (u * 16), v_exp_f32 on x log2(e) (1 ulp = 2 u, and the rounded argument: 2 u |x|, |x| <= 16: the peaked family
  is held to that spread), and the two scores' errors: relative error eps <= 2 ds + 16 u + 34 u;
  out = sum p_j v_j / sum p_j is a convex combination: relative errors eps_j of the weights move it by at most 2 eps V_e;
  the f32 sums: at most 16 slots per lane, one DPP step, 16 LDS rows, for numerator and denominator, and the division: 67 u V_e.
  bound_e = V_e (4 ds + 167 u), never above the project's attention tolerance 2e-4 absolute (TOL["attention"], test_gpu_ops.py).
k_attention sums in another order (at most 33 + 5 and 9 + 6 terms deep) and uses expf: the same bound covers it.  On these inputs the bound reaches 1.6e-4 (5e-5 is typical);
test_emulation_stays_within_half_the_bound (no GPU) runs a numpy f32 emulation in the kernel's order of reduction over every case and holds it to HALF the
bound (it comes out at 0.01 of it).  OBSERVED on the MI355X (profiles/attn_step_parity.txt): k_attn_step errs by at most 3.6e-7, 0.009 of the bound,
k_attention by 1.7e-7, 0.007 -- the device's __expf is no coarser than numpy's exp on these arguments, no term was underestimated, and the observed
maximum is far inside a tenth of the bound, so the bound is used as derived.  It is a worst case (every rounding at its limit, all in one direction); what
makes a wrong key fail is not its tightness but the flat family below.

The flat family (q scaled by 0.25: scores spread by 1-2) is what makes a dropped, duplicated or mis-sourced key fail: test_flat_cases_feel_every_key (no GPU)
asserts for every flat case that removing any one key, or replacing any key's K and V rows by its neighbour's, moves the f64 reference by at least 10 x the
tolerance.  The peaked family (q at scale 1: spread about 6) is for errors in scores, max and exp."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round
from _parity import record

F32 = np.float32
U = 2.0 ** -24
CEIL = 2e-4                      # TOL["attention"] (test_gpu_ops.py): the reference's own attention tolerance, absolute
H, LAYERS, LAYER = 3, 2, 1       # layer 1 of 2: the prefix offset of the layer is not zero
D = H * 64
QLD, OLD = 3 * D + 2, D + 4
BURST = {"f32": 256, "bf16": 512}   # the longest cache k_attn_step takes (ATT_NI * keys per round)


# ------------------------------------------------------------------------------------------------ host arithmetic the launcher does (restated)
def keys_per_round(fmt):
    """attn_step_keys_per_round: 4 waves x keys per wave-instruction (1 KiB: 8 keys of 128 B in bf16, 4 of 256 B in f32)."""
    return 4 * kpi(fmt)


def kpi(fmt):
    return 8 if fmt == "bf16" else 4


def rounds(keys, fmt):
    """attn_step_rounds."""
    kpr = keys_per_round(fmt)
    return max(1, min(16, (keys + kpr - 1) // kpr))


def launch_rounds(keys_now, cap, fmt):
    """attn_step_launch_rounds: bounded by keys_now when the host knows it, by the cache capacity otherwise."""
    return rounds(min(keys_now, cap) if keys_now > 0 else cap, fmt)


# ------------------------------------------------------------------------------------------------ number formats
def to_fmt(a, fmt):
    """f32 values in the cache format's precision."""
    return bf16_round(a) if fmt == "bf16" else np.ascontiguousarray(a, F32)


def to_bits(a, fmt):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (u >> 16).astype(np.uint16) if fmt == "bf16" else u.copy()


def from_bits(b, fmt):
    return (b.astype(np.uint32) << 16).view(F32) if fmt == "bf16" else np.ascontiguousarray(b).view(F32)


def fill_bits(fmt, pad):
    """what unused cache rows hold: 0xff bytes, or the canonical NaN"""
    if pad == "ff":
        return np.uint16(0xFFFF) if fmt == "bf16" else np.uint32(0xFFFFFFFF)
    return np.uint16(0x7FC0) if fmt == "bf16" else np.uint32(0x7FC00000)


# ------------------------------------------------------------------------------------------------ cases
def case(fmt, rows, voices=(), cap=None, keys_now="exact", family="flat", pad="ff", own_copy=False, tag=""):
    """rows: (pos, voice, active) or (pos, voice) or pos; voice: index into `voices` (their lengths) or -1; the row's prefix length is its voice's length.
    keys_now: "exact" (longest live row + 1), 0 (unknown), or a number.  own_copy: own rows j < pre hold the prefix (k_attention reads them)."""
    rr = []
    for r in rows:
        r = (r,) if isinstance(r, int) else tuple(r)
        r = r + (-1, 1)[len(r) - 1:]
        rr.append(r)
    cap = BURST[fmt] if cap is None else cap
    live = [p for p, _, a in rr if a]
    kn = (max(live) + 1 if live else 1) if keys_now == "exact" else int(keys_now)
    c = dict(fmt=fmt, rows=tuple(rr), voices=tuple(voices), cap=cap, keys_now=kn, family=family, pad=pad, own_copy=own_copy, tag=tag)
    c["kernel"] = "k_attn_step" if cap <= BURST[fmt] else "k_attention"
    c["ni"] = launch_rounds(kn, cap, fmt) if c["kernel"] == "k_attn_step" else 0
    return c


def cid(c):
    pos = ",".join(("" if a else "off") + str(p) for p, _, a in c["rows"])
    pre = ",".join(str(c["voices"][v]) if v >= 0 else "0" for _, v, _ in c["rows"])
    s = f"{c['fmt']}-ni{c['ni']}-pos{pos}-pre{pre}-{c['family']}"
    if c["cap"] != BURST[c["fmt"]]:
        s += f"-cap{c['cap']}"
    if c["pad"] != "ff":
        s += "-nanpad"
    return s + (("-" + c["tag"]) if c["tag"] else "")


FMTS = ("f32", "bf16")
# every instantiation: keys_now = NI rounds; rows at the last slot of the last round, its first slot, and two smaller offsets (for a large NI most slots of
# those rows are clamp slots)
EVERY_NI = []
for _f in FMTS:
    for _ni in range(1, 17):
        _kpr = keys_per_round(_f)
        EVERY_NI.append(case(_f, [_ni * _kpr - 1, (_ni - 1) * _kpr, (_ni * _kpr) // 3 + 1, 2 + _ni % 5], keys_now=_ni * _kpr,
                             family="flat" if _ni % 4 else "peaked"))
# the own-key slot: every (w_p, kq_p) at i_p = 0 -- offsets 0..15 (f32), 0..31 (bf16) -- and one full round later (i_p = 1) and two (i_p = 2) for a few
OWN_SLOT = []
for _f in FMTS:
    _kpr = keys_per_round(_f)
    for _o in range(0, _kpr, 8):
        OWN_SLOT.append(case(_f, list(range(_o, _o + 8)), family="peaked" if (_o // 8) % 2 else "flat"))
    OWN_SLOT.append(case(_f, [_kpr + o for o in (0, 1, kpi(_f) - 1, kpi(_f), _kpr // 2 + 1, _kpr - 1)] + [2 * _kpr + 3, 2 * _kpr + kpi(_f) + 2], family="flat"))
# the prefix: pre in {0, 1, KPI - 1, KPI + 1, one round, pos, 125}; rows of a launch: two voices, no voice, rows sharing a voice
PREFIX = []
for _f in FMTS:
    _kpr, _k = keys_per_round(_f), kpi(_f)
    PREFIX += [
        case(_f, [(1, 0), (_k + 4, 1), (9, -1), (20, 0), (_k - 1, 1), (_k, 1)], voices=(1, _k - 1)),
        case(_f, [(_kpr + 3, 0), (_kpr, 1), (2 * _kpr + 1, 1), (7, -1), (_k + 1, 0), (_k + 2, 0)], voices=(_k + 1, _kpr)),
        case(_f, [(125, 0), (140, 0), (200, 0), (130, -1), (1, 1), (126, 0), (255, 0)], voices=(125, 1)),
        case(_f, [(125, 0), (128, 0), (131, -1), (_kpr + 2, 1), (190, 0)], voices=(125, _kpr), family="peaked"),
        case(_f, [(125, 0), (_kpr, 1), (40, -1), (125, 0), (_kpr, 1)], voices=(125, _kpr), tag="allprefix"),   # every cached key of a voiced row from the prefix
    ]
# padding: canonical NaNs (not 0xff bytes) at and beyond pos, and in the own rows below pre
PADDING = [case(_f, [(0, -1), (kpi(_f) + 3, 1), (37, -1), (125, 0), (150, 0), (1, -1)], voices=(125, kpi(_f) + 1), pad="nan") for _f in FMTS]
# inactive rows next to live ones
INACTIVE = [case(_f, [(40, 0), (60, 0, 0), (3, -1), (0, -1, 0), (90, 1, 0), (33, 1)], voices=(keys_per_round(_f), 33)) for _f in FMTS]
# the first step of a slot: no key in memory, the own cache holds NaNs
FIRST = [case(_f, [0, 0], keys_now=kn, pad=pad, tag="first") for _f in FMTS for kn, pad in (("exact", "ff"), (0, "nan"))]
# keys_now forms (test_keys_now_forms_give_the_same_bits runs each at 0, exact and beyond the capacity)
FORMS = [case(_f, [(keys_per_round(_f) + 3, 0), (7, -1), (2 * keys_per_round(_f), 1), (0, -1), (50, 0, 0)], voices=(kpi(_f) + 1, 2 * keys_per_round(_f)),
              family=fam, tag="forms") for _f in FMTS for fam in ("flat", "peaked")]
# beyond one burst launch_attention hands the fused step to k_attention, which reads the slot's own copy of the prefix.  The hook refuses seg_len >= cap, so
# the offsets beyond the burst (260, 264 / 516, 520) need a capacity above them: 272 / 528 beside the first capacity that leaves k_attn_step (257 / 513)
FALLBACK = []
for _f in FMTS:
    _b = BURST[_f]
    FALLBACK += [
        case(_f, [(_b, 0), (_b - 1, -1), (130, 0), (0, -1), (17, 1), (_b // 2, -1, 0)], voices=(125, 17), cap=_b + 1, own_copy=True),
        case(_f, [(_b + 4, 0), (_b + 8, -1), (_b, 1), (3, -1), (125, 0)], voices=(125, keys_per_round(_f)), cap=_b + 16, own_copy=True, family="peaked"),
        case(_f, [(_b + 8, -1), (_b - 3, 1), (40, 0)], voices=(33, kpi(_f) - 1), cap=_b + 16, own_copy=True),
    ]
# operands both kernels accept: the own copy of the prefix present, once at the burst capacity and once one key above it
BOTH = [(case(_f, rows, voices=(125, 9), cap=BURST[_f], own_copy=True, family=fam, tag="both"),
         case(_f, rows, voices=(125, 9), cap=BURST[_f] + 1, own_copy=True, family=fam, tag="both"))
        for _f in FMTS for fam in ("flat", "peaked") for rows in ([(BURST[_f] - 1, 0), (126, 0), (9, 1), (60, -1), (0, -1)],)]
STEP_CASES = EVERY_NI + OWN_SLOT + PREFIX + PADDING + INACTIVE + FIRST + FORMS + [b[0] for b in BOTH]
ALL_CASES = STEP_CASES + FALLBACK + [b[1] for b in BOTH]


# ------------------------------------------------------------------------------------------------ operands and the f64 reference
@functools.lru_cache(maxsize=None)
def _operands(key):
    c = CASE_BY_ID[key]
    fmt, cap, rows = c["fmt"], c["cap"], c["rows"]
    n = len(rows)
    # (the seed leaves the capacity out: the two cases of a BOTH pair draw the same numbers)
    rng = np.random.default_rng(zlib.crc32(f"{fmt} {rows} {c['voices']} {c['family']} {c['tag']}".encode()))
    qkv = np.full((n, QLD), np.nan, F32)   # (the two padding columns: NaN)
    qkv[:, :D] = (0.25 if c["family"] == "flat" else 1.0) * rng.standard_normal((n, D))
    qkv[:, D:3 * D] = rng.standard_normal((n, 2 * D))
    ang = rng.uniform(-np.pi, np.pi, (BURST[fmt] + 16, 32))[:cap]
    cos, sin = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
    vk = [to_fmt(rng.standard_normal((LAYERS, H, L, 64)), fmt) for L in c["voices"]]
    vv = [to_fmt(rng.standard_normal((LAYERS, H, L, 64)), fmt) for L in c["voices"]]
    kv = to_fmt(rng.standard_normal((2, n, H, BURST[fmt] + 16, 64)), fmt)[:, :, :, :cap]
    k, v = to_bits(kv[0], fmt), to_bits(kv[1], fmt)
    fill = fill_bits(fmt, c["pad"])
    for r, (pos, vo, act) in enumerate(rows):
        if not act:
            continue   # an inactive row's cache: finite data everywhere, and it must come back unchanged
        pre = c["voices"][vo] if vo >= 0 else 0
        k[r, :, pos:], v[r, :, pos:] = fill, fill
        if c["own_copy"] and pre:
            k[r, :, :pre], v[r, :, :pre] = to_bits(vk[vo][LAYER], fmt), to_bits(vv[vo][LAYER], fmt)
        else:
            k[r, :, :pre], v[r, :, :pre] = fill, fill
    return dict(qkv=qkv, cos=cos, sin=sin, k=k, v=v, vk=vk, vv=vv, pre_k=[to_bits(a, fmt) for a in vk], pre_v=[to_bits(a, fmt) for a in vv],
                seg_len=np.array([p for p, _, _ in rows], np.int32), active=np.array([a for _, _, a in rows], np.int32),
                pre_len=np.array([c["voices"][vo] if vo >= 0 else 0 for _, vo, _ in rows], np.int32), voice_of_row=np.array([vo for _, vo, _ in rows], np.int32))


def operands(c):
    return _operands(cid(c))


def rope64(x, cos, sin):
    """x [..., 64] rotated in pairs (2t, 2t + 1) by the table row; also |x0 c| + |x1 s| per element (the scale of the rotation's rounding error)"""
    x = np.asarray(x, np.float64)
    c, s = np.asarray(cos, np.float64), np.asarray(sin, np.float64)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    out, mag = np.empty_like(x), np.empty_like(x)
    out[..., 0::2], out[..., 1::2] = x0 * c - x1 * s, x0 * s + x1 * c
    mag[..., 0::2], mag[..., 1::2] = np.abs(x0 * c) + np.abs(x1 * s), np.abs(x0 * s) + np.abs(x1 * c)
    return out, mag


def row_keys(c, o, r, own_k=None):
    """(q [H, 64], K [H, pos + 1, 64], V [H, pos + 1, 64], k_want [H, 64], k_mag [H, 64], v_own bits [H, 64]) of live row r in f64"""
    fmt = c["fmt"]
    pos, vo, _ = c["rows"][r]
    pre = c["voices"][vo] if vo >= 0 else 0
    x = o["qkv"][r, :3 * D].reshape(3, H, 64)
    q, _ = rope64(x[0], o["cos"][pos], o["sin"][pos])
    k_want, k_mag = rope64(x[1], o["cos"][pos], o["sin"][pos])
    v_own = to_fmt(x[2], fmt)
    if own_k is None:
        own_k = to_fmt(k_want.astype(F32), fmt)
    K, V = np.empty((H, pos + 1, 64)), np.empty((H, pos + 1, 64))
    if pre:
        K[:, :pre], V[:, :pre] = o["vk"][vo][LAYER], o["vv"][vo][LAYER]
    K[:, pre:pos], V[:, pre:pos] = from_bits(o["k"][r, :, pre:pos], fmt), from_bits(o["v"][r, :, pre:pos], fmt)
    K[:, pos], V[:, pos] = own_k, v_own
    return q, K, V, k_want, k_mag, to_bits(v_own, fmt)


def softmax_pv(q, K, V):
    """(out [H, 64], weights [H, nk], scores [H, nk]) in f64"""
    s = np.einsum("he,hje->hj", q, K) * 0.125
    w = np.exp(s - s.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    return np.einsum("hj,hje->he", w, V), w, s


def bound(q, K, V):
    """the docstring's bound per output element [H, 64]"""
    A = np.einsum("he,hje->hj", np.abs(q), np.abs(K)).max(axis=1)   # [H]
    ds = 0.125 * 13 * U * A
    return np.minimum(CEIL, np.abs(V).max(axis=1) * (4 * ds + 167 * U)[:, None])


def reference(c, own_k=None):
    """out [rows, D] (zeros for inactive rows), bound [rows, D]; own_k [rows, H, 64]: the stored keys to use at `pos` (default: the f64 rotation, rounded)"""
    o = operands(c)
    n = len(c["rows"])
    out, bnd = np.zeros((n, D)), np.zeros((n, D))
    for r, (_, _, act) in enumerate(c["rows"]):
        if act:
            q, K, V = row_keys(c, o, r, None if own_k is None else own_k[r])[:3]
            out[r], bnd[r] = softmax_pv(q, K, V)[0].reshape(D), bound(q, K, V).reshape(D)
    return out, bnd


CASE_BY_ID = {cid(c): c for c in ALL_CASES}


def test_case_ids_are_unique_and_name_format_rounds_and_offsets():
    assert len(CASE_BY_ID) == len(ALL_CASES)
    for c in ALL_CASES:
        assert cid(c).startswith(f"{c['fmt']}-ni{c['ni']}-pos") and "-pre" in cid(c)
        assert len(c["rows"]) <= 8 and all(0 <= p < c["cap"] for p, _, _ in c["rows"])


def test_cases_reach_every_instantiation(pkg):
    """all 32 (KVBF16, NI) instantiations of k_attn_step are launched by some case; the launcher's round count, restated in rounds() above, is the library's
    (attn_step_rounds / attn_step_keys_per_round through the hook, no GPU) for every key count a launch here can have."""
    assert {(c["fmt"], c["ni"]) for c in EVERY_NI} == {(f, ni) for f in FMTS for ni in range(1, 17)}
    assert {(c["fmt"], c["ni"]) for c in STEP_CASES} == {(f, ni) for f in FMTS for ni in range(1, 17)}
    for f in FMTS:
        for keys in range(0, 600):
            assert pkg.runtime.attn_step_rounds(keys, f == "bf16") == (rounds(keys, f), keys_per_round(f)), (f, keys)
    for c in EVERY_NI:   # rows at the last and the first slot of the last round
        kpr = keys_per_round(c["fmt"])
        assert c["rows"][0][0] == c["ni"] * kpr - 1 and c["rows"][1][0] == (c["ni"] - 1) * kpr and all(p < c["keys_now"] for p, _, _ in c["rows"])


def test_cases_reach_every_own_key_slot_and_prefix_boundary():
    """g_p = pos / KPI, i_p = g_p >> 2, w_p = g_p & 3, kq_p = pos % KPI: every (w_p, kq_p) at i_p = 0, some at i_p = 1 and 2; the prefix lengths the issue lists."""
    for f in FMTS:
        k = kpi(f)
        slots = {((p // k) >> 2, (p // k) & 3, p % k) for c in OWN_SLOT if c["fmt"] == f for p, _, _ in c["rows"]}
        assert {(0, w, q) for w in range(4) for q in range(k)} <= slots
        assert sum(1 for i, _, _ in slots if i == 1) >= 5 and any(i == 2 for i, _, _ in slots)
        pres = set()
        for c in PREFIX:
            if c["fmt"] == f:
                vos = [vo for _, vo, _ in c["rows"]]
                assert -1 in vos and len({vo for vo in vos if vo >= 0}) == 2 and max(vos.count(0), vos.count(1)) >= 2   # two voices, none, a shared one
                pres |= {(c["voices"][vo] if vo >= 0 else 0, p) for p, vo, _ in c["rows"]}
        assert {0, 1, k - 1, k + 1, keys_per_round(f), 125} <= {pre for pre, _ in pres}
        assert sum(1 for pre, p in pres if pre == p and pre > 0) >= 4   # every cached key from the prefix


def test_flat_cases_feel_every_key():
    """for every flat case, live row and head: removing any one key, and replacing any key's K and V rows by its neighbour's, moves the f64 reference by at
    least 10 x the tolerance (max over the 64 elements against the largest element tolerance) -- what makes a dropped, duplicated or mis-sourced key fail."""
    worst = {}
    for c in ALL_CASES:
        if c["family"] != "flat":
            continue
        o = operands(c)
        for r, (pos, _, act) in enumerate(c["rows"]):
            if not act or pos == 0:
                continue
            q, K, V = row_keys(c, o, r)[:3]
            out, w, s = softmax_pv(q, K, V)
            tol = bound(q, K, V).max(axis=1)   # [H]
            drop = np.abs(w[:, :, None] * (out[:, None, :] - V) / (1.0 - w[:, :, None])).max(axis=2)   # [H, nk]
            e = np.exp(s - s.max(axis=1, keepdims=True))
            Z, N = e.sum(axis=1), np.einsum("hj,hje->he", e, V)
            nb = np.r_[np.arange(1, pos + 1), pos - 1]   # the neighbour of key j: j + 1, of the last key: j - 1
            Z2 = Z[:, None] - e + e[:, nb]
            N2 = N[:, None, :] - e[:, :, None] * V + e[:, nb, None] * V[:, nb]
            swap = np.abs(N2 / Z2[:, :, None] - out[:, None, :]).max(axis=2)
            ratio = min(float((drop / tol[:, None]).min()), float((swap / tol[:, None]).min()))
            worst[cid(c), r] = ratio
            assert ratio >= 10.0, (cid(c), r, pos, float(drop.min()), float(swap.min()), tol)
    assert len(worst) > 100
    print("smallest move / tolerance:", min(worst.values()))


def test_peaked_cases_keep_the_spread_the_bound_assumes():
    """max(sc) - min(sc) <= 16 (the argument of __expf the bound is derived for), and the peaked family really is peaked: a spread above 3 at 60+ keys"""
    for c in ALL_CASES:
        o = operands(c)
        for r, (pos, _, act) in enumerate(c["rows"]):
            if act:
                q, K, V = row_keys(c, o, r)[:3]
                s = softmax_pv(q, K, V)[2]
                spread = s.max(axis=1) - s.min(axis=1)
                assert (spread <= 16.0).all(), (cid(c), r, spread)
                if c["family"] == "peaked" and pos >= 60:
                    assert (spread > 3.0).all(), (cid(c), r, spread)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in numpy f32 (no GPU)
def emulate(c):
    """k_attn_step in numpy f32, in the kernel's order: the rotation in f32, the dot as DPL products per lane and a butterfly over the key's lanes, exp in f32,
    the sums per lane group over the NI slots, (bf16) the two key groups of a row, then the 16 rows in order.  Returns (out [rows, D] f32, own_k [rows, H, 64])."""
    o = operands(c)
    fmt = c["fmt"]
    lpk = 8 if fmt == "bf16" else 16
    k_, dpl, ni = 64 // lpk, 64 // lpk, max(c["ni"], 1) if c["kernel"] == "k_attn_step" else 16 * ((c["cap"] + BURST[fmt] - 1) // BURST[fmt])
    n = len(c["rows"])
    out, own = np.zeros((n, D), F32), np.zeros((n, H, 64), F32)
    for r, (pos, _, act) in enumerate(c["rows"]):
        if not act:
            continue
        x = o["qkv"][r, :3 * D].reshape(3, H, 64)
        cs, sn = o["cos"][pos], o["sin"][pos]

        def rot(a):
            y = np.empty((H, 64), F32)
            y[:, 0::2] = a[:, 0::2] * cs - a[:, 1::2] * sn
            y[:, 1::2] = a[:, 0::2] * sn + a[:, 1::2] * cs
            return y
        qs, own[r] = rot(x[0]), to_fmt(rot(x[1]), fmt)
        _, K, V = row_keys(c, o, r, own[r])[:3]
        slots = ni * 4 * k_
        Ks, Vs = np.zeros((H, slots, 64), F32), np.zeros((H, slots, 64), F32)
        Ks[:, :pos + 1], Vs[:, :pos + 1] = K, V
        valid = np.arange(slots) <= pos
        prod = (qs[:, None, :] * Ks).reshape(H, slots, lpk, dpl)
        part = prod[..., 0]
        for e in range(1, dpl):
            part = part + prod[..., e]          # [H, slots, lpk]: the lane's sum
        while part.shape[-1] > 1:               # lanes ^1, ^2, the other quad, (f32) the other half
            part = part[..., 0::2] + part[..., 1::2]
        sc = np.where(valid, part[..., 0] * F32(0.125), F32(-np.inf)).astype(F32)
        mx = sc.max(axis=1, keepdims=True)
        p = np.exp(sc - mx).astype(F32)          # [H, slots]
        # slot jj = (i * 4 + wave) * KPI + kq
        p4 = p.reshape(H, ni, 4, k_)
        v4 = Vs.reshape(H, ni, 4, k_, 64)
        l, ov = np.zeros((H, 4, k_), F32), np.zeros((H, 4, k_, 64), F32)
        for i in range(ni):
            l = l + p4[:, i]
            ov = ov + p4[:, i, :, :, None] * v4[:, i]
        if lpk == 8:                             # the other key group of the 16-lane row
            l, ov = l[:, :, 0::2] + l[:, :, 1::2], ov[:, :, 0::2] + ov[:, :, 1::2]
        l, ov = l.reshape(H, 16), ov.reshape(H, 16, 64)   # row = wave * 4 + (lane >> 4)
        den, num = np.zeros(H, F32), np.zeros((H, 64), F32)
        for row in range(16):
            den, num = den + l[:, row], num + ov[:, row]
        out[r] = (num / den[:, None]).reshape(D)
    return out, own


def test_emulation_stays_within_half_the_bound():
    worst = 0.0
    for c in ALL_CASES:
        got, own = emulate(c)
        want, bnd = reference(c, own)
        live = np.array([a for _, _, a in c["rows"]], bool)
        ratio = float((np.abs(got[live] - want[live]) / bnd[live]).max())
        worst = max(worst, ratio)
        assert np.isfinite(got).all() and ratio <= 0.5, (cid(c), ratio)
        assert (bnd[live] > 0).all() and (bnd <= CEIL).all()
    print("emulation: largest error / bound", worst)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
FILL = np.uint32(0xFFFFFFFF)


def run(pkg, c, **over):
    o = operands(c)
    kw = dict(kv_bf16=c["fmt"] == "bf16", heads=H, layers=LAYERS, layer=LAYER, keys_now=c["keys_now"], active=o["active"], pre_len=o["pre_len"],
              voice_of_row=o["voice_of_row"], pre_k=o["pre_k"], pre_v=o["pre_v"], out_ld=OLD)
    kw.update(over)
    return pkg.runtime.debug_attn_step(kw.pop("qkv", o["qkv"]), o["cos"], o["sin"], kw.pop("seg_len", o["seg_len"]), kw.pop("k", o["k"]), kw.pop("v", o["v"]), **kw)


def check(c, r, name=None, slack=1.0):
    """every property of one launch's result: the kernel and round count the launcher picked, untouched padding columns, zeros and unchanged caches for inactive
    rows, no cache byte changed but row `pos`, V row `pos` bit for bit, K row `pos` against the f64 rotation, the output against the reference within the
    bound (recorded through _parity.record: profiles/attn_step_parity.txt is one run's summary).  Returns the largest error / bound."""
    o = operands(c)
    fmt = c["fmt"]
    name = name or f"{c['kernel']} {cid(c)}"
    assert r["kernel"] == c["kernel"], (name, r["kernel"])
    assert r["launches"] == 1 and r[c["kernel"]] == 1 and r["rounds"] == c["ni"], (name, r["launches"], r["rounds"])
    out = r["out"]
    assert (out[:, D:].view(np.uint32) == FILL).all(), name + ": the padding columns of the output were written"
    own = np.zeros((len(c["rows"]), H, 64), F32)
    for i, (pos, _, act) in enumerate(c["rows"]):
        if not act:
            assert (out[i, :D].view(np.uint32) == 0).all(), f"{name}: inactive row {i} is not exact zeros"
            assert np.array_equal(r["k"][i], o["k"][i]) and np.array_equal(r["v"][i], o["v"][i]), f"{name}: inactive row {i}'s cache changed"
            continue
        keep = np.arange(c["cap"]) != pos
        assert np.array_equal(r["k"][i][:, keep], o["k"][i][:, keep]), f"{name}: row {i}: K cache rows other than {pos} changed"
        assert np.array_equal(r["v"][i][:, keep], o["v"][i][:, keep]), f"{name}: row {i}: V cache rows other than {pos} changed"
        _, _, _, k_want, k_mag, v_bits = row_keys(c, o, i)
        assert np.array_equal(r["v"][i][:, pos], v_bits), f"{name}: row {i}: V row {pos} is not the input rounded to the cache format"
        own[i] = from_bits(r["k"][i][:, pos], fmt)
        k_bound = 2.0 ** -22 * k_mag + (2.0 ** -8 * np.abs(k_want) if fmt == "bf16" else 0.0)
        k_err = np.abs(own[i].astype(np.float64) - k_want)
        assert np.isfinite(own[i]).all() and (k_err <= k_bound).all(), f"{name}: row {i}: K row {pos} misses the f64 rotation by {float((k_err / k_bound).max()):.2f} bounds"
    want, bnd = reference(c, own)
    live = np.array([a for _, _, a in c["rows"]], bool)
    got = out[:, :D]
    assert np.isfinite(got).all(), name + ": non-finite output"
    err = np.abs(got[live].astype(np.float64) - want[live])
    worst = float((err / (slack * bnd[live])).max())
    record(name, float(err.max()), worst, float(np.abs(want).max()), (CEIL, 0))   # (max_rel slot: error / bound)
    print(f"{name}: max abs {float(err.max()):.3e}, error / bound {worst:.3f}")
    assert worst <= 1.0, (name, float(err.max()), worst)
    return worst


@gpu
@pytest.mark.parametrize("c", EVERY_NI, ids=cid)
def test_every_instantiation(pkg, c):
    """KVBF16 x NI = 1..16, each by a keys_now that yields it: rows at the last and the first slot of the last round and at two small offsets."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("c", OWN_SLOT, ids=cid)
def test_own_key_slot(pkg, c):
    """this step's own k and v reach the sums from LDS through exactly one slot (i_p, w_p, kq_p): every (w_p, kq_p), and i_p = 1 and 2; the rows of a launch sit
    at different offsets.  Cache row `pos` holds 0xff bytes before the launch: a slot that takes it from memory instead reads NaN or the clamp row."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("c", PREFIX, ids=cid)
def test_prefix_is_read_from_the_voice(pkg, c):
    """keys j < pre come from the voice's buffer at `layer` (the slot's own rows j < pre hold 0xff bytes), keys pre <= j < pos from the slot: pre = 0, 1,
    KPI - 1, KPI + 1, one round, pos and 125, two voices, no voice and a shared voice in one launch."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("c", PADDING, ids=cid)
def test_nan_padding_never_reaches_the_output(pkg, c):
    """canonical NaNs at and beyond pos (the padding of a voice state, attention.go:402-406) and in the own rows below pre: the output is finite and right."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("c", INACTIVE, ids=cid)
def test_inactive_rows_write_zeros_and_append_nothing(pkg, c):
    """next to live rows of the same launch: exact zeros, both caches byte for byte the input."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("c", FIRST, ids=cid)
def test_first_step_of_a_slot_whose_cache_holds_nan(pkg, c):
    """pos = 0, pre = 0: the only key is the step's own, so out = v in the cache format, bit for bit, whatever the cache holds.  Reachable through the public
    API: ptts_batch_step asks for no prompt (capi.cpp: a fresh or reset batch steps at length 0), batch_reset sets the lengths to 0 and leaves the cache bytes
    of the last tenant, and ptts_batch_set_voice accepts a state of offset 0 with NaN-padded rows (check_voice).  Before the early exit at pos == 0 every slot
    of the burst re-read own row 0, zero weight times NaN was NaN, and the whole output row was NaN (at any NI)."""
    r = run(pkg, c)
    check(c, r)
    o = operands(c)
    v = to_fmt(o["qkv"][:, 2 * D:3 * D], c["fmt"])
    assert np.array_equal(r["out"][:, :D].view(np.uint32), v.view(np.uint32))


@gpu
@pytest.mark.parametrize("c", FORMS, ids=cid)
def test_keys_now_forms_give_the_same_bits(pkg, c):
    """keys_now exact, 0 (unknown: NI from the capacity) and beyond the capacity: output and caches bit for bit the same (slots past the end weigh exp(-inf) = 0
    times a finite row), and a second run of one form repeats the first.  NI independence is what lets graph replay (NI from capture_keys) equal plain launches."""
    first = run(pkg, c)
    check(c, first)
    cap = c["cap"]
    for kn in (0, cap + 100, c["keys_now"]):
        r = run(pkg, c, keys_now=kn)
        assert r["kernel"] == "k_attn_step" and r["rounds"] == launch_rounds(kn, cap, c["fmt"]), (kn, r["rounds"])
        for what in ("out", "k", "v"):
            assert np.array_equal(np.ascontiguousarray(r[what]).view(np.uint8), np.ascontiguousarray(first[what]).view(np.uint8)), (cid(c), kn, what)
    assert launch_rounds(0, cap, c["fmt"]) == 16 and c["ni"] < 16


@gpu
@pytest.mark.parametrize("c", FALLBACK, ids=cid)
def test_beyond_one_burst_k_attention_takes_the_step(pkg, c):
    """capacity 257 (f32) / 513 (bf16) and above: k_attention<4, KVBF16> with the fused step, against the same reference (it reads the slot's own copy of the
    prefix), with offsets at and beyond the burst (256, 260, 264 / 512, 516, 520)."""
    check(c, run(pkg, c))


@gpu
@pytest.mark.parametrize("pair", BOTH, ids=lambda p: cid(p[0]))
def test_both_kernels_agree_where_both_apply(pkg, pair):
    """the same operands (own copy of the prefix present) at the burst capacity (k_attn_step) and one key above it (k_attention): each within the bound of the
    reference, and within twice the bound of each other."""
    a, b = pair
    ra, rb = run(pkg, a), run(pkg, b)
    check(a, ra)
    check(b, rb)
    assert (ra["kernel"], rb["kernel"]) == ("k_attn_step", "k_attention")
    _, bnd = reference(a)
    live = np.array([x for _, _, x in a["rows"]], bool)
    d = np.abs(ra["out"][live, :D].astype(np.float64) - rb["out"][live, :D])
    assert (d <= 2 * bnd[live]).all(), float((d / bnd[live]).max())


@gpu
def test_dispatch_by_capacity(pkg):
    """256 / 512 keys of capacity: k_attn_step; 257 / 513: k_attention."""
    for f in FMTS:
        for cap, want in ((BURST[f], "k_attn_step"), (BURST[f] + 1, "k_attention")):
            c = case(f, [5, (9, 0)], voices=(3,), cap=cap, own_copy=True, tag="dispatch")
            CASE_BY_ID[cid(c)] = c
            r = run(pkg, c)
            assert r["kernel"] == want and pkg.runtime.last_attention_kernel() == want
            check(c, r)


@gpu
def test_refusals_before_any_launch(pkg):
    """everything that could send the kernel outside the hook's buffers is PTTS_EINVAL, and nothing is launched."""
    c = PREFIX[1]   # voices of KPI + 1 and one round
    o = operands(c)
    n = len(c["rows"])

    def arr(a, i, val):
        a = a.copy()
        a[i] = val
        return a
    bad = {
        "seg_len == cap": dict(seg_len=arr(o["seg_len"], 3, c["cap"]), keys_now=0),
        "seg_len < 0": dict(seg_len=arr(o["seg_len"], 3, -1)),
        "pre_len > seg_len": dict(seg_len=arr(o["seg_len"], 0, 2)),
        "pre_len not the buffer's length": dict(pre_len=arr(o["pre_len"], 0, o["pre_len"][0] - 1)),
        "pre_len without a voice": dict(voice_of_row=arr(o["voice_of_row"], 0, -1)),
        "voice out of range": dict(voice_of_row=arr(o["voice_of_row"], 3, 2)),
        "keys_now below a live row": dict(keys_now=c["keys_now"] - 1),
        "qkv_ld < 3 d_model": dict(qkv=o["qkv"][:, :3 * D - 2]),
        "out_ld < d_model": dict(out_ld=D - 4),
        "layer == layers": dict(layer=LAYERS),
        "layer < 0": dict(layer=-1),
    }
    assert n > 3 and o["pre_len"][0] > 2 and o["voice_of_row"][3] == -1
    pkg.runtime.launch_counts(True)
    try:
        for what, kw in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                run(pkg, c, **kw)
            assert e.value.code == pkg.runtime.PTTS_EINVAL, what
            assert pkg.runtime.launch_counts(True) == {}, what
        check(c, run(pkg, c))   # ... and the operands themselves are taken: the same census sees that launch
        assert pkg.runtime.launch_counts(True) == {"k_attn_step": 1}
        # keys_now counts live rows only: an inactive row beyond it is no refusal
        ci = INACTIVE[0]
        check(ci, run(pkg, ci))
        assert max(p for p, _, a in ci["rows"] if not a) + 1 > ci["keys_now"]
    finally:
        pkg.runtime.launch_counts(False)
