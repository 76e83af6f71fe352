"""The fused SEANet blocks (csrc/resblock.hip: k_resblock; csrc/resblock_up.hip: k_resblock_up) stand-alone, value by value, against f64 numpy on the same
operands -- every kernel instance and both launch forms.

What they replace (mimi.go:146-164, 740-788): a residual block on channels-last rows with two rows of zero history,
    hidden[t] = elu(b1 + W1 . (elu u[t-2] | elu u[t-1] | elu u[t]))        W1 [H][3 C], tap-major
    s[t]      = elu(u[t] + b2 + W2 . hidden[t])                            W2 [C][H]             (every reader of the sum applies ELU first: uo = s)
and, for the last block, the model's final causal convolution  pcm[t] = bf + sum_{tap, c} s[t-2+tap][c] wf[tap C + c]  with zeros before row 0; the fused
kernel makes u itself, u[4 t + r][oc] = bup[oc] + (x[t-1] | x[t]) . Wup[r 64 + oc]  (the transposed convolution 128 -> 64, stride 4, as a product: x[t-1]
meets the taps r + 4, x[t] the taps r).  The hook (ptts_debug_resblock) packs the weights with the model loader's packers, fills every output with 0xff bytes
first (a NaN where nothing is stored), puts NaN into the slack rows behind every utterance and returns the buffers whole.

Kernel instances (FORMS; every test id carries one): k_resblock<C, H, NW, FINAL, WBF16, PERS> at 64 / 32 and 128 / 64 channels, with and without the final
convolution, bf16 or f32 (hi + lo) weights, one tile per block ("tile") or persistent blocks walking the tiles ("pers": 64-wide final and 128-wide plain,
bf16) -- ten of them -- and k_resblock_up ("up").  T is the number of new rows of a tile: 16 NW - 2, or - 4 with the final convolution.

Reference: f64 numpy on the operands the kernel multiplies: W1, W2 and Wup rounded to bf16 (round to nearest even) when w_bf16 and f32 otherwise, wf always f32
(the kernels keep it as hi + lo planes in either mode), activations and biases f32, ELU by expm1.

Bound (derived, not measured): a product's error is <= TOL (sum_k |a_k w_k| + |bias| + |residual|) + FLOOR, TOL = 3e-5, FLOOR = 1e-6 -- the bf16 hi + lo split of
the activations (2^-17), the same split of f32 weights with lo * lo dropped and f32 accumulation; tests/test_gpu_step_linear.py and tests/test_gpu_tall.py use
the same.  It is propagated through the stages with ELU's Lipschitz constant 1:
    E_u      = 0, or TOL (|Wup| . |x| + |bup|) + FLOOR when the transposed convolution is fused
    E_hidden = |W1| . E_u + TOL (|W1| . |elu u| + |b1|) + FLOOR
    E_sum    = E_u + |W2| . E_hidden + TOL (|W2| . |hidden| + |b2| + |u|) + FLOOR
    E_pcm    = |wf| . E_sum (three taps) + TOL (|wf| . |sum| + |bf|) + FLOOR
The kernels' ELU is exp(x) - 1 with the fast exponential: one v_exp_f32 on x log2(e), relative error ~(|x| + 2) 2^-24, and |x| e^x <= 1 / e on (-inf, 0], so at
most about 2^-23 absolute -- below FLOOR, which every stage adds once: it needs no term of its own.  The bound is per element; every element is compared.
test_emulation_stays_within_half_the_bound (no GPU) runs a numpy emulation of the kernels' arithmetic over every case of this file and holds it to HALF the
bound; test_planted_defects_are_caught (no GPU) shows that the defects a tile kernel can have exceed it on named cases.

Operands: u ~ 2 N(0, 1) with a few exact zeros and a few values at -30 (exp saturates: both ELU branches), weights N(0, 1) / sqrt(fan_in) (the final
convolution's with one dominant channel per tap, so that a sample is not an average that hides its operands' low bits), seeds from the data part of the case id (width, length, variant), so that forms which must agree bit for bit see the same numbers."""
import dataclasses
import os
import sys
import tempfile
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_bits, bf16_round, elu64, untouched
from _parity import record

TOL = 3e-5
FLOOR = 1e-6
F32 = np.float32
F64 = np.float64
B = 3
WFS = 0.1      # scale of the final convolution's weights: samples of a few units, a fair share of them inside [-1, 1]

# id -> (C, final, bf16 weights, persistent, fused transposed convolution, T = new rows per tile)
FORMS = {
    "c64-plain-bf16-tile": (64, 0, 1, 0, 0, 126), "c64-plain-f32-tile": (64, 0, 0, 0, 0, 126),
    "c64-final-bf16-tile": (64, 1, 1, 0, 0, 124), "c64-final-f32-tile": (64, 1, 0, 0, 0, 124), "c64-final-bf16-pers": (64, 1, 1, 1, 0, 124),
    "c128-plain-bf16-tile": (128, 0, 1, 0, 0, 62), "c128-plain-f32-tile": (128, 0, 0, 0, 0, 62), "c128-plain-bf16-pers": (128, 0, 1, 1, 0, 94),
    "c128-final-bf16-tile": (128, 1, 1, 0, 0, 60), "c128-final-f32-tile": (128, 1, 0, 0, 0, 60),
    "up-final-bf16-pers": (64, 1, 1, 1, 1, 124),
}
PERS_FORMS = ["c64-final-bf16-pers", "c128-plain-bf16-pers", "up-final-bf16-pers"]
TILE_TWIN = {"c64-final-bf16-pers": "c64-final-bf16-tile", "c128-plain-bf16-pers": "c128-plain-bf16-tile"}   # same width and weights, one tile per block


# ------------------------------------------------------------------------------------------------ host arithmetic the launcher does (restated)
def plan(C, final, bf16, batch, rows, cus):
    """(waves per block, persistent, grid, tiles per utterance, new rows per tile) as resblock.hip resblock_plan picks them for the production path."""
    halo = 4 if final else 2
    if bf16 and ((C == 64 and final) or (C == 128 and not final)):
        nw = 8 if C == 64 else 6
        tout = nw * 16 - halo
        tiles = (rows + tout - 1) // tout
        resident = 2 * cus if C == 64 else cus          # two blocks per CU (77 KB of LDS), or one (139 KB)
        if batch * tiles >= resident * 8:                # every block gets eight tiles to amortise its weight copy
            return nw, 1, resident, tiles, tout
    nw = 8 if C == 64 else 4
    tout = nw * 16 - halo
    tiles = (rows + tout - 1) // tout
    return nw, 0, batch * tiles, tiles, tout


def plan_up(batch, rows, cus):
    """resblock_up.hip resblock_up_plan: always persistent, one block per CU; grid 0 = not taken (resblock_up_supported's threshold)."""
    tiles = (rows + 123) // 124
    return 8, 1, (cus if batch * tiles >= cus * 8 else 0), tiles, 124


def test_production_thresholds_are_the_stated_ones(pkg):
    """resblock_plan / resblock_up_plan (the one place that chooses a launch form) against their restatement above, around every threshold."""
    f = pkg.runtime.debug_resblock_plan
    for cus in (8, 256, 304):
        for C in (64, 128):
            for final in (0, 1):
                for bf16 in (0, 1):
                    tout = (8 if C == 64 else 6) * 16 - (4 if final else 2)
                    resident = 2 * cus if C == 64 else cus
                    for batch in (1, 3, 64):
                        edge = -(-resident * 8 // batch)          # tiles per utterance at which batch * tiles reaches the threshold
                        for tiles in {1, 2, max(1, edge - 1), edge, edge + 1}:
                            for rows in {(tiles - 1) * tout + 1, tiles * tout}:
                                assert f(C, final, bf16, batch, rows, cus) == plan(C, final, bf16, batch, rows, cus), (C, final, bf16, batch, rows, cus)
        for batch in (1, 3, 64):
            edge = -(-cus * 8 // batch)
            for tiles in {1, max(1, edge - 1), edge, edge + 1}:
                for rows in {(tiles - 1) * 124 + 1, tiles * 124}:
                    assert f(64, 1, 1, batch, rows, cus, fuse_up=True) == plan_up(batch, rows, cus), (batch, rows, cus)
    # at full size (64 x 10 s: 3.84 M rows at 128 channels, 15.36 M at 64) the persistent forms are what runs; a single utterance gets one tile per block
    assert plan(64, 1, 1, 64, 240000, 256)[:3] == (8, 1, 512) and plan(128, 0, 1, 64, 60000, 256)[:3] == (6, 1, 256) and plan_up(64, 240000, 256)[2] == 256
    assert plan(64, 1, 1, 1, 24000, 256)[1] == 0 and plan(128, 0, 1, 1, 6000, 256)[1] == 0 and plan_up(1, 24000, 256)[2] == 0
    # the forms the test hook may ask for: a persistent form only where an instance exists, with the grid it names
    assert f(64, 1, 1, 3, 253, 256, form=2, grid=2) == (8, 1, 2, 3, 124) and f(128, 0, 1, 3, 193, 256, form=2, grid=9) == (6, 1, 9, 3, 94)
    assert f(64, 0, 1, 3, 253, 256, form=2, grid=2)[0] == 0 and f(128, 1, 1, 3, 125, 256, form=2, grid=2)[0] == 0 and f(64, 1, 0, 3, 253, 256, form=2, grid=2)[0] == 0
    assert f(128, 0, 1, 64, 60000, 256, form=1) == (4, 0, 64 * 968, 968, 62)


# ------------------------------------------------------------------------------------------------ number formats
def elu32(v):
    """the kernels' form in f32: exp(v) - 1 on (-inf, 0]"""
    v = np.asarray(v, F32)
    return np.where(v > 0, v, np.exp(np.minimum(v, F32(0))).astype(F32) - F32(1)).astype(F32)


def pcm16(x):
    """audio.WritePCM16Samples' rule: clamp to [-1, 1], times 32767 in f64, truncate toward zero; NaN -> 0."""
    x = np.asarray(x, F32).astype(F64)
    return np.where(np.isnan(x), 0.0, np.trunc(np.clip(x, -1.0, 1.0) * 32767.0)).astype(np.int16)


# ------------------------------------------------------------------------------------------------ cases
def case(form, L, pad=2, slack=0, nob=(), t0=0, t1=None, grid=None, x_pad=1, alt=0, wfs=WFS):
    C, final, bf16, pers, fused, T = FORMS[form]
    tiles = ((L if t1 is None else t1) - t0 + T - 1) // T
    if pers and grid is None:
        grid = min(2, B * tiles)
    return dict(form=form, L=L, pad=pad, slack=slack, nob=tuple(nob), t0=t0, t1=L if t1 is None else t1, grid=grid, x_pad=x_pad, alt=alt, wfs=wfs)


def data_id(c):
    """what the operands depend on: width, fused or not, length, variant -- not the launch form, the weight format, pad, range or biases dropped"""
    C, _, _, _, fused, _ = FORMS[c["form"]]
    return f"{'up' if fused else 'c%d' % C}-L{c['L']}-v{c['alt']}-wf{c['wfs']}"


def cid(c):
    s = f"{c['form']}-L{c['L']}-pad{c['pad']}"
    s += f"-slack{c['slack']}" if c["slack"] else ""
    s += "".join(f"-no_{b}" for b in c["nob"])
    s += f"-rows{c['t0']}:{c['t1']}" if (c["t0"], c["t1"]) != (0, c["L"]) else ""
    s += f"-grid{c['grid']}" if c["grid"] else ""
    s += f"-xpad{c['x_pad']}" if FORMS[c["form"]][4] and c["x_pad"] != 1 else ""
    s += f"-v{c['alt']}" if c["alt"] else ""
    s += f"-wf{c['wfs']}" if c["wfs"] != WFS else ""
    return s


def lengths(form):
    """1, 3, T - 1, T, T + 1, 2 T + 5: below the halo, at, one below and one above a tile, three tiles.  The fused form's rows come in fours."""
    T = FORMS[form][5]
    return [4, 8, T - 4, T, T + 4, 2 * T + 8] if FORMS[form][4] else [1, 3, T - 1, T, T + 1, 2 * T + 5]


def three_tiles(form):
    return lengths(form)[-1]


def _values():
    out = []
    for form in FORMS:
        fused, final = FORMS[form][4], FORMS[form][1]
        for i, L in enumerate(lengths(form)):
            out.append(case(form, L, pad=(2, 5)[i % 2], slack=3 if i == 4 else 0, x_pad=(1, 3)[i % 2]))
        Lb = lengths(form)[4]                             # T + 1 (T + 4): two tiles, the second one nearly empty
        for b in ["b1", "b2"] + (["bf"] if final else []) + (["bup"] if fused else []):
            out.append(case(form, Lb, pad=5, nob=[b], x_pad=3 if b == "bup" else 1))
        out.append(case(form, Lb, nob=["b1", "b2"] + (["bf"] if final else []) + (["bup"] if fused else [])))
    return out


VALUES = _values()
WALKS = [case(form, three_tiles(form), grid=g) for form in PERS_FORMS for g in (2, 9, 1)]        # 3 utterances x 3 tiles: blocks of 5 + 4 tiles, 1 each, all 9


def _ranges():
    out = []
    for form in FORMS:
        C, final, bf16, pers, fused, T = FORMS[form]
        if not bf16 and C == 128:
            continue                                       # (the range arithmetic does not depend on the weight format: one f32 form is enough)
        L = three_tiles(form)
        for t0 in ((4, T, T + 4) if final else (7, T, T + 1)):
            out.append(case(form, L, t0=t0, t1=L - (4 if fused else 3), pad=(2, 5)[t0 % 2]))
    return out


RANGES = _ranges()
# row destinations: lim per utterance, f32 and int16 mixed in one launch; "t" stands for T, "l" for L
ROW_SETS = [((0, 0), (1, 1), (2, 0)), ((3, 1), (4, 0), ("t-1", 1)), (("t", 0), ("t+1", 1), ("l-1", 0)), (("l", 1), ("l+7", 0), ("t+1", 0)),
            (("l-1", 1), (2, 1), ("l+7", 1))]
ROW_FORMS = ["c64-final-bf16-tile", "c64-final-f32-tile", "c64-final-bf16-pers", "c128-final-bf16-tile", "c128-final-f32-tile", "up-final-bf16-pers"]


def row_table(form, L, rs):
    T = FORMS[form][5]
    val = lambda v: v if isinstance(v, int) else {"t-1": T - 1, "t": T, "t+1": T + 1, "l-1": L - 1, "l": L, "l+7": L + 7}[v]   # noqa: E731
    return [(val(v), s16) for v, s16 in rs]


ROWS = [(case(form, three_tiles(form), pad=(2, 5)[i % 2], wfs=20 * WFS if i == 3 else WFS), i) for form in ROW_FORMS for i in range(len(ROW_SETS))]
ROWS += [(case(form, three_tiles(form), t0=FORMS[form][5], t1=three_tiles(form) - 4), 2) for form in ("c64-final-bf16-pers", "c128-final-bf16-tile", "up-final-bf16-pers")]
ALL_CASES = VALUES + WALKS + RANGES + [c for c, _ in ROWS]


def test_cases_reach_every_kernel_form(pkg):
    """the ten k_resblock instances and k_resblock_up, each at every length of its set, with every bias absent once; what the hook would launch for a case is
    the form its id names (the hook's own plan, asked for 256 compute units -- the explicit forms do not depend on them)."""
    assert {c["form"] for c in VALUES} == set(FORMS) and len(FORMS) == 11
    for form, (C, final, bf16, pers, fused, T) in FORMS.items():
        assert T == (6 if pers and C == 128 else (8 if C == 64 else 4)) * 16 - (4 if final else 2)
        mine = [c for c in VALUES if c["form"] == form]
        assert {c["L"] for c in mine} >= set(lengths(form)) and {c["pad"] for c in mine} == {2, 5} and any(c["slack"] for c in mine)
        assert {b for c in mine for b in c["nob"]} == {"b1", "b2"} | ({"bf"} if final else set()) | ({"bup"} if fused else set())
        for c in mine:
            got = pkg.runtime.debug_resblock_plan(C, final, bf16, B, c["t1"] - c["t0"], 256, fuse_up=bool(fused), form=2 if pers else 1, grid=c["grid"] or 0)
            tiles = (c["L"] + T - 1) // T
            assert got == ((6 if C == 128 else 8) if pers else (8 if C == 64 else 4), pers, c["grid"] if pers else B * tiles, tiles, T), cid(c)
    assert {(c["form"], c["grid"]) for c in WALKS} == {(f, g) for f in PERS_FORMS for g in (2, 9, 1)}
    assert all((c["L"] + FORMS[c["form"]][5] - 1) // FORMS[c["form"]][5] == 3 for c in WALKS)         # 9 tiles: 5 + 4 for two blocks, crossing utterances
    for group in (VALUES, WALKS, RANGES):
        assert len({cid(c) for c in group}) == len(group)
    assert len({(cid(c), i) for c, i in ROWS}) == len(ROWS)
    assert max(c["pad"] + c["L"] + c["slack"] for c in ALL_CASES) <= 400
    lims = {(v, L) for form in ROW_FORMS for rs in ROW_SETS for (v, _), L in zip(row_table(form, three_tiles(form), rs), [three_tiles(form)] * 3)}
    assert {v % 4 for v, _ in lims} == {0, 1, 2, 3} and any(v == 0 for v, _ in lims) and any(v > L for v, L in lims)


def operands(c):
    C, final, bf16, pers, fused, T = FORMS[c["form"]]
    H, L = C // 2, c["L"]
    rng = np.random.default_rng(zlib.crc32(data_id(c).encode()))
    o = {}
    if fused:
        x = rng.standard_normal((B, L // 4, 128)).astype(F32)
        x[rng.random(x.shape) < 0.01] = 0.0
        o["x"] = x
        o["wup"] = (2.0 * rng.standard_normal((256, 256)) / np.sqrt(256.0)).astype(F32)
        o["bup"] = (0.5 * rng.standard_normal(64)).astype(F32)
    else:
        u = (2.0 * rng.standard_normal((B, L, C))).astype(F32)
        r = rng.random(u.shape)
        u[r < 0.01] = 0.0
        u[r > 0.995] = -30.0
        o["u"] = u
    o["w1"] = (rng.standard_normal((H, 3 * C)) / np.sqrt(3.0 * C)).astype(F32)
    o["w2"] = (rng.standard_normal((C, H)) / np.sqrt(float(H))).astype(F32)
    o["b1"] = (0.5 * rng.standard_normal(H)).astype(F32)
    o["b2"] = (0.5 * rng.standard_normal(C)).astype(F32)
    wf = c["wfs"] * rng.standard_normal(3 * C) / np.sqrt(3.0 * C)
    wf[rng.integers(0, C, 3) + C * np.arange(3)] *= 40.0        # one dominant channel per tap: a sample then shows its operands' low bits (the no_lo defect)
    o["wf"] = wf.astype(F32)
    o["bf"] = (0.1 * rng.standard_normal(1)).astype(F32)
    for b in c["nob"]:
        o[b] = None
    return o


# ------------------------------------------------------------------------------------------------ the operation, in f64 and as the kernels' arithmetic
def win(a, k, front=None):
    """[B][L][C] -> [B][L][k C]: rows t-k+1 .. t side by side, zeros (or `front` [k-1][C]) before row 0"""
    Bn, L, C = a.shape
    z = np.zeros((Bn, k - 1, C), a.dtype) if front is None else np.broadcast_to(front.astype(a.dtype), (Bn, k - 1, C))
    p = np.concatenate([z, a], axis=1)
    return np.concatenate([p[:, j:j + L] for j in range(k)], axis=2)


def kernel_product(x, w, lo_w):
    """x [.., K] f32 times w [N][K] as the kernels form it: x as bf16 hi + lo, w as bf16 hi (+ lo against x hi only), one f32 accumulator over the 32-deep
    matrix steps in k order: hi * hi, then hi-weight * lo-activation, then lo-weight * hi-activation"""
    x = np.ascontiguousarray(x, F32)
    shp = x.shape[:-1]
    x = x.reshape(-1, x.shape[-1])
    xh = bf16_round(x)
    xl = bf16_round(x - xh)
    wh = bf16_round(w)
    wl = bf16_round(np.asarray(w, F32) - wh) if lo_w else None
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for s in range(x.shape[1] // 32):
        k = slice(32 * s, 32 * s + 32)
        acc = acc + xh[:, k] @ wh[:, k].T
        acc = acc + xl[:, k] @ wh[:, k].T
        if lo_w:
            acc = acc + xh[:, k] @ wl[:, k].T
    return acc.reshape(shp + (w.shape[0],))


def weights(c, o):
    bf16 = FORMS[c["form"]][2]
    r = (lambda w: bf16_round(w)) if bf16 else (lambda w: w)
    z = lambda b, n: np.zeros(n, F32) if b is None else b   # noqa: E731
    C = FORMS[c["form"]][0]
    return dict(w1=r(o["w1"]), w2=r(o["w2"]), wf=o["wf"], wup=r(o["wup"]) if "wup" in o else None, b1=z(o["b1"], C // 2), b2=z(o["b2"], C), bf=z(o["bf"], 1),
                bup=z(o.get("bup"), 64))


def stage0(c, o, w, emulate=False, defect=None):
    """the block's input rows u [B][L][C] and their error bound: the operand itself, or the fused transposed convolution of x"""
    if "x" not in o:
        return (o["u"] if emulate else o["u"].astype(F64)), np.zeros(o["u"].shape, F64)
    xw = win(o["x"], 2)                                            # (x[t-1] | x[t]); x[-1] = 0
    Bn, xl, _ = xw.shape
    ab = np.abs(xw.astype(F64)) @ np.abs(w["wup"].astype(F64)).T + np.tile(np.abs(w["bup"].astype(F64)), 4)
    if emulate:
        u = kernel_product(xw, w["wup"], False) + np.tile(w["bup"], 4)
    else:
        xa = bf16_round(xw).astype(F64) if defect == "no_lo" else xw.astype(F64)
        u = xa @ w["wup"].astype(F64).T + np.tile(w["bup"].astype(F64), 4)
    return u.reshape(Bn, xl * 4, 64), (TOL * ab + FLOOR).reshape(Bn, xl * 4, 64)     # column (r, oc) of input row t is channel oc of output row 4 t + r


def block(c, w, u, Eu, emulate=False, defect=None):
    """u -> (uo, E_sum) or (pcm, E_pcm): f64 (with the bound of every output), or -- emulate -- the kernels' arithmetic in f32.  defect: a planted fault."""
    C, final, bf16 = FORMS[c["form"]][:3]
    dt = F32 if emulate else F64
    elu = elu32 if emulate else elu64
    act = (lambda a: bf16_round(a.astype(F32)).astype(F64)) if defect == "no_lo" else (lambda a: a)
    prod = (lambda a, m, lo: kernel_product(a, m, lo)) if emulate else (lambda a, m, lo: act(a) @ m.astype(F64).T)
    A = lambda m: np.abs(m.astype(F64))   # noqa: E731
    w1 = w["w1"]
    if defect == "taps_reversed":
        w1 = np.ascontiguousarray(w1.reshape(-1, 3, C)[:, ::-1].reshape(-1, 3 * C))
    b1 = np.zeros_like(w["b1"]) if defect == "no_b1" else w["b1"]
    b2 = np.zeros_like(w["b2"]) if defect == "no_b2" else w["b2"]
    bf = np.zeros_like(w["bf"]) if defect == "no_bf" else w["bf"]
    eu = elu(u)
    ew = win(eu, 3)
    hid = elu(prod(ew, w1, not bf16) + b1.astype(dt))
    E_h = win(Eu, 3) @ A(w["w1"]).T + TOL * (A(ew) @ A(w["w1"]).T + A(w["b1"])) + FLOOR
    res = u
    if defect == "residual_neighbour":                            # the residual of 4-channel group g taken from group g ^ 1
        res = u.reshape(u.shape[:2] + (C // 8, 2, 4))[:, :, :, ::-1].reshape(u.shape)
    s = elu(res + (prod(hid, w["w2"], not bf16) + b2.astype(dt)))
    E_s = Eu + E_h @ A(w["w2"]).T + TOL * (A(hid) @ A(w["w2"]).T + A(w["b2"]) + A(u)) + FLOOR
    if not final:
        return s, E_s
    front = None
    if defect == "pad_rows_not_zeroed":                           # the two rows before the utterance computed like any row (u = 0 there) instead of zeros
        front = np.broadcast_to(elu64(w["b2"].astype(F64) + w["w2"].astype(F64) @ elu64(w["b1"].astype(F64))), (2, C))
    sw = win(s, 3, front)
    pcm = prod(sw, w["wf"][None, :], True)[..., 0] + bf.astype(dt)[0]
    E_p = win(E_s, 3) @ A(w["wf"]) + TOL * (A(sw) @ A(w["wf"]) + abs(float(w["bf"][0]))) + FLOOR
    return pcm, E_p


def model(c, o, emulate=False, defect=None):
    """(out, bound) of case c over all L rows: out [B][L][C] (plain) or [B][L] (final)"""
    w = weights(c, o)
    u, Eu = stage0(c, o, w, emulate, defect)
    if defect in ("halo_short", "stale_utterance"):
        return tile_defect(c, w, u, Eu, defect)
    return block(c, w, u, Eu, emulate, defect)


def tile_defect(c, w, u, Eu, defect):
    """faults of the tiling, applied to the f64 reference tile by tile (tile k of an utterance produces rows [t0 + k T, t0 + (k + 1) T)):
    halo_short: a tile sees one row of history less than it needs (HALO - 1 rows before its first new row; zeros before that);
    stale_utterance: a persistent block keeps the utterance index of its previous tile (tile + G handled with utterance tile / tiles): it recomputes rows of
    that utterance and never produces those of the right one."""
    C, final, bf16, pers, fused, T = FORMS[c["form"]]
    halo = 4 if final else 2
    good, bound = block(c, w, u, Eu)
    out = good.copy()
    tiles = (c["t1"] - c["t0"] + T - 1) // T
    if defect == "halo_short":
        for k in range(1, tiles):
            tb = c["t0"] + k * T
            cut = u.copy()
            cut[:, :tb - (halo - 1)] = 0.0
            out[:, tb:tb + T] = block(c, w, cut, Eu)[0][:, tb:tb + T]
        return out, bound
    G = c["grid"]
    out[:] = np.nan
    for g in range(G):
        prev = None
        for tile in range(g, B * tiles, G):
            bi = (tile if prev is None else prev) // tiles
            tb = c["t0"] + (tile % tiles) * T
            out[bi, tb:min(tb + T, c["t1"])] = good[bi, tb:min(tb + T, c["t1"])]
            prev = tile
    return out, bound


def row_image(pcm_b, lim, s16, c, nbytes, defect=None):
    """utterance's row destination as bytes: samples [t0, min(lim, L, t1)) as f32 or int16, 0xff everywhere else"""
    n = min(lim & ~3 if defect == "lim_floor4" else lim, c["L"], c["t1"])
    img = np.full(nbytes, 0xFF, np.uint8)
    if n > c["t0"]:
        v = np.ascontiguousarray(pcm16(pcm_b[c["t0"]:n]) if s16 else np.asarray(pcm_b[c["t0"]:n], F32)).view(np.uint8)
        sz = 2 if s16 else 4
        img[c["t0"] * sz:c["t0"] * sz + v.size] = v
    return img


_REF = {}


def reference(c):
    """operands and f64 model of a case, computed once and shared (keyed by everything the values depend on)"""
    k = (data_id(c), FORMS[c["form"]][:3], c["nob"])
    if k not in _REF:
        o = operands(c)
        _REF[k] = (o,) + model(c, o)
    return _REF[k]


# ------------------------------------------------------------------------------------------------ no GPU: the bound has room for the kernel, and none for its faults
@pytest.mark.parametrize("form", list(FORMS))
def test_emulation_stays_within_half_the_bound(form):
    """The kernels' arithmetic, emulated in numpy (round-to-nearest-even hi / lo split of the activations, the weights' hi plane plus -- f32 weights and the
    final convolution -- the lo plane against the activations' hi plane only, f32 accumulation per 32-deep matrix step in the kernels' k order, ELU as
    exp - 1 in f32), stays within HALF the bound the GPU tests use, for every case of this file."""
    worst, seen = 0.0, set()
    for c in ALL_CASES:
        k = (data_id(c), c["nob"])
        if c["form"] != form or k in seen:
            continue
        seen.add(k)
        o, want, bound = reference(c)
        got = model(c, o, emulate=True)[0]
        r = float((np.abs(got.astype(F64) - want) / bound).max())
        worst = max(worst, r)
        assert np.isfinite(got).all() and r <= 0.5, (cid(c), r)
    print(f"{form}: emulated error / bound, worst {worst:.3f}")


def _named(form, L=None, **kw):
    """a case of the tables above (so that the GPU tests run it): full range, all biases, the given form, length (default: three tiles) and fields"""
    L = three_tiles(form) if L is None else L
    return next(c for c in ALL_CASES if c["form"] == form and c["L"] == L and not c["nob"] and (c["t0"], c["t1"]) == (0, L) and c["wfs"] == WFS and
                all(c[k] == v for k, v in kw.items()))


# defect -> the named cases that must catch it
DEFECT_CASES = {
    # both T of each width: 126 / 124 at 64 channels, 62 / 94 / 60 at 128; and the fused kernel
    "halo_short": [_named(f) for f in ("c64-plain-bf16-tile", "c64-final-bf16-tile", "c128-plain-bf16-tile", "c128-plain-bf16-pers", "c128-final-bf16-tile",
                                       "c64-final-bf16-pers", "up-final-bf16-pers")],
    "taps_reversed": [_named(f) for f in ("c64-plain-f32-tile", "c128-final-bf16-tile", "up-final-bf16-pers")],
    "no_b1": [_named(f) for f in FORMS], "no_b2": [_named(f) for f in FORMS], "no_bf": [_named(f) for f in FORMS if FORMS[f][1]],
    # (the samples of the 128-wide final forms and of the fused kernel stay at 0.3 - 1.9 of the bound without the lo plane, depending on the draw: three to
    # four stages of absolute sums stand against one stage's rounding.  Their stages B and C are the plain forms' code, instantiated)
    "no_lo": [_named(f) for f in FORMS if not FORMS[f][1]] + [_named(f) for f in ("c64-final-bf16-tile", "c64-final-f32-tile", "c64-final-bf16-pers")],
    "pad_rows_not_zeroed": [_named(f, L) for f in FORMS if FORMS[f][1] for L in lengths(f)[:2]],
    "residual_neighbour": [_named(f) for f in ("c64-plain-bf16-tile", "c128-plain-f32-tile", "c64-final-bf16-pers", "up-final-bf16-pers")],
    "stale_utterance": [_named(f, grid=2) for f in PERS_FORMS],
}


@pytest.mark.parametrize("defect", list(DEFECT_CASES))
def test_planted_defects_are_caught(defect):
    """Each fault a tile kernel can have, applied to the f64 reference, exceeds the bound against the true reference on EVERY case named for it (all of them
    cases the GPU tests run): a halo one row short at the tile seams, the taps reversed, a bias dropped, the activations' lo plane dropped, the rows before the
    utterance not zeroed in front of the final convolution, the residual taken from the neighbouring 4-channel group, a persistent block that keeps its
    previous tile's utterance index."""
    ids = {cid(c) for c in ALL_CASES}
    for c in DEFECT_CASES[defect]:
        assert cid(c) in ids, cid(c)
        o, want, bound = reference(c)
        bad = model(c, o, defect=defect)[0]
        rows = slice(c["t0"], c["t1"])
        ratio = np.abs(bad[:, rows] - want[:, rows]) / bound[:, rows]
        worst = float(np.where(np.isfinite(ratio), ratio, np.inf).max())
        print(f"{defect} on {cid(c)}: error / bound {worst:.3g}")
        assert worst > 1.0, (defect, cid(c), worst)


def test_rows_past_the_end_cannot_reach_a_sample():
    """Not zeroing the rows at and beyond L in front of the final convolution is NOT a fault a test can see: the convolution is causal, sample t reads rows
    t - 2 .. t, so no row >= L reaches a sample < L -- whatever those rows hold.  (The rows BEFORE the utterance do: pad_rows_not_zeroed above.)"""
    c = case("c64-final-bf16-tile", 125)
    o, want, _ = reference(c)
    longer = dict(o, u=np.concatenate([o["u"], np.full((B, 3, 64), 7.0, F32)], axis=1))
    assert float(np.abs(model(dict(c, L=128, t1=128), longer)[0][:, :125] - want).max()) < 1e-12      # (f64 sums of another matrix shape: last bits)


def test_row_rule_defect_is_caught():
    """lim rounded down to a multiple of four leaves up to three samples unwritten: the expected row image differs for every lim % 4 != 0 below L, f32 and int16."""
    n = 0
    for c, i in ROWS:
        o, want, _ = reference(c)
        for b, (lim, s16) in enumerate(row_table(c["form"], c["L"], ROW_SETS[i])):
            same = np.array_equal(row_image(want[b], lim, s16, c, 4 * c["L"] + 32), row_image(want[b], lim, s16, c, 4 * c["L"] + 32, defect="lim_floor4"))
            assert same == (lim % 4 == 0 or (lim & ~3) >= min(c["L"], c["t1"]) or lim <= c["t0"]), (cid(c), lim)
            n += not same
    assert n >= 12


def test_int16_rule():
    x = np.array([0.0, 1.0, -1.0, 1.5, -7.0, np.nan, 0.99999, -0.99999, 3.0519e-5, -3.0519e-5, 0.5], F32)
    assert pcm16(x).tolist() == [0, 32767, -32767, 32767, -32767, 0, 32766, -32766, 1, -1, 16383]


def test_loader_and_hook_pack_the_same_bytes(pkg):
    """The loader's fragment-ordered copies (conv k3 and conv k1 of the three blocks, the last transposed convolution with its rows regrouped, the final
    convolution's one-column hi / lo matrix) of a checkpoint, taken from the host image of its arena, equal what the hook's entry to the same packers makes
    of the checkpoint's tensors -- f32 (hi + lo planes) and bf16 weights -- and the layout is the one resblock.hip states: lane l of k step s of 16-row tile t
    holds W[16 t + (l & 15)][32 s + 8 (l >> 4) .. + 8)."""
    rt, synth = pkg.runtime, pkg.synth
    cfg = dataclasses.replace(synth.SynthConfig.tiny(), n_filters=64)      # the tiny model with the full-size SEANet ladder (512 -> 256 -> 128 -> 64)
    t = synth.make_checkpoint(cfg, seed=7)
    conv = lambda w: np.ascontiguousarray(np.transpose(w, (0, 2, 1)).reshape(w.shape[0], -1))   # noqa: E731  [oc][ic][k] -> [oc][tap ic + c]
    mats = {}
    for j, (idx, ) in enumerate([(3,), (6,), (9,)]):
        mats[j] = (0, conv(t[f"mimi.decoder.model.{idx}.block.1.conv.weight"]))
        mats[3 + j] = (0, conv(t[f"mimi.decoder.model.{idx}.block.3.conv.weight"]))
    wt = t["mimi.decoder.model.8.convtr.weight"].astype(F32)       # [ic][oc][k = 8]: row (r, oc) = (W[.., oc, r + 4] | W[.., oc, r])
    ic, oc, _ = wt.shape
    mats[6] = (1, np.concatenate([np.transpose(wt[:, :, 4:], (2, 1, 0)).reshape(4 * oc, ic), np.transpose(wt[:, :, :4], (2, 1, 0)).reshape(4 * oc, ic)], axis=1))
    mats[7] = (2, conv(t["mimi.decoder.model.11.conv.weight"])[0])
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.safetensors")
        synth.write_safetensors(path, t)
        for mode in (rt.WEIGHTS_F32, rt.WEIGHTS_BF16):
            plan_h, _ = rt.Model.plan(path, weights=mode)
            try:
                seen = 0
                for item, (kind, rm) in mats.items():
                    got = rt.debug_plan_seanet_frags(plan_h, item)
                    if got is None:
                        assert item == 6 and mode == rt.WEIGHTS_F32          # the fused kernel's operand exists with bf16 weights only
                        continue
                    hi, lo, dims = got
                    assert dims == ((1, rm.size) if kind == 2 else rm.shape)
                    mine_hi, mine_lo = rt.debug_seanet_pack(kind, rm, want_lo=lo is not None)
                    assert np.array_equal(hi, mine_hi) and (lo is None or np.array_equal(lo, mine_lo)), (item, mode)
                    seen += 1
                assert seen == (8 if mode == rt.WEIGHTS_BF16 else 7)
            finally:
                rt.Model.plan_free(plan_h)
    # the stated layout, in numpy, on the 128 -> 64 channel block's conv k3
    rm = mats[2][1]
    hi, lo = rt.debug_seanet_pack(0, rm)
    out, inn = rm.shape
    tt, s, l, j = np.meshgrid(np.arange(out // 16), np.arange(inn // 32), np.arange(64), np.arange(8), indexing="ij")
    v = rm[16 * tt + (l & 15), 32 * s + 8 * (l >> 4) + j].reshape(-1)
    assert np.array_equal(hi, bf16_bits(v)) and np.array_equal(lo, bf16_bits(v - bf16_round(v)))
    fh, fl = rt.debug_seanet_pack(2, mats[7][1])
    col0 = fh.reshape(-1, 64, 8)[:, ::16][:, :4].reshape(-1)       # lanes 0, 16, 32, 48 hold column 0: k = 32 s + 8 (l >> 4) + j
    assert np.array_equal(col0, bf16_bits(mats[7][1])) and int(np.count_nonzero(fh)) <= mats[7][1].size


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def check(name, got, want, bound):
    """every element against its own bound.  The record holds the largest error, the bound AT THAT ELEMENT (the `scale` slot) and the worst error / bound ratio
    of the case (the `max_rel` slot)."""
    got = np.asarray(got)
    err = np.abs(got.astype(F64) - want)
    worst = float((err / bound).max())
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    record("seanet_block " + name, float(err[at]), worst, float(bound[at]), (TOL, FLOOR))
    print(f"{name}: max abs {float(err[at]):.3e} (bound there {float(bound[at]):.3e}), error / bound {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0, (name, float(err[at]), worst)


def host_rows(a, pad):
    """[B][L][C] with `pad` zero rows of history in front of every utterance"""
    return np.concatenate([np.zeros((a.shape[0], pad, a.shape[2]), F32), a], axis=1)


def run(pkg, c, o, rows=None, form=None, grid=None):
    C, final, bf16, pers, fused, T = FORMS[c["form"]]
    kw = dict(pad=c["pad"], slack=c["slack"], t0=c["t0"], t1=c["t1"], w_bf16=bool(bf16), wf=o["wf"] if final else None, b1=o["b1"], b2=o["b2"],
              bf=o["bf"] if final else None, rows=rows, form=(2 if pers else 1) if form is None else form, grid=(c["grid"] or 0) if grid is None else grid)
    if fused:
        r = pkg.runtime.debug_resblock(None, o["w1"], o["w2"], xin=host_rows(o["x"], c["x_pad"]), wup=o["wup"], bup=o["bup"], x_pad=c["x_pad"], x_slack=c["slack"], **kw)
    else:
        r = pkg.runtime.debug_resblock(host_rows(o["u"], c["pad"]), o["w1"], o["w2"], **kw)
    if kw["form"]:
        tiles = (c["t1"] - c["t0"] + T - 1) // T
        assert r["plan"] == ((6 if C == 128 else 8) if pers else (8 if C == 64 else 4), pers, c["grid"] if pers else B * tiles, tiles, T), (cid(c), r["plan"])
    return r


def check_case(pkg, c):
    """runs case c and checks the whole output buffer: rows [t0, t1) against the reference, everything else still the 0xff fill"""
    o, want, bound = reference(c)
    r = run(pkg, c, o)
    rows = slice(c["t0"], c["t1"])
    if FORMS[c["form"]][1]:
        out = r["pcm"]
        assert r["uo"] is None and out.shape == (B, c["L"])
        assert untouched(out[:, :c["t0"]]) and untouched(out[:, c["t1"]:]), cid(c) + ": samples outside [t0, t1) were written"
        check(cid(c), out[:, rows], want[:, rows], bound[:, rows])
    else:
        out = r["uo"]
        p = c["pad"]
        assert out.shape == (B, p + c["L"] + c["slack"], FORMS[c["form"]][0])
        assert untouched(out[:, :p + c["t0"]]) and untouched(out[:, p + c["t1"]:]), cid(c) + ": rows outside [t0, t1) (history, slack) were written"
        check(cid(c), out[:, p + c["t0"]:p + c["t1"]], want[:, rows], bound[:, rows])
    return out


@gpu
@pytest.mark.parametrize("c", VALUES, ids=cid)
def test_every_form_against_the_reference(pkg, c):
    """each of the eleven kernels at L = 1, 3, T - 1, T, T + 1, 2 T + 5 (the fused one at multiples of four), pad 2 and 5 (x_pad 1 and 3), NaN slack rows once,
    with all biases, with each one absent and with none."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", WALKS, ids=cid)
def test_persistent_walk(pkg, c):
    """3 utterances x 3 tiles walked by 2 blocks (5 and 4 tiles each, crossing utterance boundaries mid-walk; the prefetch clamp on the last tile), by 9 and by 1:
    within the bound, and the bits of the one-tile-per-block form of the same width (the arithmetic of a row does not depend on its tile: resblock.hip) -- for
    the fused kernel, which has no such twin, the bits of its own other grids."""
    out = check_case(pkg, c)
    o = reference(c)[0]
    if c["form"] in TILE_TWIN:
        twin = case(TILE_TWIN[c["form"]], c["L"])
        other = run(pkg, twin, o)
    else:
        twin = dict(c, grid=9 if c["grid"] != 9 else 2)
        other = run(pkg, twin, o)
    other = other["pcm"] if other["uo"] is None else other["uo"]
    assert np.array_equal(out.view(np.uint32), other.view(np.uint32)), f"{cid(c)} differs in bits from {cid(twin)}"


@gpu
@pytest.mark.parametrize("c", RANGES, ids=cid)
def test_range_mode(pkg, c):
    """rows [t0, t1) of every utterance only, t0 = 7, T, T + 1 (4, T, T + 4 with the final convolution) and t1 < L: the values of the full run's reference,
    everything outside still the fill -- uo's history and rows, pcm's samples."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("ci", ROWS, ids=lambda ci: cid(ci[0]) + "-set%d" % ci[1])
def test_row_destinations(pkg, ci):
    """lim in {0, 1, 2, 3, 4, T - 1, T, T + 1, L - 1, L, L + 7} over the utterances, f32 and int16 rows mixed in one launch, once with samples far outside
    [-1, 1] (wf scaled), once in range mode: an f32 row holds the plain pcm output of the same form bit for bit, an int16 row WritePCM16Samples' rule applied
    to those samples exactly, everything at or beyond min(lim, L, t1) (and before t0) is still fill, and pcm itself is not written."""
    c, i = ci
    o = reference(c)[0]
    table = row_table(c["form"], c["L"], ROW_SETS[i])
    plain = check_case(pkg, c)
    r = run(pkg, c, o, rows=table)
    assert untouched(r["pcm"]), cid(c) + ": pcm written beside the row destinations"
    assert (c["wfs"] == WFS and float((np.abs(plain) < 1.0).mean()) > 0.2) or float((np.abs(plain) > 1.0).mean()) > 0.5
    for b, (lim, s16) in enumerate(table):
        want = row_image(plain[b], lim, s16, c, r["rows"].shape[1])
        assert np.array_equal(r["rows"][b], want), (cid(c), b, lim, s16, int(np.flatnonzero(r["rows"][b] != want)[0]))


@gpu
@pytest.mark.parametrize("form", ["c64-plain-f32-tile", "c64-final-bf16-pers", "c128-plain-bf16-pers", "c128-final-bf16-tile", "up-final-bf16-pers"])
def test_utterances_do_not_see_each_other(pkg, form):
    """utterance 1's output keeps its bits when utterances 0 and 2 hold other data (persistent forms: blocks that cross from one utterance into the next)"""
    c = case(form, three_tiles(form))
    o = reference(c)[0]
    other = operands(dict(c, alt=1))
    key = "x" if "x" in o else "u"
    mixed = other[key].copy()
    mixed[1] = o[key][1]
    a, b = run(pkg, c, o), run(pkg, c, dict(o, **{key: mixed}))
    pick = lambda r: r["pcm"] if r["uo"] is None else r["uo"]   # noqa: E731
    assert np.array_equal(pick(a)[1].view(np.uint32), pick(b)[1].view(np.uint32)) and not np.array_equal(pick(a)[0].view(np.uint32), pick(b)[0].view(np.uint32))


@gpu
def test_refusals_before_any_launch(pkg):
    """what resblock_supported / resblock_up_supported refuse (apart from the size threshold), a form the block does not have and a persistent grid with a block
    past the last tile: PTTS_EINVAL with a message that names the reason, and nothing is launched."""
    f = pkg.runtime.debug_resblock
    z = lambda *s: np.zeros(s, F32)   # noqa: E731
    w64, w128 = dict(w1=z(32, 192), w2=z(64, 32)), dict(w1=z(64, 384), w2=z(128, 64))
    fused = dict(u=None, xin=z(3, 1 + 64, 128), wup=z(256, 256), wf=z(192), form=2, grid=2, **w64)
    bad = {
        "grid 10 outside [1, B * tiles = 9]": dict(u=z(3, 2 + 253, 64), wf=z(192), form=2, grid=10, **w64),
        "grid 0 outside": dict(u=z(3, 2 + 193, 128), form=2, grid=0, **w128),
        "grid 10 outside [1, B * tiles = 9]  ": dict(fused, grid=10),
        "t0 % 4 != 0 with row destinations": dict(u=z(3, 2 + 253, 64), wf=z(192), form=1, t0=6, rows=[(9, 0)] * 3, **w64),
        "pad < 2": dict(u=z(3, 1 + 100, 64), pad=1, form=1, **w64),
        "unsupported widths": dict(u=z(3, 2 + 100, 32), w1=z(16, 96), w2=z(32, 16), form=1),
        "x_L * 4 != L": dict(fused, L=252),
        "f32 weights with the fused form": dict(fused, w_bf16=False),
        "t0 % 4 != 0 with the fused form": dict(fused, t0=2),
        "no persistent form of this block": dict(u=z(3, 2 + 125, 128), wf=z(384), form=2, grid=2, **w128),
        "the fused form is not taken at this size": dict(fused, form=0),
    }
    for what, kw in bad.items():
        kw = dict(kw)
        with pytest.raises(pkg.PttsError) as e:
            f(kw.pop("u"), kw.pop("w1"), kw.pop("w2"), **kw)
        assert e.value.code == pkg.runtime.PTTS_EINVAL and what.strip() in str(e.value), (what, str(e.value))
    # and their neighbours are taken: the last admissible grid, the automatic choice of the unfused block (one tile per block at this size)
    assert np.isfinite(f(z(3, 2 + 253, 64), w64["w1"], w64["w2"], wf=z(192), form=2, grid=9)["pcm"]).all()
    r = f(z(3, 2 + 253, 64), w64["w1"], w64["w2"], wf=z(192), form=0)
    assert r["plan"] == (8, 0, 9, 3, 124) and np.isfinite(r["pcm"]).all()
    assert np.isfinite(f(None, w64["w1"], w64["w2"], xin=z(3, 1 + 64, 128), wup=z(256, 256), wf=z(192), form=2, grid=9)["pcm"]).all()
