"""k_flow_cluster (csrc/flow_cluster.hip) stand-alone, value by value, against f64 numpy on operands the test controls -- every launch form.

What it replaces: flowResBlock.Forward x depth (flow_net.go:116-172); one block, on a row x [512] of the residual stream:
    y   = (LN(x) ln_w + ln_b) (1 + scale) + shift          LN: biased variance over the 512 columns, the block's own eps (linear.go:295-309)
    h   = silu(y W0^T + b0)
    out = x + gate (h W2^T + b2)
The hook (ptts_debug_flow_cluster) fills FlowClusterArgs as step.cpp step_flow does and runs a SEQUENCE of launches on one granule buffer and one set of
tag words; on the device fx, the outputs and ada carry NaN slack rows, every output is 0xff before the launch and comes back whole.

Inputs (operands()), unless a case says otherwise: x ~ 1.5 N + 0.2; ln_w ~ 1 + 0.1 N, ln_b ~ 0.1 N; shift, scale, gate ~ 0.5 N per row and block; weights
~ 0.05 N rounded to bf16, biases ~ 0.2 N; every block its own draw; eps 1e-5.  ada is [rows][ldmod] with ldmod = (3 depth + 2) 512 + 4, block r's shift | scale |
gate at columns 3 r 512 and NaN in every other column.  The small-variance case: rows of standard deviation 1e-3 around an offset ~ 0.5 N, gate ~ 5e-4 N (so
that the rows stay that narrow through three blocks and eps decides LN's scale in each), eps 1e-5 / 1e-6 / 1e-3.

Reference: one block in f64 (block64).  A launch of depth d equals d launches of depth 1 bit for bit -- the residual stream is published as the f32 it is kept
in -- so values are checked per block, on the f32 input that block actually had: no bound has to be carried through several blocks.

Bound per element, u = 2^-17 (what the bf16 hi + lo split of an operand leaves), e = 2^-23, rss(a, W) = sqrt(a^2 (W^2)^T) (independent roundings add in
squares; the weights are bf16 exactly: no weight term):
    e_y = e (|y| + (|x - mu| inv_std |ln_w| + |ln_b|) (1 + |scale|))                     the roundings of LN, affine and modulation
    e_h = 1.1 (u rss(y, W0) + rss(e_y, W0) + e |pre|) + e |h|                             pre = y W0^T + b0; |silu'| <= 1.0998
    B   = |gate| (u rss(h, W2) + rss(e_h, W2) + e |h W2^T + b2|) + e (|x| + |out|)
The tolerance is KAPPA B.  KAPPA is measured, not chosen: emulate_block restates the kernel's arithmetic in numpy f32 -- the lanes' partial sums and the
wave's tree for mean and variance, 1 / sqrt in f32, the modulation in the kernel's order, the hi + lo split, one accumulator pair per K quarter over its four
32-deep matrix steps, hi + lo, the quarters in order, the f32 epilogues -- and over every case of this file its worst |error| / B against the f64 reference is
0.84 (one block 0.71, depth 0.84 -- 256 rows, more elements to find a worst one among --, small variance 0.56; the largest B is 6.0e-5, the largest
KAPPA B 4.2e-5 of max(1, max|want|)).  KAPPA = 4 x that, rounded up = 4: the factor 4 is for what the
emulation leaves out (the summation order inside a matrix instruction, rcp / rsq at 1 ulp, the device's exp, contraction into fma).
test_emulation_stays_within_a_quarter_of_the_bound holds the emulation to KAPPA B / 4 on every block of every case, and test_cases... holds KAPPA B to
1e-4 max(1, max|want|).  A worst-case L1 bound (the style of test_gpu_tall.py) is 200 times looser and would not see a biased / unbiased variance slip.

What a wrong kernel would do to these numbers is asserted on the f64 reference alone (test_mistakes_move_the_reference): the `1 +` of the modulation missing,
shift and scale swapped, the gate taken from the scale column, gate / shift / scale / ln_w / ln_b / b0 / b2 of block r +- 1, Bessel's variance, the eps of
another block -- each moves at least 25 % of a block's elements by more than 10 KAPPA B.

OBSERVED on the MI355X (profiles/flow_cluster_parity.txt, one run): largest error / B 0.76 one block (in place and out of place alike), 0.78 at depths 6 and 8,
0.56 on the narrow rows (the emulation's own figure there) -- error / (KAPPA B) <= 0.19 throughout, largest |error| 2.6e-5; bit equality with the k_skinny
launches, with the composition of depth-1 launches, across changing row counts and through the wrap held on every case.  Tried on two deliberately wrong
kernels (not committed): rk = 1 / 511 in LayerNorm fails 35 of the 37 GPU tests here (all but the wrap and the row-isolation test, which compare the kernel with
itself), the gate read from block r + 1 fails 17 (every test that launches more than one block but those two)."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round, bits, split
from _parity import record

F32 = np.float32
C = 512
E, U = 2.0 ** -23, 2.0 ** -17
KAPPA = 4.0
CEIL = 1e-4
TILE, TILES, MAX_ROWS = 12, 22, 264
FILL = np.uint32(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ cases
def case(rows, depth, kind="std"):
    return dict(rows=rows, depth=depth, kind=kind)


def cid(c):
    return f"{c['kind']}-r{c['rows']}-d{c['depth']}"


ONE_BLOCK_ROWS = (1, 11, 12, 13, 25, 64, 129, 256, 264)          # a lone row; one short of a tile, a tile, one more; three tiles; the predicate's limit
ONE_BLOCK = [case(r, 1) for r in ONE_BLOCK_ROWS]
DEPTH = [case(r, d) for d in (2, 6, 8) for r in (13, 37, 256)]  # one exchange of x, the model's depth, FC_MAX_DEPTH
REPLACED = [case(r, d) for r in (1, 13, 64) for d in (2, 6)]    # against the 2 x depth k_skinny launches
CONTINUITY = case(24, 6)
WRAP = case(13, 6)
ISOLATION = case(25, 2)
SMALL_VAR = case(13, 3, "smallvar")
CASE_BY_ID = {}
for _c in ONE_BLOCK + DEPTH + REPLACED + [CONTINUITY, WRAP, ISOLATION, SMALL_VAR]:
    CASE_BY_ID.setdefault(cid(_c), _c)          # (13 rows at depths 2 and 6 serve three tests)
ALL_CASES = list(CASE_BY_ID.values())


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def _operands(key):
    """x [alloc, 512] and per block its parameters; alloc = rows + 2 (up to the kernel's 264): the hook's operands may hold more rows than a launch takes."""
    c = CASE_BY_ID[key]
    rows, depth = c["rows"], c["depth"]
    alloc = min(rows + 2, MAX_ROWS)
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    n = lambda *s: rng.standard_normal(s)   # noqa: E731
    small = c["kind"] == "smallvar"
    x = (0.5 * n(alloc, 1) + 1e-3 * n(alloc, C)) if small else (1.5 * n(alloc, C) + 0.2)
    blocks = []
    for _ in range(depth):
        blocks.append(dict(ln_w=1.0 + 0.1 * n(C), ln_b=0.1 * n(C), shift=0.5 * n(alloc, C), scale=0.5 * n(alloc, C), gate=(5e-4 if small else 0.5) * n(alloc, C),
                           w0=bf16_round((0.05 * n(C, C)).astype(F32)), w2=bf16_round((0.05 * n(C, C)).astype(F32)), b0=0.2 * n(C), b2=0.2 * n(C)))
    blocks = [{k: np.ascontiguousarray(v, F32) for k, v in b.items()} for b in blocks]
    eps = (1e-5, 1e-6, 1e-3) if small else (1e-5,) * depth
    o = dict(x=np.ascontiguousarray(x, F32), blocks=blocks, eps=tuple(float(F32(e)) for e in eps), rows=rows, alloc=alloc, depth=depth)
    for a in [o["x"]] + [v for b in blocks for v in b.values()]:
        a.setflags(write=False)
    return o


def operands(c):
    return _operands(cid(c))


def rows_of(p, n):
    """a block's parameters for the first n rows"""
    return {k: (v[:n] if k in ("shift", "scale", "gate") else v) for k, v in p.items()}


def pack_ada(blocks, n):
    """[n][ldmod], ldmod = (3 depth + 2) 512 + 4: block r's shift | scale | gate at 3 r 512, NaN in every other column"""
    d = len(blocks)
    ada = np.full((n, (3 * d + 2) * C + 4), np.nan, F32)
    for r, p in enumerate(blocks):
        for i, k in enumerate(("shift", "scale", "gate")):
            ada[:, (3 * r + i) * C:(3 * r + i + 1) * C] = p[k][:n]
    return ada


# ------------------------------------------------------------------------------------------------ one block in f64, with the bound
def rss(a, w):
    return np.sqrt((a * a) @ (w * w).T)


def block64(x, p, eps, bound=True, one=1.0, bessel=False):
    """out [n, 512] (and B [n, 512]) of one block on the f32 rows x, in f64"""
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1, keepdims=True)
    d = x - mu
    var = (d * d).sum(axis=1, keepdims=True) / (C - 1 if bessel else C)
    inv = 1.0 / np.sqrt(var + eps)
    y = (d * inv * q["ln_w"] + q["ln_b"]) * (one + q["scale"]) + q["shift"]
    pre = y @ q["w0"].T + q["b0"]
    h = pre / (1.0 + np.exp(-pre))
    z = h @ q["w2"].T + q["b2"]
    out = x + q["gate"] * z
    if not bound:
        return out
    e_y = E * (np.abs(y) + (np.abs(d) * inv * np.abs(q["ln_w"]) + np.abs(q["ln_b"])) * (1.0 + np.abs(q["scale"])))
    e_h = 1.1 * (U * rss(y, q["w0"]) + rss(e_y, q["w0"]) + E * np.abs(pre)) + E * np.abs(h)
    B = np.abs(q["gate"]) * (U * rss(h, q["w2"]) + rss(e_h, q["w2"]) + E * np.abs(z)) + E * (np.abs(x) + np.abs(out))
    return out, B


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in numpy f32 (no GPU)
def wave_sum(v):
    """wave_sum_dpp on [n, 64]: neighbours, quads' halves, the two quads of 8 lanes, the two halves of a row of 16, then (r0 + r1) + (r2 + r3)"""
    for _ in range(4):
        v = v[:, 0::2] + v[:, 1::2]
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def emulate_product(a, w):
    """a [n, 512] f32 times the bf16 weights w [512, 512]: per K quarter an (hi, lo) accumulator pair over four matrix steps (lane group q brings
    k = 128 ss + 32 q + 8 s + (0..7) to step s), hi + lo, the quarters added in order"""
    ah, al = split(a)
    total = None
    for ss in range(4):
        acc_h, acc_l = np.zeros((a.shape[0], C), F32), np.zeros((a.shape[0], C), F32)
        for s in range(4):
            ks = np.concatenate([np.arange(ss * 128 + q * 32 + s * 8, ss * 128 + q * 32 + s * 8 + 8) for q in range(4)])
            wk = np.ascontiguousarray(w[:, ks].T)
            acc_h = acc_h + ah[:, ks] @ wk
            acc_l = acc_l + al[:, ks] @ wk
        accv = acc_h + acc_l
        total = accv if total is None else total + accv
    return total


def emulate_block(x, p, eps):
    n = x.shape[0]
    xx = np.ascontiguousarray(x, F32).reshape(n, 2, 64, 4)   # lane l holds columns 4 l .. 4 l + 3 and 256 + 4 l ..
    sx = (xx[:, 0, :, 0] + xx[:, 0, :, 1]) + (xx[:, 1, :, 0] + xx[:, 1, :, 1])
    sy = (xx[:, 0, :, 2] + xx[:, 0, :, 3]) + (xx[:, 1, :, 2] + xx[:, 1, :, 3])
    rk = F32(1.0) / F32(C)
    mean = wave_sum(sx + sy) * rk
    d = xx - mean[:, None, None, None]
    dd = d * d
    vx = (dd[:, 0, :, 0] + dd[:, 0, :, 2]) + (dd[:, 1, :, 0] + dd[:, 1, :, 2])
    vy = (dd[:, 0, :, 1] + dd[:, 0, :, 3]) + (dd[:, 1, :, 1] + dd[:, 1, :, 3])
    inv = F32(1.0) / np.sqrt(wave_sum(vx + vy) * rk + F32(eps), dtype=F32)
    o = (d * inv[:, None, None, None]).reshape(n, C)
    o = o * p["ln_w"] + p["ln_b"]
    y = o * (p["scale"] + F32(1.0)) + p["shift"]
    v = emulate_product(y, p["w0"]) + p["b0"]
    h = v / (F32(1.0) + np.exp(-v))
    out = x + p["gate"] * (emulate_product(h, p["w2"]) + p["b2"])
    assert y.dtype == F32 and h.dtype == F32 and out.dtype == F32
    return out


@functools.lru_cache(maxsize=None)
def _chain(key):
    """the case block by block on the CPU: (input f32, the emulation's output f32, the f64 block on that input, its bound) -- computed once, read-only"""
    o = _operands(key)
    n = o["rows"]
    x, steps = o["x"][:n], []
    for r in range(o["depth"]):
        p = rows_of(o["blocks"][r], n)
        out = emulate_block(x, p, o["eps"][r])
        want, B = block64(x, p, o["eps"][r])
        for a in (out, want, B):
            a.setflags(write=False)
        steps.append((x, out, want, B))
        x = out
    return steps


def chain(c):
    return _chain(cid(c))


# ------------------------------------------------------------------------------------------------ no GPU
def test_case_ids_are_unique_and_every_listed_case_is_present():
    listed = ONE_BLOCK + DEPTH + REPLACED + [CONTINUITY, WRAP, ISOLATION, SMALL_VAR]
    assert len(ALL_CASES) == len({cid(c) for c in listed}) == 9 + 9 + 6 - 2 + 1 + 0 + 1 + 1
    assert {(c["rows"], c["depth"]) for c in ONE_BLOCK} == {(r, 1) for r in (1, 11, 12, 13, 25, 64, 129, 256, 264)}
    assert {(c["rows"], c["depth"]) for c in DEPTH} == {(r, d) for r in (13, 37, 256) for d in (2, 6, 8)}
    assert {(c["rows"], c["depth"]) for c in REPLACED} == {(r, d) for r in (1, 13, 64) for d in (2, 6)}
    assert all(cid(c) in CASE_BY_ID for c in listed) and all(1 <= c["rows"] <= MAX_ROWS and 1 <= c["depth"] <= 8 for c in ALL_CASES)
    for c in ALL_CASES:
        o = operands(c)
        ada = pack_ada(o["blocks"], o["alloc"])
        assert ada.shape[1] == (3 * c["depth"] + 2) * C + 4 and ada.shape[1] % 4 == 0 and np.isnan(ada[:, 3 * c["depth"] * C:]).all() and np.isfinite(ada[:, :3 * c["depth"] * C]).all()
        for x, out, want, B in chain(c):
            assert np.isfinite(want).all() and (B > 0).all()
            assert (KAPPA * B).max() <= CEIL * max(1.0, float(np.abs(want).max())), (cid(c), float(B.max()), float(np.abs(want).max()))
    sv = operands(SMALL_VAR)
    assert len(set(sv["eps"])) == 3
    for x, out, want, B in chain(SMALL_VAR):   # the rows stay narrow: eps decides LN's scale in every block
        assert 0.5e-3 < x.astype(np.float64).std(axis=1).min() and x.astype(np.float64).std(axis=1).max() < 2e-3


def test_emulation_stays_within_a_quarter_of_the_bound():
    """KAPPA is 4 x the emulation's worst error / B over every block of every case, rounded up: the emulation stays within KAPPA B / 4."""
    worst, b_max = {}, 0.0
    for c in ALL_CASES:
        for r, (x, out, want, B) in enumerate(chain(c)):
            ratio = float((np.abs(out.astype(np.float64) - want) / B).max())
            fam = c["kind"] if c["kind"] != "std" else ("one block" if c["depth"] == 1 else "depth")
            worst[fam] = max(worst.get(fam, 0.0), ratio)
            b_max = max(b_max, float(B.max()))
            assert np.isfinite(out).all() and ratio <= KAPPA / 4.0, (cid(c), r, ratio)
    print("emulation: largest error / B", {k: round(v, 3) for k, v in worst.items()}, "largest B", b_max)
    assert KAPPA == np.ceil(4.0 * max(worst.values())), (KAPPA, worst)   # KAPPA is the measured figure, not a looser one


def _share(x, p, eps, want, B, **kw):
    return float((np.abs(block64(x, p, eps, bound=False, **kw) - want) > 10.0 * KAPPA * B).mean())


def test_mistakes_move_the_reference():
    """each mistake a kernel could make in offsets, per-block parameters or the variance moves the f64 block by more than 10 KAPPA B on >= 25 % of its elements"""
    c = CASE_BY_ID[cid(case(13, 2))]
    o, steps = operands(c), chain(c)
    low = {}

    def note(what, s):
        low[what] = min(low.get(what, 1.0), s)
    for r in (0, 1):
        x, _, want, B = steps[r]
        p, other, eps = rows_of(o["blocks"][r], 13), rows_of(o["blocks"][1 - r], 13), o["eps"][r]   # (1 - r: block r + 1 for the first, r - 1 for the second)
        note("the 1 + of the modulation missing", _share(x, p, eps, want, B, one=0.0))
        note("shift and scale swapped", _share(x, dict(p, shift=p["scale"], scale=p["shift"]), eps, want, B))
        note("gate from the scale column", _share(x, dict(p, gate=p["scale"]), eps, want, B))
        for k in ("gate", "shift", "scale", "ln_w", "ln_b", "b0", "b2"):
            note(f"{k} of block r +- 1", _share(x, dict(p, **{k: other[k]}), eps, want, B))
        note("Bessel's variance", _share(x, p, eps, want, B, bessel=True))
    o, steps = operands(SMALL_VAR), chain(SMALL_VAR)
    for r in range(3):
        x, _, want, B = steps[r]
        note("the eps of another block", _share(x, rows_of(o["blocks"][r], 13), o["eps"][(r + 1) % 3], want, B))
    print("smallest share of elements moved by more than 10 KAPPA B:", {k: round(v, 3) for k, v in low.items()})
    assert len(low) == 12 and min(low.values()) >= 0.25, low


def test_refusals_before_any_device(pkg):
    """every refusal of the hook that needs no device: PTTS_EINVAL with a message that names it, no launch in the census"""
    rt = pkg.runtime
    z = lambda *s: np.zeros(s, F32)   # noqa: E731

    def call(rows=13, depth=2, ldmod=None, **kw):
        ldmod = (3 * depth + 2) * C + 4 if ldmod is None else ldmod
        return lambda: rt.debug_flow_cluster(z(rows, C), z(rows, ldmod), z(depth, C), z(depth, C), z(depth, C, C), z(depth, C), z(depth, C, C), z(depth, C), [1e-5] * depth, **kw)
    bad = {
        "0 rows": (call(rows=0), "0 rows"),
        "265 rows": (call(rows=265), "265 rows"),
        "depth 0": (call(depth=0), "depth 0"),
        "depth 9": (call(depth=9), "depth 9"),
        "ldmod % 4": (call(ldmod=6 * C + 2), "ldmod 3074"),
        "ldmod < 3 depth 512": (call(ldmod=6 * C - 4), "ldmod 3068"),
        "ldmod > 65536": (call(ldmod=65540), "above 65536"),
        "no launch": (call(launch_rows=[]), "0 launches"),
        "9 launches": (call(launch_rows=[1] * 9), "9 launches"),
        "a launch of 0 rows": (call(launch_rows=[13, 0]), "launch 1 of 0 rows"),
        "a launch beyond the operands": (call(launch_rows=[14]), "launch 0 of 14 rows"),
        "an odd tag base": (call(tag_base0=7), "tag_base0 7 is odd"),
        "fx_back missing out of place": (call(in_place=False, null=("fx_back",)), "null operand"),
    }
    for name in ("fx", "ada", "ln_w", "ln_b", "b0", "b2", "eps", "w0", "w2", "launch_rows", "out", "state"):
        bad["null " + name] = (call(null=(name,)), "null operand")
    rt.launch_counts(True)
    try:
        for what, (f, msg) in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                f()
            assert e.value.code == rt.PTTS_EINVAL and "ptts_debug_flow_cluster" in str(e.value) and msg in str(e.value), (what, str(e.value))
            assert rt.launch_counts(True) == {}, what
    finally:
        rt.launch_counts(False)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def first_difference(a, b):
    d = np.argwhere(bits(a) != bits(b))
    return None if d.size == 0 else (tuple(int(i) for i in d[0]), float(a[tuple(d[0])]), float(b[tuple(d[0])]), int(d.shape[0]))


def launch(pkg, o, x, which=None, n=None, eps=None, **kw):
    """the hook on rows [0, n) of x and of the blocks `which` of case operands o (ada packed for exactly those blocks)"""
    which = list(range(o["depth"])) if which is None else list(which)
    n = x.shape[0] if n is None else n
    bl = [o["blocks"][r] for r in which]
    st = lambda k: np.stack([p[k] for p in bl])   # noqa: E731
    eps = [o["eps"][r] for r in which] if eps is None else eps
    r = pkg.runtime.debug_flow_cluster(x[:n], pack_ada(bl, n), st("ln_w"), st("ln_b"), st("w0"), st("b0"), st("w2"), st("b2"), eps, **kw)
    assert r["fault"] == 0, "the fault word is set on an undisturbed launch"
    return r


def expect_tags(r, launch_rows, depth, base=0):
    want = np.full(TILES, base, np.uint64)
    for n in launch_rows:
        want[:(n + TILE - 1) // TILE] += 2 * depth
    assert np.array_equal(r["tags"], (want & 0xFFFFFFFF).astype(np.uint32)), (r["tags"], want)
    assert r["launched"] == {"k_flow_cluster": len(launch_rows)}, r["launched"]


def check_values(name, got, x_in, p, eps, ref=None):
    """every element of one block's output within KAPPA B of the f64 block on the f32 input it had"""
    want, B = block64(x_in, p, eps) if ref is None else ref
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} non-finite outputs, first at {np.argwhere(~np.isfinite(got))[0]}"
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / (KAPPA * B)
    worst = float(ratio.max())
    record(name, float(err.max()), worst, float(np.abs(want).max()), (KAPPA, 0))   # (max_rel slot: error / (KAPPA B))
    print(f"{name}: max abs {float(err.max()):.3e}, error / (KAPPA B) {worst:.3f}, error / B {KAPPA * worst:.3f}")
    assert worst <= 1.0, (name, float(err.max()), worst, np.unravel_index(np.argmax(ratio), ratio.shape))


def compose(pkg, name, o, n, values=True):
    """the case as depth-1 launches, one per block, each on the previous one's f32 output; every step's values checked against the f64 block on its input"""
    x = o["x"][:n]
    for r in range(o["depth"]):
        out = launch(pkg, o, x, which=[r])["out"][0]
        if values:
            check_values(f"{name} block {r}", out, x, rows_of(o["blocks"][r], n), o["eps"][r])
        x = out
    return x


@gpu
@pytest.mark.parametrize("in_place", (True, False), ids=("inplace", "apart"))
@pytest.mark.parametrize("c", ONE_BLOCK, ids=cid)
def test_one_block_every_tile_edge(pkg, c, in_place):
    """depth 1 at 1 .. 264 rows: values; the operands hold up to two rows more than the launch takes, and those stay 0xff; out of place the input comes back
    unchanged; no fault; the launched tiles' tag words advanced by 2, the others still at the base"""
    o = operands(c)
    n, alloc = o["rows"], o["alloc"]
    base = 0 if in_place else 40
    r = launch(pkg, o, o["x"], launch_rows=[n], in_place=in_place, tag_base0=base)
    out = r["out"][0]
    assert out.shape == (alloc, C) and (bits(out[n:]) == FILL).all(), "rows at and beyond launch_rows were written"
    x, _, want, B = chain(c)[0]
    check_values(f"k_flow_cluster {cid(c)} {'in place' if in_place else 'apart'}", out[:n], x, None, None, ref=(want, B))
    if in_place:
        assert r["fx_back"] is None
    else:
        assert np.array_equal(bits(r["fx_back"][0][:n]), bits(o["x"][:n])) and (bits(r["fx_back"][0][n:]) == FILL).all(), "the input of an out-of-place launch changed"
    expect_tags(r, [n], 1, base)


@gpu
@pytest.mark.parametrize("c", DEPTH, ids=cid)
def test_depth_is_the_composition_of_single_blocks(pkg, c):
    """depths 2, 6 and 8 (FC_MAX_DEPTH): one launch equals depth launches of one block bit for bit, and each of those is within the bound on its own input"""
    o = operands(c)
    n = o["rows"]
    name = f"k_flow_cluster {cid(c)}"
    r = launch(pkg, o, o["x"], n=n)
    expect_tags(r, [n], o["depth"])
    steps = compose(pkg, name, o, n)
    assert first_difference(r["out"][0], steps) is None, (name, "one launch differs from the composition of depth-1 launches (index, launch, composition, count):", first_difference(r["out"][0], steps))


def skinny_block(rt, x, p, eps):
    """one block as the two k_skinny launches step_flow falls back to: mlp0 with LN + affine + modulation and the SiLU epilogue, mlp2 with the gated residual in place"""
    a = rt.debug_step_linear(x, p["w0"], wfmt=1, bias=p["b0"], epi=2, ln=True, ln_wb=(p["ln_w"], p["ln_b"]), eps=eps, shift=p["shift"], mscale=p["scale"])
    b = rt.debug_step_linear(a["out"], p["w2"], wfmt=1, bias=p["b2"], epi=6, gate=p["gate"], residual=x, inplace=True)
    assert a["k_skinny"] == 1 and b["k_skinny"] == 1 and a["launches"] == 1 and b["launches"] == 1
    return b["out"]


@gpu
@pytest.mark.parametrize("c", REPLACED, ids=cid)
def test_bits_of_the_launches_it_replaces(pkg, c):
    """the contract flow_cluster_recover relies on: the 2 x depth k_skinny launches compute the same bits.  Block by block on the same f32 input (so that the
    first differing block is named), then the whole chain against one launch."""
    o = operands(c)
    n = o["rows"]
    name = f"k_flow_cluster {cid(c)} vs k_skinny"
    x = o["x"][:n]
    for r in range(o["depth"]):
        p = rows_of(o["blocks"][r], n)
        sk = skinny_block(pkg.runtime, x, p, o["eps"][r])
        fc = launch(pkg, o, x, which=[r])["out"][0]
        d = first_difference(fc, sk)
        assert d is None, (name, f"block {r}: (row, column), cluster, k_skinny, differing elements:", d)
        x = sk
    full = launch(pkg, o, o["x"], n=n)["out"][0]
    assert first_difference(full, x) is None, (name, first_difference(full, x))


@gpu
def test_tags_carry_on_across_launches_of_changing_row_counts(pkg):
    """depth 6, launches of 24, 5, 13, 24 and 1 rows on one exchange state: every launch's output is a fresh-state launch's, bit for bit; the tag words are
    what the host computes (a tile advances only in the launches that reach it); the whole call twice gives the same bits"""
    o = operands(CONTINUITY)
    seq = [24, 5, 13, 24, 1]
    x = o["x"][:24]
    r = launch(pkg, o, x, launch_rows=seq)
    expect_tags(r, seq, 6)
    assert np.array_equal(r["tags"][:3], np.array([60, 36, 0], np.uint32))
    fresh = {n: launch(pkg, o, x, launch_rows=[n])["out"][0] for n in sorted(set(seq))}
    for i, n in enumerate(seq):
        assert (bits(r["out"][i][n:]) == FILL).all(), (i, n)
        assert first_difference(r["out"][i][:n], fresh[n][:n]) is None, (i, n, first_difference(r["out"][i][:n], fresh[n][:n]))
    assert first_difference(fresh[24][:24], compose(pkg, "k_flow_cluster " + cid(CONTINUITY), o, 24)) is None
    again = launch(pkg, o, x, launch_rows=seq)
    assert np.array_equal(bits(again["out"]), bits(r["out"])) and np.array_equal(again["tags"], r["tags"])


@gpu
def test_tags_wrap_through_2_to_the_32(pkg):
    """tag_base0 = 2^32 - 2 depth - 4, three launches of 13 rows at depth 6: the second one's tags pass through 0.  The row count stays, so every granule a sweep
    looks at was written by the launch before (no zero-tag granule of the cleared buffer is left to be taken for an awaited tag 0)."""
    o = operands(WRAP)
    x = o["x"][:13]
    base = 2 ** 32 - 2 * 6 - 4
    r0 = launch(pkg, o, x, launch_rows=[13] * 3)
    r1 = launch(pkg, o, x, launch_rows=[13] * 3, tag_base0=base)
    expect_tags(r0, [13] * 3, 6)
    expect_tags(r1, [13] * 3, 6, base)
    assert int(r1["tags"][0]) == 20 and int(r1["tags"][1]) == 20 and int(r1["tags"][2]) == base   # the words have wrapped
    assert first_difference(r1["out"], r0["out"]) is None, first_difference(r1["out"], r0["out"])
    for i in range(3):
        assert first_difference(r0["out"][i], r0["out"][0]) is None


@gpu
def test_rows_do_not_see_each_other(pkg):
    """a NaN in one row of fx, an Inf in another row's ada: those two rows are NaN, every other row keeps the clean run's bits -- and the clean run is finite
    although NaN sits in the slack rows behind fx and ada and in ada's pad columns"""
    o = operands(ISOLATION)
    n = 25
    clean = launch(pkg, o, o["x"], n=n)["out"][0]
    assert np.isfinite(clean).all()
    x = o["x"][:n].copy()
    x[7, 300] = np.nan
    bl = [dict(p) for p in o["blocks"]]
    sc = bl[0]["scale"].copy()
    sc[15, 41] = np.inf
    bl[0]["scale"] = sc
    dirty = launch(pkg, dict(o, blocks=bl), x, n=n)["out"][0]
    assert np.isnan(dirty[7]).all() and np.isnan(dirty[15]).all()
    keep = np.ones(n, bool)
    keep[[7, 15]] = False
    assert np.array_equal(bits(dirty[keep]), bits(clean[keep])), first_difference(dirty[keep], clean[keep])


@gpu
def test_small_variance_rows_and_every_block_its_own_eps(pkg):
    """rows of standard deviation 1e-3, eps 1e-5 / 1e-6 / 1e-3 over three blocks: each block within the bound with ITS eps, and the one launch of depth 3 is their
    composition bit for bit (a launch that took another block's eps would differ from it)"""
    o = operands(SMALL_VAR)
    name = "k_flow_cluster " + cid(SMALL_VAR)
    steps = compose(pkg, name, o, 13)
    full = launch(pkg, o, o["x"], n=13)["out"][0]
    assert first_difference(full, steps) is None, (name, first_difference(full, steps))
