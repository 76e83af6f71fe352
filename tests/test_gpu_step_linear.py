"""The AR step's linear (csrc/skinny.hip: k_skinny) stand-alone, value by value, against f64 numpy on the same operands -- every launch variant the host can pick.

What it replaces: Linear.Forward (internal/native/linear.go:117-182), optionally behind the pending residual update and LayerNorm (linear.go:265-329) with adaLN
modulation (tensor_util.go:175-193), with the epilogues of kernels.h Epi.  The hook (ptts_debug_step_linear) packs the weights with the model loader's packers,
fills every output with 0xff bytes first (a NaN where nothing is stored) and returns the buffers whole.

Launch variants (skinny.hip launch_pro / launch_nj, restated in plan() below and asserted in test_cases_reach_every_block_shape):
  NJ = 2 (K slice <= 512), 4 (<= 1024), 8 (2048-deep split slices on bf16 / int8 weights); CG = 4 (64-column blocks), 1 (16-column blocks: small grids), 2 (NJ = 8).
Every test id carries the variant it reaches ("nj4cg1"), the weight format (f32 / bf16 / i8) and, where it applies, the epilogue or prologue form.

Tolerance: the kernel's arithmetic is exact up to the bf16 hi + lo split of the activations (2^-17), the same split of f32 weights with the lo * lo term dropped
(2^-17 + 2^-18) and f32 accumulation, so |error| <= 3e-5 * (sum_k |a_k w_k| + |bias| + |R|) + 1e-6 -- the bound tests/test_gpu_tall.py uses -- times the epilogue's
Lipschitz bound (GELU 1.2, SiLU 1.1: max |silu'| = 1.0998; ELU 1; a per-column scale, gate or alpha multiplies the product's share) and, for a sum over split-K
planes, times the number of planes.  test_emulation_stays_within_half_the_bound (no GPU) runs a numpy emulation of the kernel's arithmetic -- round-to-nearest-even
hi / lo split, f32 products and sums per 32-deep matrix step and per K part in the kernel's order -- over every case of this file and holds it to HALF that bound."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round, check_bound, elu64, gelu64, silu64, untouched
from _parity import record

TOL = 3e-5
FLOOR = 1e-6
LN_TOL = (1e-4, 1e-4)   # the reference's own layer-norm tolerance (runtime/ops/tolerance.go; TOL["layer_norm"] in test_gpu_ops.py)
EPI = ["none", "gelu", "silu", "elu", "resadd", "scale_resadd", "gate_resadd", "axpy", "resadd_elu"]
WF = ["f32", "bf16", "i8"]
# the eight prologue instances of launch_w: name -> (ln, affine, modulation, pending planes)
FORMS = {"ln": (1, 0, 0, 0), "ln_affine": (1, 1, 0, 0), "ln_mod": (1, 0, 1, 0), "ln_affine_mod": (1, 1, 1, 0), "partial": (0, 0, 0, 1),
         "ln_affine_partial_one": (1, 1, 0, 1), "ln_affine_partial": (1, 1, 0, 1), "ln_affine_mod_partial": (1, 1, 1, 1)}
F32 = np.float32


# ------------------------------------------------------------------------------------------------ host arithmetic the launcher does (restated)
def kslice(K, S):
    return ((K + S - 1) // S + 127) // 128 * 128 if S > 1 else K


def plan(M, N, K, S, wfmt):
    """(NJ, CG) as launch_pro / launch_nj pick them."""
    ks = kslice(K, S)
    if ks > 1024:
        assert wfmt != 0 and ks <= 2048
        return 8, 2
    nj = 2 if ks <= 512 else 4
    b64 = ((N + 63) // 64) * ((M + 15) // 16) * S
    b16 = ((N + 15) // 16) * ((M + 15) // 16) * S
    return nj, (1 if b64 < 128 and (M <= 64 or b16 <= 256) and N > 16 else 4)


def pick_split(M, N, K, w_bf16):
    """step.cpp pick_split."""
    if K <= 1024:
        return 1
    if w_bf16 and M > 32 and K >= 4096 and K % 2048 == 0 and ((N + 31) // 32) * ((M + 15) // 16) * (K // 2048) >= 200:
        return K // 2048
    need = (K + 1023) // 1024
    blocks = ((N + 63) // 64) * ((M + 15) // 16)
    S = max(need, min((256 + blocks - 1) // blocks, K // 512))
    while S > need and (S - 1) * kslice(K, S) >= K:
        S -= 1
    return S


def test_pick_split_never_leaves_an_empty_slice():
    """skinny_supported refuses a split whose last slice starts at or beyond K (K = 1104 over 4: slice 3 would start at 1152).  pick_split's first form could
    produce one at widths that are no multiple of 512 -- K = 3080 with a small grid gave 6 slices of 640: 5 x 640 >= 3080 -- and now steps back to fewer slices;
    for every K % 8 == 0 up to 8192 and grids from one block to a full chip the slices are non-empty and no deeper than the kernel takes."""
    for w_bf16 in (False, True):
        for M in (1, 16, 33, 64, 256):
            for N in (32, 64, 512, 1024, 4096):
                for K in range(8, 8193, 8):
                    S = pick_split(M, N, K, w_bf16)
                    ks = kslice(K, S)
                    assert S >= 1 and (S - 1) * ks < K, (M, N, K, S)
                    assert ks <= (2048 if (w_bf16 and S > 1) else 1024), (M, N, K, S)
    assert pick_split(16, 64, 3080, False) == 5 and pick_split(64, 1024, 4096, False) == 4 and pick_split(64, 1024, 4096, True) == 2


# ------------------------------------------------------------------------------------------------ number formats
def quantize_rows(w):
    """model.cpp quantize_rows in f32: s = max|row| / 127 (1 for a zero row), q = rint(W / s) clamped to +-127, W^ = q s."""
    w = np.ascontiguousarray(w, F32)
    mx = np.abs(w).max(axis=1)
    s = np.where(mx > 0, mx / F32(127.0), F32(1.0)).astype(F32)
    q = np.clip(np.rint(w / s[:, None]), -127.0, 127.0).astype(F32)
    return q * s[:, None], q, s


# ------------------------------------------------------------------------------------------------ cases
def case(M, N, K, wfmt=0, epi=0, S=1, **kw):
    c = dict(M=M, N=N, K=K, wfmt=wfmt, epi=epi, S=S, bias=True, lda=K + 8, ldc=N + 4, form=None, psplit=0, pbias=False, tail=False, addvec=False, R=None,
             inplace=False, zrows=0, path=0)
    c.update(kw)
    if c["R"] is None:
        c["R"] = epi >= 4
    if c["form"]:
        c["lda"] = K   # the fused prologue needs dense rows
    return c


def cid(c):
    nj, cg = plan(c["M"], c["N"], c["K"], c["S"], c["wfmt"])
    s = f"{c['M']}x{c['N']}x{c['K']}-{WF[c['wfmt']]}-nj{nj}cg{cg}"
    if c["form"]:
        s += f"-{c['form']}" + (f"-p{c['psplit']}" + ("b" if c["pbias"] else "") if c["psplit"] else "")
    if c["S"] > 1:
        s += f"-split{c['S']}" + ("R" if c["R"] else "") + (f"-z{c['zrows']}" if c["zrows"] else "")
    if c["epi"] or c["tail"]:
        s += f"-{EPI[c['epi']]}" + ("-tail" if c["tail"] else "") + ("-inplace" if c["inplace"] else "")
    return s + ("-gemm" if c["path"] else "")


# plain product: the row-tile edges 1, 4, 5 (the p_m - m0 > 4 barrier), 15, 16, 17, 64, 65, 250, 256; the column-tile edges 16, 17 (the N > 16 narrow-block
# condition), 37, 63, 64, 65, 1040; the depths 8, 24, 120, 128, 136, 512, 520, 1000, 1024; lda > K and ldc > N throughout.  Which shape reaches which block:
#   (NJ 2, CG 4): 1x16x8 (N = 16 keeps 64-column blocks), 256x1040x512 (272 blocks)      (NJ 2, CG 1): 4x17x24 ... 17x65x512, 250x37x8, 256x64x512
#   (NJ 4, CG 1): 64x1040x520, 64x65x1000, 256x17x1024                                   (NJ 4, CG 4): 65x1040x1000 (325 narrow blocks), 250x1040x1024, 16x16x1024
#   (NJ 8, CG 2): 2048-deep split slices only -- SPLIT below
PLAIN_SHAPES = [(1, 16, 8), (4, 17, 24), (5, 37, 120), (15, 63, 128), (16, 64, 136), (17, 65, 512), (64, 1040, 520), (64, 65, 1000), (65, 1040, 1000),
                (250, 1040, 1024), (256, 17, 1024), (16, 16, 1024), (250, 37, 8), (256, 64, 512), (256, 1040, 512)]
PLAIN = [case(m, n, k, wfmt=w) for (m, n, k) in PLAIN_SHAPES for w in (0, 1, 2)]
# every epilogue at a ragged shape (37 x 70 x 520: NJ 4, CG 1; the residual in place) and at 250 x 1040 x 1024 (NJ 4, CG 4; the residual apart from C)
EPIS = [case(37, 70, 520, wfmt=e % 3, epi=e, inplace=e >= 4, addvec=e == 2) for e in range(9)] + \
       [case(250, 1040, 1024, wfmt=(e + 1) % 3, epi=e, addvec=e == 2) for e in range(9)] + \
       [case(37, 70, 520, wfmt=1, epi=6), case(250, 1040, 1024, wfmt=0, epi=6, inplace=True)]
TAILS = [case(37, 70, 520, wfmt=1, epi=2, tail=True, addvec=True), case(17, 65, 512, wfmt=0, epi=1, tail=True), case(250, 33, 1024, wfmt=2, epi=2, tail=True, addvec=True)]
# split-K: 4096 deep in 4 and 8 planes on f32, in 2 planes of 2048 on bf16 and int8 (NJ 8, CG 2); a ragged, non-empty last slice (3000 = 1024 + 1024 + 952);
# zrows: the planes of a row chunk of a taller operand (GemmArgs::zstride)
SPLIT = [case(16, 1040, 4096, wfmt=0, S=4, R=True), case(100, 200, 4096, wfmt=0, S=8), case(256, 200, 4096, wfmt=1, S=2, R=True), case(100, 70, 4096, wfmt=2, S=2, R=True),
         case(16, 200, 3000, wfmt=0, S=3, R=True), case(100, 64, 3000, wfmt=1, S=3, zrows=128), case(256, 37, 4096, wfmt=2, S=4, R=True, zrows=300),
         case(100, 70, 4096, wfmt=1, S=4)]


def _fused_cases():
    out, i, j = [], 0, 0
    ps, pb = [2, 3, 4, 5, 2, 3, 4, 5, 3], [True, False, True, False, False, True, False, True, True]
    for form in FORMS:
        for K in (512, 1024, (520, 1000)[i % 2]):
            M, N = (1, 17, 250)[i % 3], (70, 200, 1040)[(i // 3) % 3]
            c = case(M, N, K, wfmt=i % 3, form=form, epi=(0, 2, 6, 0)[i % 4], addvec=i % 4 == 1)
            if FORMS[form][3]:
                if form.endswith("_one"):
                    c.update(psplit=1, pbias=bool(i % 2))
                else:
                    c.update(psplit=ps[j], pbias=pb[j])
                    j += 1
            out.append(c)
            i += 1
    return out


FUSED = _fused_cases()
DISPATCH = [case(m, 70, 520, wfmt=1, epi=6, path=1) for m in (1, 64, 65, 130, 256)]
GROUPS = {"plain": PLAIN, "epilogues": EPIS, "tail": TAILS, "split": SPLIT, "fused": FUSED, "dispatch": DISPATCH}


def test_cases_reach_every_block_shape():
    got = {plan(c["M"], c["N"], c["K"], c["S"], c["wfmt"]) for c in PLAIN + SPLIT}
    assert got >= {(2, 1), (2, 4), (4, 1), (4, 4), (8, 2)}
    for c in PLAIN[::3]:
        assert plan(c["M"], c["N"], c["K"], 1, 0) == plan(c["M"], c["N"], c["K"], 1, 1)   # the block shape does not depend on the weight format
    assert {c["form"] for c in FUSED} == set(FORMS) and {c["epi"] for c in EPIS} == set(range(9))
    assert {(c["psplit"], c["pbias"]) for c in FUSED if c["psplit"] > 1} == {(p, b) for p in (2, 3, 4, 5) for b in (False, True)}
    assert {c["M"] for c in FUSED} == {1, 17, 250} and all(len({cid(c) for c in g}) == len(g) for g in GROUPS.values())


def operands(c):
    rng = np.random.default_rng(zlib.crc32(cid(c).encode()))
    M, N, K = c["M"], c["N"], c["K"]
    o = {"x": rng.standard_normal((M, c["lda"]), dtype=F32), "W": (0.05 * rng.standard_normal((N, K))).astype(F32)}
    if c["wfmt"] == 1:
        o["Weff"] = bf16_round(o["W"])
    elif c["wfmt"] == 2:
        o["Weff"], o["q"], o["ws"] = quantize_rows(o["W"])
    else:
        o["Weff"] = o["W"]
    o["bias"] = rng.standard_normal(N).astype(F32) if c["bias"] else None
    o["addvec"] = rng.standard_normal(N - 1 if c["tail"] else N).astype(F32) if c["addvec"] else None
    o["R"] = rng.standard_normal((M, c["ldc"]), dtype=F32) if c["R"] else None
    o["scale"] = rng.standard_normal(N).astype(F32) if c["epi"] == 5 else None
    o["gate"] = rng.standard_normal((M, N + 5), dtype=F32) if c["epi"] == 6 else None
    o["alpha"] = 0.7 if c["epi"] == 7 else 1.0
    if c["form"]:
        ln, aff, mod, part = FORMS[c["form"]]
        o["ln_wb"] = ((1.0 + 0.1 * rng.standard_normal(K)).astype(F32), (0.1 * rng.standard_normal(K)).astype(F32)) if aff else None
        o["shift"] = (0.3 * rng.standard_normal((M, K + 12))).astype(F32) if mod else None
        o["mscale"] = (0.3 * rng.standard_normal((M, K + 12))).astype(F32) if mod else None
        o["planes"] = (0.3 * rng.standard_normal((c["psplit"], M, K))).astype(F32) if part else None
        o["pbias"] = (0.1 * rng.standard_normal(K)).astype(F32) if c["pbias"] else None
    return o


# ------------------------------------------------------------------------------------------------ the operation, in f64 and as the kernel's arithmetic
def updated_rows(c, o):
    """x + (((p0 + p1) + ...) + pbias) in f32, in the kernel's order."""
    x = o["x"][:, :c["K"]]
    if not (c["form"] and FORMS[c["form"]][3]):
        return np.ascontiguousarray(x)
    ps = o["planes"][0].copy()
    for z in range(1, c["psplit"]):
        ps = ps + o["planes"][z]
    if o["pbias"] is not None:
        ps = ps + o["pbias"]
    return x + ps


def normed_rows(c, o, xs, dt):
    if not (c["form"] and FORMS[c["form"]][0]):
        return xs.astype(dt)
    K = c["K"]
    x = xs.astype(dt)
    if dt == F32:   # the kernel: sums in f32, 1 / K and 1 / sqrt by the approximate instructions (1 ulp)
        rk = F32(1.0) / F32(K)
        mean = x.sum(axis=1, keepdims=True, dtype=F32) * rk
        var = ((x - mean) ** 2).sum(axis=1, keepdims=True, dtype=F32) * rk
        y = (x - mean) * (F32(1.0) / np.sqrt(var + F32(1e-5), dtype=F32))
    else:
        mean = x.mean(axis=1, keepdims=True)
        y = (x - mean) / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + 1e-5)      # biased, linear.go:295-309
    if o["ln_wb"] is not None:
        y = y * o["ln_wb"][0].astype(dt) + o["ln_wb"][1].astype(dt)
    if o["mscale"] is not None:
        y = y * (o["mscale"][:, :K].astype(dt) + dt(1.0)) + o["shift"][:, :K].astype(dt)
    return y


def emulated_sums(c, o, y, k0, k1):
    """The f32 sums of K slice [k0, k1) as k_skinny forms them: activations as bf16 hi + lo, f32 weights as hi + lo with lo * lo dropped (int8: the integers, the row
    scale afterwards), one f32 accumulator pair per K part over its 32-deep matrix steps (lane group q brings k = 128 ss + 32 q + 8 s + (0..7) to step s), hi + lo,
    then the K parts in order."""
    cg = plan(c["M"], c["N"], c["K"], c["S"], c["wfmt"])[1]
    kp = 16 // cg
    klen = k1 - k0
    nss = (klen + 127) // 128
    ssq = (nss + kp - 1) // kp
    ys = np.ascontiguousarray(y[:, k0:k1], F32)
    xh = bf16_round(ys)
    xl = bf16_round(ys - xh)
    w = np.ascontiguousarray((o["q"] if c["wfmt"] == 2 else o["Weff"])[:, k0:k1], F32)
    wh = bf16_round(w)
    wl = bf16_round(w - wh) if c["wfmt"] == 0 else None
    total = None
    for p in range(kp):
        ah = np.zeros((c["M"], c["N"]), F32)
        al = np.zeros((c["M"], c["N"]), F32)
        for ss in range(p * ssq, min(nss, (p + 1) * ssq)):
            for s in range(4):
                ks = np.concatenate([np.arange(ss * 128 + q * 32 + s * 8, ss * 128 + q * 32 + s * 8 + 8) for q in range(4)])
                ks = ks[ks < klen]
                if ks.size == 0:
                    continue
                ah = ah + xh[:, ks] @ wh[:, ks].T
                al = al + xl[:, ks] @ wh[:, ks].T
                if wl is not None:
                    al = al + xh[:, ks] @ wl[:, ks].T
        accv = ah + al
        total = accv if total is None else total + accv
    return total * o["ws"][None, :] if c["wfmt"] == 2 else total


def model(c, o, emulate=False):
    """The operation of case c: f64 numpy (with the bound of every output), or -- emulate -- the kernel's arithmetic in f32."""
    dt = F32 if emulate else np.float64
    M, N, K, S = c["M"], c["N"], c["K"], c["S"]
    xs = updated_rows(c, o)
    y = normed_rows(c, o, xs, dt)
    W = o["Weff"].astype(np.float64)
    bias = (o["bias"] if o["bias"] is not None else np.zeros(N, F32)).astype(dt)
    R = o["R"][:, :N].astype(dt) if o["R"] is not None else None
    res = {"xs": xs, "y": y}
    ks = kslice(K, S)
    sums, ab = [], []
    for z in range(S):
        k0, k1 = z * ks, min(K, (z + 1) * ks)
        sums.append(emulated_sums(c, o, y, k0, k1) if emulate else y[:, k0:k1] @ W[:, k0:k1].T)
        ab.append(np.abs(y[:, k0:k1].astype(np.float64)) @ np.abs(W[:, k0:k1]).T)
    if S > 1:   # plane 0 = R + (sums_0 + bias) when R is given, raw sums otherwise
        planes, bounds = [], []
        for z in range(S):
            if z == 0 and R is not None:
                planes.append(R + (sums[0] + bias))
                bounds.append(TOL * (ab[0] + np.abs(bias) + np.abs(R)) + FLOOR)
            else:
                planes.append(sums[z])
                bounds.append(TOL * ab[z] + FLOOR)
        res["planes"], res["plane_bounds"] = planes, bounds
        res["out"] = np.sum(np.stack([p.astype(np.float64) for p in planes]), axis=0)
        res["bound"] = S * TOL * (sum(ab) + (np.abs(bias) + np.abs(R) if R is not None else 0.0)) + FLOOR
        return res
    pre = sums[0] + bias
    b0 = TOL * (ab[0] + np.abs(bias))
    absR = np.abs(R) if R is not None else 0.0
    e = c["epi"]
    p64 = pre.astype(np.float64)
    if e == 0:
        out, bound = pre, b0
    elif e == 1:
        out, bound = gelu64(p64), 1.2 * b0                                   # |gelu'| <= 1.13
    elif e == 2:
        av = np.zeros(N, dt)
        av[:o["addvec"].size] = o["addvec"]
        out, bound = silu64((av + pre).astype(np.float64)), 1.1 * (b0 + TOL * np.abs(av))   # |silu'| <= 1.0998
    elif e == 3:
        out, bound = elu64(p64), b0
    elif e == 4:
        out, bound = R + pre, b0 + TOL * absR
    elif e == 5:
        out, bound = R + o["scale"].astype(dt) * pre, np.abs(o["scale"]) * b0 + TOL * absR
    elif e == 6:
        g = o["gate"][:, :N].astype(dt)
        out, bound = R + g * pre, np.abs(g) * b0 + TOL * absR
    elif e == 7:
        out, bound = R + dt(o["alpha"]) * pre, abs(o["alpha"]) * b0 + TOL * absR
    else:
        out, bound = elu64((R + pre).astype(np.float64)), b0 + TOL * absR
    res["out"], res["bound"] = np.asarray(out, np.float64), np.asarray(bound, np.float64) + FLOOR
    if c["tail"]:   # the last column leaves as acc + bias, without the epilogue
        res["tail"], res["tail_bound"] = p64[:, N - 1], b0[:, N - 1] + FLOOR
    return res


_REF = {}


def reference(c):
    """operands and f64 model of a case, computed once and shared."""
    k = cid(c)
    if k not in _REF:
        o = operands(c)
        _REF[k] = (o, model(c, o))
    return _REF[k]


# ------------------------------------------------------------------------------------------------ the emulation against the bound: no GPU
@pytest.mark.parametrize("group", list(GROUPS))
def test_emulation_stays_within_half_the_bound(group):
    """The kernel's arithmetic, emulated in numpy, stays within HALF the bound the GPU tests use, for every case of this file: the bound has room for the kernel."""
    worst = 0.0
    for c in GROUPS[group]:
        o = operands(c)
        ref, emu = model(c, o), model(c, o, emulate=True)
        pairs = [(emu["out"], ref["out"], ref["bound"])]
        if c["S"] > 1:
            pairs += list(zip(emu["planes"], ref["planes"], ref["plane_bounds"]))
        if c["tail"]:
            pairs = [(emu["out"][:, :-1], ref["out"][:, :-1], ref["bound"][:, :-1]), (emu["tail"], ref["tail"], ref["tail_bound"])]
        for got, want, bound in pairs:
            r = float((np.abs(np.asarray(got, np.float64) - want) / bound).max())
            worst = max(worst, r)
            assert r <= 0.5, (cid(c), r)
        if c["form"] and FORMS[c["form"]][0]:
            assert np.allclose(emu["y"], ref["y"], atol=LN_TOL[0] / 2, rtol=LN_TOL[1] / 2), cid(c)
    print(f"{group}: emulated error / bound, worst {worst:.3f}")


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
def check(name, got, want, bound):
    check_bound(name, got, want, bound, TOL)


def run(pkg, c, o, **over):
    kw = dict(wfmt=c["wfmt"], bias=o["bias"], addvec=o["addvec"], residual=o["R"], inplace=c["inplace"], scale=o["scale"], gate=o["gate"], alpha=o["alpha"],
              epi=c["epi"], tail=c["tail"], ldc=c["ldc"], splitk=c["S"], zrows=c["zrows"], path=c["path"])
    if c["form"]:
        kw.update(ln=bool(FORMS[c["form"]][0]), ln_wb=o["ln_wb"], shift=o["shift"], mscale=o["mscale"], planes=o["planes"], pbias=o["pbias"])
    kw.update(over)
    x = kw.pop("x", o["x"])
    r = pkg.runtime.debug_step_linear(x, o["W"], **kw)
    if c["wfmt"] == 2:   # the reference's weights ARE the kernel's: W^ = q s by the loader's quantiser
        assert np.array_equal(r["w_eff"], o["Weff"]) and np.array_equal(r["w_scale"], o["ws"])
    return r


def check_case(pkg, c):
    """runs case c and checks every output: values, the padding columns N..ldc, the prologue's rows."""
    o, ref = reference(c)
    r = run(pkg, c, o)
    name, M, N = "k_skinny " + cid(c), c["M"], c["N"]
    assert r["k_skinny"] >= 1 and r["launches"] == r["k_skinny"], (name, r["k_skinny"], r["launches"])
    out = r["out"]
    if c["S"] > 1:
        assert out.shape == (c["S"], c["zrows"] or M, N)
        assert untouched(out[:, M:, :]), name + ": rows beyond M of a plane were written"
        for z in range(c["S"]):
            check(f"{name} plane {z}", out[z, :M], ref["planes"][z], ref["plane_bounds"][z])
        check(f"{name} sum", out[:, :M].astype(np.float64).sum(axis=0), ref["out"], ref["bound"])
        return r
    pad = out[:, N:]
    if c["inplace"]:
        assert np.array_equal(pad.view(np.uint32), o["R"][:, N:].view(np.uint32)), name + ": padding columns of the in-place residual changed"
    else:
        assert untouched(pad), name + ": padding columns N..ldc were written"
    if c["tail"]:
        assert untouched(out[:, N - 1]), name + ": C's last column was written beside the tail"
        check(name + " tail", r["tail"], ref["tail"], ref["tail_bound"])
        check(name, out[:, :N - 1], ref["out"][:, :N - 1], ref["bound"][:, :N - 1])
    else:
        check(name, out[:, :N], ref["out"], ref["bound"])
    if c["form"]:
        ln, _, _, part = FORMS[c["form"]]
        if part:
            assert np.array_equal(r["x_out"].view(np.uint32), ref["xs"].view(np.uint32)), name + ": x_out is not x + (((p0 + p1) + ...) + pbias) bit for bit"
        else:
            assert untouched(r["x_out"])
        if ln:
            err = np.abs(r["y_out"].astype(np.float64) - ref["y"])
            record(name + " y_out", float(err.max()), 0.0, float(np.abs(ref["y"]).max()), LN_TOL)
            assert np.isfinite(r["y_out"]).all() and (err <= LN_TOL[0] + LN_TOL[1] * np.abs(ref["y"])).all(), (name, float(err.max()))
        else:
            assert untouched(r["y_out"])
    return r


@gpu
@pytest.mark.parametrize("c", PLAIN, ids=cid)
def test_plain_product(pkg, c):
    """bias only, all three weight formats, every block shape at the tile edges (PLAIN_SHAPES above says which shape reaches which)."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", EPIS, ids=cid)
def test_every_epilogue(pkg, c):
    """EPI_NONE .. EPI_RESADD_ELU with a gate of ldg > N, alpha = 0.7, the residual in place (R == C) and apart."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", TAILS, ids=cid)
def test_tail_column(pkg, c):
    """the last column arrives in tail[m] as acc + bias without the epilogue, C's last column keeps the fill, addvec has N - 1 entries."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", SPLIT, ids=cid)
def test_split_k_planes(pkg, c):
    """each plane on its own (plane 0 = R + (sums_0 + bias) with R, raw sums otherwise), then the sum; NJ 8 / CG 2 is the 2048-deep bf16 and int8 form."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", FUSED, ids=cid)
def test_fused_prologue(pkg, c):
    """each prologue instance at K = 512, 1024 and 520 / 1000 (1 / K no longer exact), 1 / 17 / 250 rows, 1 to 5 planes with and without pbias, ldmod > K:
    x_out bit for bit, y_out to the layer-norm tolerance, the product to the operand-split bound against the f64 LayerNorm."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("form", [None, "ln_affine"])
def test_rows_do_not_see_each_other(pkg, form):
    """250 copies of one row give 250 copies of one output row, bit for bit; one NaN in one row gives NaN in that output row only."""
    c = case(250, 70, 520 if form is None else 1000, wfmt=1, epi=6, form=form)
    o = dict(reference(c)[0])
    x = np.repeat(o["x"][:1], 250, axis=0)
    same = dict(o, x=x, R=np.repeat(o["R"][:1], 250, axis=0), gate=np.repeat(o["gate"][:1], 250, axis=0))
    r = run(pkg, c, same)
    bits = r["out"][:, :70].view(np.uint32)
    assert np.isfinite(r["out"][:, :70]).all() and (bits == bits[0]).all()
    if form:
        assert (r["y_out"].view(np.uint32) == r["y_out"].view(np.uint32)[0]).all()
    clean = run(pkg, c, o)["out"][:, :70]
    xn = o["x"].copy()
    xn[37, 333] = np.nan
    dirty = run(pkg, c, o, x=xn)["out"][:, :70]
    assert np.isnan(dirty[37]).all()
    keep = np.arange(250) != 37
    assert np.array_equal(dirty[keep].view(np.uint32), clean[keep].view(np.uint32))


@gpu
@pytest.mark.parametrize("c", DISPATCH, ids=cid)
def test_launch_gemm_hands_over_to_the_step_kernel(pkg, c):
    """launch_gemm with a tiled weight copy: k_skinny is what runs (one launch up to 64 rows, 64-row chunks up to 256), with path 0's bits up to 64 rows."""
    r = check_case(pkg, c)
    assert r["k_skinny"] == (c["M"] + 63) // 64 and r["launches"] == r["k_skinny"]
    if c["M"] <= 64:
        direct = run(pkg, c, reference(c)[0], path=0)
        assert np.array_equal(direct["out"].view(np.uint32), r["out"].view(np.uint32))


@gpu
def test_int8_quantiser_is_the_stated_rule(pkg):
    """W^ and the scales the hook returns (the loader's quantize_rows) against the rule in numpy, with a zero row and a row whose maximum is negative."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((20, 24)).astype(F32)
    w[3] = 0.0
    w[7] = -np.abs(w[7])
    w[7, 5] = -9.0
    weff, q, s = quantize_rows(w)
    assert s[3] == 1.0 and (weff[3] == 0).all() and q[7, 5] == -127.0 and s[7] == F32(9.0) / F32(127.0)
    r = pkg.runtime.debug_step_linear(np.ones((1, 24), F32), w, wfmt=2)
    assert np.array_equal(r["w_scale"], s) and np.array_equal(r["w_eff"], weff)
    want = weff.astype(np.float64).sum(axis=1)[None, :]
    check("k_skinny int8 quantiser rows", r["out"], want, TOL * np.abs(weff.astype(np.float64)).sum(axis=1)[None, :] + FLOOR)


@gpu
def test_refusals_before_any_launch(pkg):
    """what skinny_supported / skinny_fuse_supported refuse, the hook answers with PTTS_EINVAL and launches nothing."""
    f = pkg.runtime.debug_step_linear
    z = lambda *s: np.zeros(s, F32)   # noqa: E731
    ones = (np.ones(512, F32), np.zeros(512, F32))
    bad = {
        "LN|PARTIAL without the affine": dict(x=z(16, 512), w=z(64, 512), ln=True, planes=z(2, 16, 512)),
        "LN|MOD|PARTIAL": dict(x=z(16, 512), w=z(64, 512), ln=True, shift=z(16, 512), mscale=z(16, 512), planes=z(2, 16, 512)),
        "K = 1104 over 4: an empty last slice": dict(x=z(16, 1104), w=z(64, 1104), splitk=4),
        "K % 8 != 0": dict(x=z(16, 100), w=z(64, 100)),
        "M = 257": dict(x=z(257, 512), w=z(64, 512)),
        "an f32 slice deeper than 1024": dict(x=z(16, 4096), w=z(64, 4096), splitk=2),
        "pgate": dict(x=z(16, 512), w=z(64, 512), ln=True, ln_wb=ones, planes=z(1, 16, 512), pgate=True),
        "ldmod % 4 != 0": dict(x=z(16, 512), w=z(64, 512), ln=True, shift=z(16, 514), mscale=z(16, 514)),
    }
    for what, kw in bad.items():
        kw = dict(kw)
        with pytest.raises(pkg.PttsError) as e:
            f(kw.pop("x"), kw.pop("w"), **kw)
        assert e.value.code == pkg.runtime.PTTS_EINVAL, what
    # and their neighbours are taken: K = 1104 over 3 (slices of 384: the last one holds 336), LN|AFFINE|PARTIAL
    assert np.isfinite(f(z(16, 1104), z(64, 1104), splitk=3)["out"]).all()
    assert np.isfinite(f(z(16, 512), z(64, 512), ln=True, ln_wb=ones, planes=z(2, 16, 512))["out"]).all()
