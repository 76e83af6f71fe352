"""The many-row GEMMs (csrc/kernels.hip k_gemm, gemm2.hip, gemm3.hip, gemm_wres.hip, gemm5.hip) stand-alone, value by value, against f64 numpy on the same host
operands -- every launch form the host can pick, at the smallest shape that reaches it.

What they replace: every Linear / Conv1d / ConvTranspose1d of the Mimi decoder and the prompt prefill at hundreds to millions of rows (linear.go:117-182,
conv1d.go:20-83, convtranspose1d.go:73-148) with the epilogues of kernels.h Epi and interleaved-pair RoPE (rope.go:81-105).  The hook (ptts_debug_gemm_rows) runs
ONE launch of a named kernel on the caller's buffers with kernels.h' RowMaps on A and C, fills C with 0xff bytes first and returns it whole; it checks every row of
both maps against the buffers before anything is uploaded (these kernels clamp addresses instead of bounding loads).

Forms (restated in plan() below, asserted in test_cases_reach_every_instance): k_gemm3<BN 32|64|128, f32|bf16, NW 4|8, CH 64|128> and <256, ., 8, 64>;
k_gemm5<BN 128|256, NW 4|8, ELU_A>; k_gemm_wres<256,256> and <128,512> with rgl row groups per XCD; k_gemm2<BN 32|64|128, f32|bf16>; k_gemm<f32|bf16>.  Every test
id names kernel, form, weight format and epilogue.

Bound: the arithmetic is exact up to the bf16 hi + lo split of the activations (2^-17), the same split of f32 weights with lo * lo dropped (2^-17 + 2^-18) and f32
accumulation, so |error| <= 3e-5 * (sum_k |a_k w_k| + |bias| + |R|) + 1e-6 -- the bound tests/test_gpu_step_linear.py and tests/test_gpu_tall.py use -- times the
epilogue's Lipschitz bound (GELU 1.2, SiLU 1.1, ELU 1; a scale, gate or alpha multiplies the product's share), times the plane count for a split sum.  RoPE carries
the pair's pre-rotation bounds through the rotation (|cos| b_x + |sin| b_y: never more than (|cos| + |sin|) max(b_x, b_y)) and adds the f32 rounding of two products
and one sum, 2^-23 (|x cos| + |y sin|).  ELU on the hardware exponential (elu_fast: __expf = v_exp_f32(x log2 e)) adds ELU_ABS per activation (times sum_k |w_k|) in
the prologue and per output in the epilogue: 4 x the worst |elu_fast - expm1| test_elu_fast_against_f64 measured on the MI355X through this hook with identity
weights, where the product is exact (profiles/many_row_gemm_parity_observed.json).  test_emulation_stays_within_half_the_bound (no GPU) holds a numpy emulation of
the kernels' arithmetic to HALF the bound on every case; test_planted_defects_exceed_the_bound plants the defects such kernels get into that emulation."""
import math
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _kernel_ref import bf16_round, check_bound, elu64, silu64, untouched
from _parity import record

TOL = 3e-5
FLOOR = 1e-6
ELU_ABS = 2.61e-7    # 4 x 6.51e-8, the worst |elu_fast - expm1| test_elu_fast_against_f64 observed on the MI355X (see its docstring)
RND = 2.0 ** -23
EPI = ["none", "gelu", "silu", "elu", "resadd", "scale_resadd", "gate_resadd", "axpy", "resadd_elu"]
F32 = np.float32
DISPATCH, K_GEMM, K_GEMM2, K_GEMM3, K_WRES, K_GEMM5 = 0, 1, 2, 3, 4, 5
KNAME = ["dispatch", "k_gemm", "k_gemm2", "k_gemm3", "k_gemm_wres", "k_gemm5"]
CUS = 256            # compute units plan() assumes for the production rgl (MI355X); the GPU tests take the device's from the hook


# ------------------------------------------------------------------------------------------------ number formats, functions
try:
    from scipy.special import erf as erf64
except ImportError:   # pragma: no cover
    def erf64(v):
        return np.vectorize(math.erf, otypes=[np.float64])(v)


def gelu64(v):
    return 0.5 * v * (1.0 + erf64(v / math.sqrt(2.0)))


def elu_fast32(v):
    """device_util.h elu_fast in f32: v <= 0 ? exp2(fl(v log2 e)) - 1 : v (the hardware exponential taken as correctly rounded)."""
    v = np.asarray(v, F32)
    y = np.minimum(v, F32(0.0)) * F32(1.4426950408889634)
    return np.where(v <= 0, np.exp2(y.astype(np.float64)).astype(F32) - F32(1.0), v).astype(F32)


def elu32(v):
    v = np.asarray(v, F32)
    return np.where(v <= 0, np.exp(np.minimum(v, F32(0.0)).astype(np.float64)).astype(F32) - F32(1.0), v).astype(F32)


# ------------------------------------------------------------------------------------------------ cases
def case(kern, M, N, K, wb=1, epi=0, **kw):
    """a / cl: the RowMaps -- ("flat", pad): ld = width + pad; ("seg", S, H, pad): segments of S rows behind H history rows each; ("win", S, T, Cc) (A only):
    overlapping windows of T rows of Cc channels (K = T Cc, row stride Cc), T - 1 history rows per segment of S.  rope: (hd, cols, mode) with mode "seg" (positions
    3 + m % 50), "flat" (3 + m) or "rowpos" (a table with repeated, out-of-order positions)."""
    c = dict(kern=kern, M=M, N=N, K=K, wb=wb, epi=epi, cfg=0, rgl=0, aop=0, bias=True, scale=epi == 5, addvec=epi == 2, inplace=False, a=("flat", 0), cl=("flat", 0),
             rope=None, kslice=0, win=None, ldw_pad=0)
    c.update(kw)
    return c


def amap(c):
    """(ld, rows_per_batch, batch_stride, off, elems) of A."""
    M, K, lay = c["M"], c["K"], c["a"]
    if lay[0] == "flat":
        ld = K + lay[1]
        return ld, 0, 0, 0, M * ld
    if lay[0] == "seg":
        _, S, H, pad = lay
        ld = K + pad
        return ld, S, (H + S) * ld, H * ld, -(-M // S) * (H + S) * ld
    _, S, T, Cc = lay
    assert K == T * Cc
    return Cc, S, (T - 1 + S) * Cc, 0, -(-M // S) * (T - 1 + S) * Cc


def cmap(c):
    """(ld, rows_per_batch, batch_stride, off, elems of one plane) of C."""
    M, N, lay = c["M"], c["N"], c["cl"]
    if lay[0] == "flat":
        ld = N + lay[1]
        return ld, 0, 0, 0, M * ld
    _, S, H, pad = lay
    ld = N + pad
    return ld, S, (H + S) * ld, H * ld, -(-M // S) * (H + S) * ld


def row_offsets(m, M):
    ld, rpb, bs, off = m[:4]
    r = np.arange(M, dtype=np.int64)
    return off + ((r // rpb) * bs + (r % rpb) * ld if rpb else r * ld)


def planes(c):
    return -(-c["K"] // c["kslice"]) if c["kslice"] else 1


# ------------------------------------------------------------------------------------------------ host logic of the launchers (restated)
def _al(c, kalign):   # the alignment conditions every *_supported shares (csrc/gemm_tile.h gemm_operands_aligned)
    a, cm = amap(c), cmap(c)
    return a[0] % 4 == 0 and a[2] % 4 == 0 and a[3] % 4 == 0 and (c["K"] + c["ldw_pad"]) % kalign == 0, cm[0] % 4 == 0 and cm[2] % 4 == 0 and cm[3] % 4 == 0


def wres_shape(c):
    a_ok, c_ok = _al(c, 8)
    if not (c["wb"] and c["K"] % 32 == 0 and c["N"] % 4 == 0 and c["M"] >= 2048 and c["aop"] == 0 and c["epi"] in (0, 1, 3) and not c["rope"] and not c["kslice"]
            and a_ok and c_ok):
        return 0
    if 128 < c["K"] <= 256 and 128 < c["N"] <= 256:
        return 1
    if 256 < c["K"] <= 512 and c["N"] >= 512 and (c["N"] + 127) // 128 <= 32 and c["M"] >= 16384:
        return 2
    return 0


def wres_rgl(c, cus=CUS):
    """(production rgl, largest rgl)."""
    per = max(1, cus // 8)
    if wres_shape(c) == 1:
        return max(1, min(per, ((c["M"] + 31) // 32 + 63) // 64)), per
    mx = max(1, per // ((c["N"] + 127) // 128))
    return mx, mx


def gemm5_supported(c):
    a_ok, c_ok = _al(c, 8)
    M, N, K, ks, w = c["M"], c["N"], c["K"], c["kslice"], c["win"]
    if w and (w[0] < 2 or w[1] % 64 or K != w[0] * w[1] or ks):
        return False
    return bool(c["wb"] and c["epi"] in (0, 1, 3, 4, 5, 8) and M >= 1024 and K % 64 == 0 and K >= 64 and N % 128 == 0 and a_ok and c_ok and
                (not ks or (ks % 64 == 0 and K % ks == 0 and c["epi"] == 0 and not c["bias"] and not c["rope"])) and
                (not c["rope"] or (c["rope"][0] == 64 and c["rope"][1] % 64 == 0 and c["epi"] == 0)))


def gemm3_supported(c):
    a_ok, c_ok = _al(c, 8 if c["wb"] else 4)
    ks = c["kslice"]
    return bool(c["M"] >= 512 and c["K"] % 32 == 0 and c["N"] % 4 == 0 and a_ok and c_ok and (not c["rope"] or (c["rope"][0] % 4 == 0 and c["rope"][1] % 4 == 0 and c["epi"] == 0))
                and (not ks or (ks % 128 == 0 and c["epi"] == 0 and not c["bias"] and not c["rope"])))


def gemm2_supported(c):
    kalign = 8 if c["wb"] else 4
    return bool(c["M"] >= 96 and c["K"] % kalign == 0 and _al(c, kalign)[0])


def dispatch(c):
    """launch_gemm / launch_gemm_rope above 256 rows (no tiled weight copy: the step kernel is not in reach)."""
    if c["kern"] != DISPATCH:
        return c["kern"]
    if c["rope"]:
        return K_GEMM5 if gemm5_supported(c) else K_GEMM3
    return K_WRES if wres_shape(c) else K_GEMM5 if gemm5_supported(c) else K_GEMM3 if gemm3_supported(c) else K_GEMM2 if gemm2_supported(c) else K_GEMM


def plan(c, cus=CUS):
    """the template instance case c reaches: ("k_gemm3", BN, bf16, NW, CH), ("k_gemm5", BN, NW, ELU_A), ("k_gemm_wres", N tile, K, rgl, most panels of a wave),
    ("k_gemm2", BN, bf16), ("k_gemm", bf16)."""
    M, N, K, cfg, k = c["M"], c["N"], c["K"], c["cfg"], dispatch(c)
    if k == K_GEMM3:
        assert gemm3_supported(c) and cfg in (0, 1, 2, 3, 4, 6) and not (cfg == 4 and N < 256)
        wide = cfg == 4 or (cfg == 0 and N >= 512 and M >= 16384)
        narrow = cfg == 0 and M < 16384 and ((M + 127) // 128) * ((N + 127) // 128) * planes(c) < 200
        if wide and N >= 256:
            return "k_gemm3", 256, c["wb"], 8, 64
        bn = 128 if (N > 64 and not narrow) else 64 if N > 32 else 32
        nw, ch = {1: (4, 64), 2: (4, 128), 3: (8, 64), 6: (8, 128)}.get(cfg, (4, 64) if M < 16384 else (8, 128))
        return "k_gemm3", bn, c["wb"], nw, ch
    if k == K_GEMM5:
        assert gemm5_supported(c) and cfg in (0, 1, 2, 3, 4) and not (cfg in (1, 2) and N % 256)
        bn, nw = {1: (256, 8), 2: (256, 4), 3: (128, 8), 4: (128, 4)}.get(cfg, (128, 4) if M < 16384 else (256, 8) if N % 256 == 0 else (128, 8))
        return "k_gemm5", bn, nw, c["aop"]
    if k == K_WRES:
        sh = wres_shape(c)
        assert sh
        prod, mx = wres_rgl(c, cus)
        rgl = c["rgl"] or prod
        assert 1 <= rgl <= mx
        return ("k_gemm_wres",) + ((256, 256), (128, 512))[sh - 1] + (rgl, -(-((M + 31) // 32) // (64 * rgl)))
    if k == K_GEMM2:
        assert gemm2_supported(c) and not c["rope"] and not c["kslice"]
        return "k_gemm2", 128 if N > 64 else 64 if N > 32 else 32, c["wb"]
    assert not (wres_shape(c) or gemm5_supported(c) or gemm3_supported(c) or gemm2_supported(c)) and not c["rope"] and not c["kslice"]
    return "k_gemm", c["wb"]


def census_name(c):
    p = plan(c)
    if p[0] == "k_gemm_wres":
        return f"k_gemm_wres<{p[1]},{p[2]}>"
    return p[0] + (("+rope" if c["rope"] else "+splitk" if c["kslice"] else "") if p[0] in ("k_gemm3", "k_gemm5") else "")


def cid(c):
    p = plan(c)
    s = ("dispatch:" if c["kern"] == DISPATCH else "") + p[0] + "<" + ",".join(str(v) for v in p[1:]) + ">" + (f"cfg{c['cfg']}" if c["cfg"] else "") + f"-{c['M']}x{c['N']}x{c['K']}-" + ("bf16" if c["wb"] else "f32")
    s += f"-{EPI[c['epi']]}" + ("-inplace" if c["inplace"] else "") + ("-elu_a" if c["aop"] else "") + ("" if c["bias"] else "-nobias")
    s += ("-noscale" if c["epi"] == 5 and not c["scale"] else "") + ("-noaddvec" if c["epi"] == 2 and not c["addvec"] else "")
    if c["rope"]:
        s += f"-rope{c['rope'][0]}c{c['rope'][1]}{c['rope'][2]}"
    if c["kslice"]:
        s += f"-kslice{c['kslice']}"
    if c["win"]:
        s += f"-win{c['win'][0]}x{c['win'][1]}"
    for key in ("a", "cl"):
        if c[key] != ("flat", 0):
            s += f"-{key}" + "_".join(str(v) for v in c[key])
    return s + (f"-ldw{c['ldw_pad']}" if c["ldw_pad"] else "")


SEG_A, SEG_C = ("seg", 100, 6, 0), ("seg", 100, 3, 8)
_KS = (32, 96, 160, 544)
# k_gemm3: every <BN, weights, NW, CH> through the forced cfgs at M = 520 (a 128-row block with 8 live rows; 5 panels: the pan >= npan return) and 777 (256-row
# panels: 4, the last one ragged), K = 32 (fewer steps than the ring), 96 / 160 (no whole number of 64- / 128-deep chunks), 544; cfg 0 is the production choice
# (narrow: 64-column blocks below 200 tiles)
G3_FORMS = [case(K_GEMM3, (520, 777)[(i + j) % 2], n, _KS[(i + j + wb) % 4], wb=wb, cfg=cfg)
            for wb in (0, 1) for i, cfg in enumerate((1, 2, 3, 6)) for j, n in enumerate((4, 36, 132))] + \
           [case(K_GEMM3, 777, 260, 160, wb=wb, cfg=4) for wb in (0, 1)] + \
           [case(K_GEMM3, (520, 777)[j % 2], n, _KS[j % 4], wb=j % 2, cfg=0) for j, n in enumerate((4, 36, 68, 132, 200, 260))] + \
           [case(K_GEMM3, 777, 200, 96, wb=0, cfg=6, ldw_pad=8, a=("flat", 8), cl=("flat", 4)), case(K_GEMM3, 520, 68, 544, wb=1, cfg=2, ldw_pad=8, a=("flat", 4))]
# all nine epilogues at one ragged shape, R in place and apart, addvec / scale present and absent, the ELU prologue
G3_EPIS = [case(K_GEMM3, 777, 200, 160, wb=e % 2, epi=e, cfg=(1, 3)[e % 2], inplace=e in (4, 6, 8), cl=("flat", 4)) for e in range(9)] + \
          [case(K_GEMM3, 777, 200, 160, wb=(e + 1) % 2, epi=e, cfg=(2, 6)[e % 2], inplace=e in (5, 7), cl=("flat", 4)) for e in range(4, 9)] + \
          [case(K_GEMM3, 777, 200, 160, wb=1, epi=2, addvec=False), case(K_GEMM3, 777, 200, 160, wb=0, epi=5, scale=False, inplace=True),
           case(K_GEMM3, 520, 132, 96, wb=0, epi=3, aop=1, cfg=1), case(K_GEMM3, 777, 68, 544, wb=1, epi=8, aop=1, cfg=6), case(K_GEMM3, 520, 36, 32, wb=1, epi=0, bias=False)]
G3_ROPE = [case(K_GEMM3, 520, 192, 96, wb=1, rope=(64, 128, "seg"), cfg=1), case(K_GEMM3, 777, 132, 160, wb=0, rope=(32, 88, "seg"), cfg=3, bias=False),
           case(K_GEMM3, 520, 96, 32, wb=1, rope=(32, 64, "rowpos")), case(K_GEMM3, 777, 192, 96, wb=0, rope=(64, 128, "rowpos"), cfg=6),
           case(K_GEMM3, 520, 132, 544, wb=1, rope=(32, 88, "flat"), cfg=2), case(K_GEMM3, 777, 384, 160, wb=1, rope=(64, 256, "seg"), cfg=4, a=SEG_A, cl=SEG_C)]
G3_SPLIT = [case(K_GEMM3, 520, 132, 544, wb=wb, kslice=128, bias=False, cfg=cfg) for wb, cfg in ((0, 1), (1, 6), (1, 0))] + \
           [case(K_GEMM3, 520, 36, 2048, wb=1, kslice=1024, bias=False), case(K_GEMM3, 777, 68, 2048, wb=0, kslice=1024, bias=False, cfg=3, cl=SEG_C)]
G3_MAPS = [case(K_GEMM3, 520, 132, 96, wb=wb, epi=4 * wb, a=SEG_A, cl=SEG_C, cfg=(1, 6)[wb], inplace=bool(wb)) for wb in (0, 1)] + \
          [case(K_GEMM3, 777, 68, 192, wb=wb, epi=(3, 8)[wb], aop=1, a=("win", 100, 3, 64), cl=SEG_C, win=(3, 64), cfg=(2, 3)[wb]) for wb in (0, 1)]
# k_gemm5: cfg 1..4 and the production choice, each with and without the ELU prologue; its six epilogues; bias / scale absent; the whole-tile and the per-column
# RoPE switch; split-K; the window order
G5_FORMS = [case(K_GEMM5, (1030, 1290)[(i + aop) % 2], 512 if cfg in (1, 2) else (128, 384)[aop], (64, 128, 448)[(i + aop) % 3], cfg=cfg, aop=aop, epi=(0, 3)[aop])
            for i, cfg in enumerate((0, 1, 2, 3, 4)) for aop in (0, 1)]
G5_EPIS = [case(K_GEMM5, 1030, 384, 128, epi=e, cfg=(0, 3, 4)[i % 3], inplace=e in (4, 8), cl=("flat", 4)) for i, e in enumerate((0, 1, 3, 4, 5, 8))] + \
          [case(K_GEMM5, 1290, 512, 64, epi=5, cfg=1, scale=False, bias=False), case(K_GEMM5, 1030, 128, 448, epi=0, cfg=0, bias=False),
           case(K_GEMM5, 1290, 512, 128, epi=8, cfg=2, bias=False, inplace=True, aop=1), case(K_GEMM5, 1030, 384, 64, epi=5, cfg=3, inplace=True)]
G5_ROPE = [case(K_GEMM5, 1030, 384, 128, rope=(64, 256, "seg"), cfg=0), case(K_GEMM5, 1290, 512, 64, rope=(64, 320, "seg"), cfg=1),
           case(K_GEMM5, 1030, 512, 128, rope=(64, 320, "flat"), cfg=2, bias=False), case(K_GEMM5, 1290, 384, 448, rope=(64, 256, "rowpos"), cfg=3, a=SEG_A, cl=SEG_C)]
G5_SPLIT = [case(K_GEMM5, 1030, 128, 128, kslice=64, bias=False), case(K_GEMM5, 1290, 384, 448, kslice=64, bias=False, cfg=3),
            case(K_GEMM5, 1030, 128, 2048, kslice=1024, bias=False), case(K_GEMM5, 1030, 512, 2048, kslice=1024, bias=False, cfg=1, cl=SEG_C)]
G5_WIN = [case(K_GEMM5, 1030, 128, 448, epi=3, a=("win", 103, 7, 64), cl=("seg", 103, 2, 4), win=(7, 64)),
          case(K_GEMM5, 1290, 512, 448, epi=3, a=("win", 129, 7, 64), cl=("seg", 129, 2, 4), win=(7, 64), cfg=1),
          case(K_GEMM5, 1030, 384, 384, epi=3, aop=1, a=("win", 103, 3, 128), cl=("seg", 103, 2, 4), win=(3, 128), cfg=3),
          case(K_GEMM5, 1290, 128, 384, epi=8, aop=1, a=("win", 129, 3, 128), cl=("seg", 129, 2, 4), win=(3, 128), cfg=4)]
# k_gemm_wres: the 256 x 256 form at K = 160 (five steps: no multiple of the ring of four) and 256, rgl = production and 1 (M = 4100: waves with 3 and with 2
# panels, a 4-row last panel), the transposed convolution's maps; the 128 x 512 form needs 16384 rows (four cases)
WR_256 = [case(K_WRES, m, n, k, epi=e, rgl=rgl, bias=b) for (m, n, k, e, rgl, b) in
          ((2048, 132, 160, 0, 0, True), (2048, 256, 256, 3, 1, True), (4100, 132, 256, 1, 0, False), (4100, 256, 160, 0, 1, True), (4100, 132, 160, 3, 1, False),
           (4100, 256, 256, 1, 1, True), (4100, 200, 160, 0, 2, True))] + \
         [case(K_WRES, 4100, 256, 256, epi=0, rgl=rgl, a=("win", 205, 2, 128), cl=("seg", 205, 1, 0)) for rgl in (0, 1)]
WR_512 = [case(K_WRES, 16384, 512, 288, epi=0), case(K_WRES, 16390, 640, 512, epi=1, rgl=1), case(K_WRES, 16390, 512, 512, epi=3, rgl=1, bias=False),
          case(K_WRES, 16384, 640, 288, epi=0, a=("win", 2048, 2, 144), cl=("seg", 2048, 1, 0))]
# k_gemm2 and k_gemm: the only many-row paths for odd shapes -- every epilogue once, both weight formats; k_gemm at a K that is no multiple of 4 and an unaligned ld
G2 = [case(K_GEMM2, (96, 300, 333)[e % 3], (20, 50, 70, 132)[e % 4], ((36, 100), (40, 104))[e % 2][(e // 2) % 2], wb=e % 2, epi=e, inplace=e in (4, 7),
           a=("flat", 4 * (e % 2)), cl=("flat", e % 3)) for e in range(9)] + \
     [case(K_GEMM2, 300, 70, 104, wb=1, epi=3, aop=1, a=("seg", 100, 2, 4), cl=("seg", 100, 1, 1)), case(K_GEMM2, 129, 33, 36, wb=0, epi=0, bias=False),
      case(K_GEMM2, 96, 20, 40, wb=1, epi=0)]
G1 = [case(K_GEMM, (70, 300, 333)[e % 3], (20, 50, 70, 132)[e % 4], (30, 37, 66)[e % 3], wb=e % 2, epi=e, inplace=e in (5, 8), a=("flat", e % 2), cl=("flat", e % 3))
      for e in range(9)] + \
     [case(K_GEMM, 300, 70, 64, wb=0, epi=0, a=("flat", 1)), case(K_GEMM, 300, 33, 30, wb=1, epi=3, aop=1, a=("seg", 100, 2, 1), cl=("seg", 100, 1, 0), bias=False)]
# launch_gemm above 256 rows, one case per branch, and launch_gemm_rope's two
DISP = [case(DISPATCH, 2048, 132, 160, epi=3), case(DISPATCH, 1030, 128, 64, epi=4), case(DISPATCH, 520, 132, 96, wb=0, epi=6), case(DISPATCH, 1030, 132, 64, epi=1),
        case(DISPATCH, 300, 70, 40, epi=7), case(DISPATCH, 300, 70, 30, wb=0, epi=2), case(DISPATCH, 1030, 384, 128, rope=(64, 256, "seg")),
        case(DISPATCH, 520, 132, 96, wb=0, rope=(32, 88, "seg")), case(DISPATCH, 1030, 128, 128, kslice=64, bias=False), case(DISPATCH, 520, 36, 544, kslice=128, bias=False)]
GROUPS = {"gemm3-forms": G3_FORMS, "gemm3-epilogues": G3_EPIS, "gemm3-rope": G3_ROPE, "gemm3-split": G3_SPLIT, "gemm3-maps": G3_MAPS, "gemm5-forms": G5_FORMS,
          "gemm5-epilogues": G5_EPIS, "gemm5-rope": G5_ROPE, "gemm5-split": G5_SPLIT, "gemm5-windows": G5_WIN, "wres-256": WR_256, "wres-512": WR_512, "gemm2": G2,
          "gemm": G1, "dispatch": DISP}
ALL = [c for g in GROUPS.values() for c in g]


def test_cases_reach_every_instance():
    got = {plan(c) for c in ALL}
    assert got >= {("k_gemm3", bn, wb, nw, ch) for bn in (32, 64, 128) for wb in (0, 1) for nw in (4, 8) for ch in (64, 128)} | {("k_gemm3", 256, wb, 8, 64) for wb in (0, 1)}
    assert got >= {("k_gemm5", bn, nw, elu) for bn in (128, 256) for nw in (4, 8) for elu in (0, 1)}
    assert got >= {("k_gemm2", bn, wb) for bn in (32, 64, 128) for wb in (0, 1)} | {("k_gemm", 0), ("k_gemm", 1)}
    wr = {p for p in got if p[0] == "k_gemm_wres"}
    # the 256 x 256 form with one, two and three panels per wave (rgl 1 at 4100 rows: 129 panels over 64 waves), production's rgl 3; the 128 x 512 form at both
    assert {p[1:3] for p in wr} == {(256, 256), (128, 512)} and {p[4] for p in wr if p[1] == 256} >= {1, 2, 3} and ("k_gemm_wres", 256, 256, 3, 1) in wr
    assert {p[3] for p in wr if p[1] == 128} >= {1, 6, 8} and max(p[4] for p in wr if p[1] == 128) == 9
    assert len(WR_512) <= 4
    for name, g in GROUPS.items():
        assert len({cid(c) for c in g}) == len(g), name
    for k, grp in ((K_GEMM3, G3_EPIS), (K_GEMM2, G2), (K_GEMM, G1)):
        assert {c["epi"] for c in grp} == set(range(9)) and all(c["kern"] == k for c in grp)
    assert {c["epi"] for c in G5_EPIS + G5_FORMS} == {0, 1, 3, 4, 5, 8}
    # the dispatch: one case per branch of launch_gemm above 256 rows, both of launch_gemm_rope, both split-K kernels
    assert [census_name(c) for c in DISP] == ["k_gemm_wres<256,256>", "k_gemm5", "k_gemm3", "k_gemm3", "k_gemm2", "k_gemm", "k_gemm5+rope", "k_gemm3+rope",
                                              "k_gemm5+splitk", "k_gemm3+splitk"]
    # K = 32: fewer steps than the ring; K no whole number of chunks at CH 64 and 128; a ragged last slice; panels no multiple of 8
    g3 = [c for c in ALL if plan(c)[0] == "k_gemm3"]
    assert any(c["K"] == 32 for c in g3) and any(c["K"] % 64 for c in g3 if plan(c)[4] == 64) and any(c["K"] % 128 for c in g3 if plan(c)[4] == 128)
    assert any(c["kslice"] and c["K"] % c["kslice"] == 32 for c in g3)
    assert all((-(-c["M"] // (32 * plan(c)[3]))) % 8 for c in g3)
    # the cases whose bits are compared with k_gemm3's are cases k_gemm3 takes: all of k_gemm5's without windows and all of k_gemm_wres', but for kslice = 64
    assert [c["kslice"] for c in G5_FORMS + G5_EPIS + G5_ROPE + G5_SPLIT + G5_WIN[:2] + WR_256 + WR_512 if not gemm3_supported(c)] == [64, 64]
    assert gemm3_supported(DISP[8]) is False and DISP[8]["kslice"] == 64


# ------------------------------------------------------------------------------------------------ operands
def rope_tables(n_pos, hd):
    """interleaved-pair tables [n_pos][hd / 2] in f32 (rope.go:81-105: theta_j = 10000^(-2 j / hd))."""
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * (10000.0 ** (-2.0 * np.arange(hd // 2) / hd))[None, :]
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def positions(c, rng=None):
    """(positions [M], n_pos, rope_pos0, rope_rows_per_seg, row table or None)."""
    M, mode = c["M"], c["rope"][2]
    if mode == "seg":
        return 3 + np.arange(M) % 50, 53, 3, 50, None
    if mode == "flat":
        return 3 + np.arange(M), M + 3, 3, 0, None
    pos = np.random.default_rng(zlib.crc32(b"pos" + cid(c).encode())).integers(0, 40, M).astype(np.int32)
    pos[1::7] = pos[0::7][:pos[1::7].size]   # repeated
    return pos, 41, 0, 0, pos


def operands(c):
    """normal activations with a per-row scale spread over 1e-3 .. 1e2 and a few exact zeros, weights N(0, 1 / sqrt(K)), R of the row's order, bias N(0, 1)."""
    rng = np.random.default_rng(zlib.crc32(cid(c).encode()))
    M, N, K = c["M"], c["N"], c["K"]
    am, cm = amap(c), cmap(c)
    nrows = am[4] // am[0]
    abuf = rng.standard_normal((nrows, am[0]), dtype=F32) * (10.0 ** rng.uniform(-3.0, 2.0, (nrows, 1))).astype(F32)
    abuf[rng.random(abuf.shape) < 0.004] = 0.0
    abuf = abuf.reshape(-1)
    W = (rng.standard_normal((N, K + c["ldw_pad"])) / math.sqrt(K)).astype(F32)
    o = {"abuf": abuf, "W": W, "amap": am[:4], "cmap": cm[:4], "zstride": cm[4] if c["kslice"] else 0, "c_elems": cm[4] * planes(c)}
    o["Weff"] = (bf16_round(W) if c["wb"] else W)[:, :K]
    o["aidx"] = row_offsets(am, M)
    o["cidx"] = row_offsets(cm, M)
    A = abuf[o["aidx"][:, None] + np.arange(K)[None, :]]
    o["A"] = A
    o["bias"] = rng.standard_normal(N).astype(F32) if c["bias"] else None
    o["addvec"] = rng.standard_normal(N).astype(F32) if c["addvec"] else None
    o["scale"] = rng.standard_normal(N).astype(F32) if c["scale"] else None
    o["gate"] = rng.standard_normal((M, N + 4), dtype=F32) if c["epi"] == 6 else None
    o["alpha"] = 0.7 if c["epi"] == 7 else 1.0
    o["R"] = None
    if c["epi"] >= 4:
        rms = np.sqrt((A.astype(np.float64) ** 2).mean(axis=1)).astype(F32)
        rb = rng.standard_normal(cm[4], dtype=F32)
        rows = rng.standard_normal((M, N), dtype=F32) * rms[:, None]
        rb[o["cidx"][:, None] + np.arange(N)[None, :]] = rows
        o["R"] = rb
    if c["rope"]:
        pos, n_pos, p0, rps, tab = positions(c)
        o["pos"], o["n_pos"], o["pos0"], o["rps"], o["row_pos"] = pos, n_pos, p0, rps, tab
        o["cos"], o["sin"] = rope_tables(n_pos, c["rope"][0])
    return o


# ------------------------------------------------------------------------------------------------ the operation, in f64 and as the kernels' arithmetic
def k_steps(c, k0, k1, defect=None):
    """[(k of the activations, k of the weights)] of the 32-deep steps of slice [k0, k1) in the kernel's order: plain, or -- k_gemm5 with win_taps -- 64-deep chunks
    channel-block-major."""
    if c["win"] and dispatch(c) == K_GEMM5:
        T, Cc = c["win"]
        ks = [(ch % T) * Cc + (ch // T) * 64 + s for ch in range(c["K"] // 64) for s in (0, 32)]
        if defect == "win_wrong_tap":   # the chunks' weights taken in plain order
            return [(k, 32 * i) for i, k in enumerate(ks)]
        return [(k, k) for k in ks]
    ks = list(range(k0, k1, 32))
    if defect == "skip_last_step" and (k1 - k0) % 64:
        ks = ks[:-1]
    return [(k, k) for k in ks]


def emulated_sums(c, o, a32, k0, k1, defect=None):
    """f32 sums of slice [k0, k1): activations as bf16 hi + lo (round to nearest even), f32 weights as hi + lo with lo * lo dropped, one f32 sum per 32-deep step
    and product kind, the steps in the kernel's order.  k_gemm multiplies in exact f32."""
    M, N = c["M"], c["N"]
    acc = np.zeros((M, N), F32)
    W = o["Weff"]
    if dispatch(c) == K_GEMM:
        for ka, kw in k_steps(c, k0, k1):
            acc = acc + a32[:, ka:min(ka + 32, k1)] @ W[:, kw:min(kw + 32, k1)].T
        return acc
    xh = bf16_round(a32)
    xl = bf16_round(a32 - xh)
    wh = bf16_round(W)
    wl = None if c["wb"] else bf16_round(W - wh)
    for ka, kw in k_steps(c, k0, k1, defect):
        sa, sw = slice(ka, min(ka + 32, k1)), slice(kw, min(kw + 32, k1))
        acc = acc + xh[:, sa] @ wh[:, sw].T
        if defect != "no_lo":
            acc = acc + xl[:, sa] @ wh[:, sw].T
        if wl is not None:
            acc = acc + xh[:, sa] @ wl[:, sw].T
    return acc


def rotate(c, o, pre, dt, defect=None):
    """interleaved-pair RoPE of the first rope_cols columns at each row's position, every product and sum rounded in dt."""
    hd, cols, _ = c["rope"]
    M, half = c["M"], hd // 2
    pos = np.asarray(o["pos"], np.int64)
    p = np.arange(cols // 2)
    if defect == "rope_no_restart":
        pos = o["pos0"] + np.arange(M, dtype=np.int64)
    if defect == "rot_whole_tile":
        bn = plan(c)[1]
        cols = min(c["N"], -(-cols // bn) * bn)
        p = np.arange(cols // 2)
    cos_t, sin_t = rope_tables(int(pos.max()) + 2, hd)
    cos_t[:o["n_pos"]], sin_t[:o["n_pos"]] = o["cos"], o["sin"]
    flat = pos[:, None] * half + (p % 32 if defect == "rope_pair32_as_64" else p % half)[None, :]
    cs, sn = cos_t.reshape(-1)[flat].astype(dt), sin_t.reshape(-1)[flat].astype(dt)
    out = pre.copy()
    x0, x1 = pre[:, 0:cols:2], pre[:, 1:cols:2]
    out[:, 0:cols:2] = x0 * cs - x1 * sn
    out[:, 1:cols:2] = x0 * sn + x1 * cs
    return out, cs, sn


def model(c, o, emulate=False, defect=None):
    """The operation of case c: f64 numpy with the bound of every output, or -- emulate -- the kernels' arithmetic in f32 (optionally with a planted defect)."""
    dt = F32 if emulate else np.float64
    M, N, K, e = c["M"], c["N"], c["K"], c["epi"]
    fast = dispatch(c) in (K_GEMM3, K_GEMM5, K_WRES)
    A = o["A"]
    if defect == "clamped_rows":   # the rows of a last partial panel all read the clamped row M - 1
        pr = 32 * plan(c)[3]
        A = A.copy()
        A[M - M % pr:] = A[M - 1]
    a = (elu_fast32(A) if fast else elu32(A)) if (emulate and c["aop"]) else elu64(A.astype(np.float64)) if c["aop"] else A.astype(dt)
    W = o["Weff"].astype(np.float64)
    absW = np.abs(W)
    ks = c["kslice"] or K
    sums, ab = [], []
    for z in range(planes(c)):
        k0, k1 = z * ks, min(K, (z + 1) * ks)
        sums.append(emulated_sums(c, o, a, k0, k1, defect) if emulate else a[:, k0:k1] @ W[:, k0:k1].T)
        if not emulate:
            ab.append(TOL * (np.abs(a[:, k0:k1]) @ absW[:, k0:k1].T) + (ELU_ABS * absW[:, k0:k1].sum(axis=1)[None, :] if c["aop"] else 0.0))
    res = {}
    if c["kslice"]:   # raw sums per plane; the consumer adds them
        res["planes"] = sums
        res["out"] = np.sum(np.stack([p.astype(np.float64) for p in sums]), axis=0)
        if not emulate:
            res["plane_bounds"] = [b + FLOOR for b in ab]
            res["bound"] = planes(c) * sum(ab) + FLOOR
        return res
    bias = (o["bias"] if o["bias"] is not None else np.zeros(N, F32)).astype(dt)
    pre = sums[0] + bias
    b0 = None if emulate else ab[0] + TOL * np.abs(bias)
    if c["rope"]:
        cols = c["rope"][1]
        x = None if emulate else np.abs(pre)
        pre, cs, sn = rotate(c, o, pre, dt, defect)
        if not emulate:
            cs, sn = np.abs(cs), np.abs(sn)
            be, bo, xe, xo = b0[:, 0:cols:2], b0[:, 1:cols:2], x[:, 0:cols:2], x[:, 1:cols:2]
            b0 = b0.copy()
            b0[:, 0:cols:2] = cs * be + sn * bo + RND * (xe * cs + xo * sn)
            b0[:, 1:cols:2] = sn * be + cs * bo + RND * (xe * sn + xo * cs)
    R = o["R"][o["cidx"][:, None] + np.arange(N)[None, :]].astype(dt) if o["R"] is not None else None
    absR = np.abs(R) if R is not None else 0.0
    eluf = (elu_fast32 if fast else elu32) if emulate else elu64
    p64 = pre if emulate else pre.astype(np.float64)
    bound = None
    if e == 0:
        out, bound = pre, b0
    elif e == 1:
        out = (F32(0.5) * pre * (F32(1.0) + erf64((pre * F32(0.70710678118654752440)).astype(np.float64)).astype(F32))) if emulate else gelu64(p64)
        bound = None if emulate else 1.2 * b0                                   # |gelu'| <= 1.13
    elif e == 2:
        av = (o["addvec"] if o["addvec"] is not None else np.zeros(N, F32)).astype(dt)
        s = av + pre
        with np.errstate(over="ignore"):   # expf(-s) = inf below -88: s / inf = -0, as on the device
            out = (s / (F32(1.0) + np.exp(-s.astype(np.float64)).astype(F32))) if emulate else silu64(s)
        bound = None if emulate else 1.1 * (b0 + TOL * np.abs(av))             # |silu'| <= 1.0998
    elif e == 3:
        out, bound = eluf(pre), None if emulate else b0 + ELU_ABS
    elif e == 4:
        out, bound = R + pre, None if emulate else b0 + TOL * absR
    elif e == 5:
        sc = (o["scale"] if o["scale"] is not None else np.ones(N, F32)).astype(dt)
        out, bound = R + sc * pre, None if emulate else np.abs(sc) * b0 + TOL * absR
    elif e == 6:
        g = o["gate"][:, :N].astype(dt)
        out, bound = R + g * pre, None if emulate else np.abs(g) * b0 + TOL * absR
    elif e == 7:
        out, bound = R + dt(o["alpha"]) * pre, None if emulate else abs(o["alpha"]) * b0 + TOL * absR
    else:
        out, bound = eluf(R + pre), None if emulate else b0 + TOL * absR + ELU_ABS
    res["out"] = np.asarray(out, np.float64)
    if not emulate:
        res["bound"] = np.asarray(bound, np.float64) + FLOOR
    return res


def reference(c):
    """operands and f64 model of a case.  Every case is checked once, so nothing is kept for the session."""
    o = operands(c)
    return o, model(c, o)


def ratios(c, ref, emu):
    """error / bound of an emulated (or measured) result: the output (a split: the sum of the planes) and every plane."""
    out = [float((np.abs(emu["out"] - ref["out"]) / ref["bound"]).max())]
    if c["kslice"]:
        out += [float((np.abs(p.astype(np.float64) - q) / b).max()) for p, q, b in zip(emu["planes"], ref["planes"], ref["plane_bounds"])]
    return out


# ------------------------------------------------------------------------------------------------ the emulation against the bound: no GPU
@pytest.mark.parametrize("group", list(GROUPS))
def test_emulation_stays_within_half_the_bound(group):
    """The kernels' arithmetic, emulated in numpy, stays within HALF the bound the GPU tests use, for every case of this file: the bound has room for the kernels."""
    worst = 0.0
    for c in GROUPS[group]:
        o = operands(c)
        r = max(ratios(c, model(c, o), model(c, o, emulate=True)))
        worst = max(worst, r)
        assert r <= 0.5, (cid(c), r)
    print(f"{group}: emulated error / bound, worst {worst:.3f}")


# each planted defect with the case it must show on (bias added to every split plane has no form to show on: gemm3_supported / gemm5_supported refuse a bias with
# kslice, and the hook refuses what they refuse)
DEFECTS = {
    "no_lo": G3_FORMS[0],                    # K = 32: the activations' lo plane dropped, 2^-9 per product
    "skip_last_step": G3_SPLIT[0],           # kslice 128 at K = 544: the last slice is one 32-deep step
    "clamped_rows": G3_FORMS[1],             # M = 777, 128-row panels: rows 768 .. 775 read row 776
    "rope_no_restart": G3_ROPE[0],           # positions 3 + m instead of 3 + m % 50
    "rope_pair32_as_64": G3_ROPE[1],         # a 32-wide head's pair index computed as for 64
    "win_wrong_tap": G5_WIN[2],              # the window order's chunks against the plain order's weights (3 x 128: with one 64-channel block per tap, 7 x 64, the two orders are one)
    "rot_whole_tile": G5_ROPE[1],            # rope_cols = 320 inside a 256-column tile: columns 320 .. 511 rotated too
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_exceed_the_bound(defect):
    c = DEFECTS[defect]
    shows = {"no_lo": lambda: c["K"] == 32, "skip_last_step": lambda: c["kslice"] and c["K"] % c["kslice"] == 32, "clamped_rows": lambda: c["M"] % (32 * plan(c)[3]) > 1,
             "rope_no_restart": lambda: c["rope"] and c["rope"][2] == "seg", "rope_pair32_as_64": lambda: c["rope"] and c["rope"][0] == 32,
             "win_wrong_tap": lambda: c["win"] and c["win"][1] > 64 and plan(c)[0] == "k_gemm5", "rot_whole_tile": lambda: c["rope"] and c["rope"][1] % plan(c)[1] != 0}
    assert shows[defect](), cid(c)
    o = operands(c)
    ref = model(c, o)
    assert max(ratios(c, ref, model(c, o, emulate=True))) <= 0.5
    r = max(ratios(c, ref, model(c, o, emulate=True, defect=defect)))
    print(f"{defect} on {cid(c)}: error / bound {r:.3g}")
    assert r > 1.0, (defect, cid(c), r)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
def check(name, got, want, bound):
    check_bound(name, got, want, bound, TOL)


def run(pkg, c, o, **over):
    kw = dict(kernel=c["kern"], cfg=c["cfg"], rgl=c["rgl"], w_bf16=bool(c["wb"]), K=c["K"], aop=c["aop"], epi=c["epi"], alpha=o["alpha"], bias=o["bias"],
              addvec=o["addvec"], scale=o["scale"], gate=o["gate"], residual=o["R"] if not c["kslice"] else None, inplace=c["inplace"], kslice=c["kslice"],
              zstride=o["zstride"], amap=o["amap"], cmap=o["cmap"], c_elems=o["c_elems"])
    if c["rope"]:
        kw.update(rope=(o["cos"], o["sin"]), rope_cols=c["rope"][1], rope_hd=c["rope"][0], rope_pos0=o["pos0"], rope_rows_per_seg=o["rps"], rope_row_pos=o["row_pos"])
    if c["win"]:
        kw.update(win_taps=c["win"][0], win_c=c["win"][1])
    kw.update(over)
    abuf = kw.pop("abuf", o["abuf"])
    return pkg.runtime.debug_gemm_rows(abuf, o["W"], c["M"], **kw)


def gather(c, o, buf):
    """[planes][M][N] of a C buffer, and the buffer's elements outside the map."""
    idx = o["cidx"][:, None] + np.arange(c["N"])[None, :]
    idx = np.stack([idx + z * o["zstride"] for z in range(planes(c))])
    outside = np.ones(buf.size, bool)
    outside[idx.reshape(-1)] = False
    return buf[idx], outside


def check_case(pkg, c, bits_of=None):
    """runs case c; checks the census, every value against the f64 reference, the 0xff fill outside the map; bits_of: another kernel that must give the same bits."""
    o, ref = reference(c)
    r = run(pkg, c, o)
    name = "gemm_rows " + cid(c)
    assert r["launched"] == {census_name(c): 1}, (name, r["launched"])
    if plan(c)[0] == "k_gemm_wres":
        assert r["rgl"] == plan(c, r["cus"])[3], (name, r["rgl"], r["cus"])
    got, outside = gather(c, o, r["out"])
    if c["inplace"]:
        assert np.array_equal(r["out"][outside].view(np.uint32), o["R"][outside].view(np.uint32)), name + ": the in-place residual changed outside the map"
    else:
        assert untouched(r["out"][outside]), name + ": written outside the map"
    if c["kslice"]:
        for z in range(planes(c)):
            check(f"{name} plane {z}", got[z], ref["planes"][z], ref["plane_bounds"][z])
        check(f"{name} sum", got.astype(np.float64).sum(axis=0), ref["out"], ref["bound"])
    else:
        check(name, got[0], ref["out"], ref["bound"])
    if bits_of is not None and gemm3_supported(c):   # all but k_gemm5's kslice = 64: gemm3_supported wants kslice % 128
        assert bits_of == K_GEMM3
        other = run(pkg, c, o, kernel=bits_of, cfg=0, rgl=0)
        assert list(other["launched"]) == [census_name(dict(c, kern=bits_of, cfg=0, rgl=0))]
        assert np.array_equal(other["out"].view(np.uint32), r["out"].view(np.uint32)), name + f": not {KNAME[bits_of]}'s bits"
    return r


@gpu
def test_elu_fast_against_f64(pkg):
    """elu_fast (device_util.h: __expf(v) - 1 = v_exp_f32(v log2 e) - 1) against f64 expm1 over (-500, 0], the range the tests' activations and pre-activations span:
    identity weights and inputs of 16 significant bits make the product exact (hi + lo is the input), so EPI_ELU's output IS elu_fast of the input.  This measures the
    intrinsic, not a GEMM: ELU_ABS is 4 x the worst observed here (MI355X: see profiles/many_row_gemm_parity_observed.json, "elu_fast").  A documented bound was
    looked for first and there is none to take: the installed HIP headers define __expf as __builtin_amdgcn_exp2f(x log2 e) (__clang_hip_math.h) and state no error
    for it or for the builtin, and no math-API accuracy table ships with them."""
    rng = np.random.default_rng(11)
    x = -(10.0 ** rng.uniform(-6.0, 2.7, (512, 128)))
    x[rng.random(x.shape) < 0.01] = 0.0
    u = x.astype(F32).view(np.uint32) & np.uint32(0xFFFFFF00)   # 16 significant bits
    x = u.view(F32)
    hi = bf16_round(x)
    assert np.array_equal(hi + bf16_round(x - hi), x)
    r = pkg.runtime.debug_gemm_rows(x, np.eye(128, dtype=F32), 512, kernel=K_GEMM3, epi=3, amap=(128, 0, 0, 0), cmap=(128, 0, 0, 0), c_elems=512 * 128)
    assert r["launched"] == {"k_gemm3": 1}
    err = np.abs(r["out"].reshape(512, 128).astype(np.float64) - np.expm1(x.astype(np.float64)))
    worst = float(err.max())
    record("gemm_rows elu_fast", worst, worst / ELU_ABS, 1.0, (ELU_ABS, 0))
    print(f"elu_fast: worst |elu_fast - expm1| {worst:.3e} at x = {float(x.reshape(-1)[err.argmax()]):.6g}; ELU_ABS {ELU_ABS:.1e}")
    assert 4.0 * worst <= ELU_ABS


@gpu
@pytest.mark.parametrize("c", G3_FORMS + G3_EPIS + G3_ROPE + G3_SPLIT + G3_MAPS, ids=cid)
def test_gemm3(pkg, c):
    """k_gemm3: every template instance with f32 and bf16 weights, all nine epilogues, RoPE with 64- and 32-wide heads and every position form, split-K with a ragged
    last slice, segmented maps and overlapping windows."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", G5_FORMS + G5_EPIS + G5_ROPE + G5_SPLIT, ids=cid)
def test_gemm5(pkg, c):
    """k_gemm5 against the reference, and -- without windows -- bit for bit k_gemm3 on the same host operands (kslice 64 is no slice k_gemm3 takes)."""
    check_case(pkg, c, bits_of=K_GEMM3)


@gpu
@pytest.mark.parametrize("c", G5_WIN, ids=cid)
def test_gemm5_window_order(pkg, c):
    """k walked channel-block-major over overlapping-window rows: the one form whose last bits may differ from k_gemm3's -- the bound only.  (With one 64-channel
    block per tap, 7 x 64, the channel-block-major order IS the plain order: k_gemm3's bits there too.)"""
    check_case(pkg, c, bits_of=K_GEMM3 if c["win"][1] == 64 else None)


@gpu
@pytest.mark.parametrize("c", WR_256 + WR_512, ids=cid)
def test_gemm_wres(pkg, c):
    """k_gemm_wres' panel walk with one, two and three panels per wave, the ring across panel boundaries, a ragged last panel: the reference, and k_gemm3's bits."""
    check_case(pkg, c, bits_of=K_GEMM3)


@gpu
@pytest.mark.parametrize("c", G2 + G1, ids=cid)
def test_gemm2_and_gemm(pkg, c):
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", DISP, ids=cid)
def test_dispatch(pkg, c):
    """launch_gemm / launch_gemm_rope pick the kernel plan() says (check_case asserts the census name)."""
    check_case(pkg, c)


@gpu
@pytest.mark.parametrize("c", [G3_MAPS[0], G3_MAPS[2], G5_WIN[0], G5_ROPE[3], WR_256[7]], ids=cid)
def test_segments_do_not_see_each_other(pkg, c):
    """with segmented maps, changing one segment's A (history rows included) leaves every other segment's C bits unchanged."""
    o = operands(c)
    clean = run(pkg, c, o)["out"]
    am = amap(c)
    S, seg = am[1], 2
    ab = o["abuf"].copy()
    lo = seg * am[2]
    ab[lo:lo + am[2]] = ab[lo:lo + am[2]] * F32(-1.5) + F32(0.25)
    dirty = run(pkg, c, o, abuf=ab)["out"]
    got_c, _ = gather(c, o, clean)
    got_d, outside = gather(c, o, dirty)
    rows = np.arange(c["M"]) // S == seg
    assert np.array_equal(got_d[0][~rows].view(np.uint32), got_c[0][~rows].view(np.uint32))
    assert (got_d[0][rows] != got_c[0][rows]).mean() > 0.5
    assert np.array_equal(dirty[outside].view(np.uint32), clean[outside].view(np.uint32))


@gpu
def test_refusals_before_any_launch(pkg):
    """what the kernels' predicates, the forced forms' production guards and the buffer check refuse is answered with PTTS_EINVAL, and nothing is launched."""
    f = pkg.runtime.debug_gemm_rows
    z = lambda *s: np.zeros(s, F32)   # noqa: E731

    def flat(M, N, K, **kw):
        d = dict(a_buf=z(M * K), w=z(N, K), M=M, amap=(K, 0, 0, 0), cmap=(N, 0, 0, 0), c_elems=M * N)
        d.update(kw)
        return d

    def call(kw):
        kw = dict(kw)
        return f(kw.pop("a_buf"), kw.pop("w"), kw.pop("M"), **kw)

    tabs = (z(60, 32), z(60, 32))
    per_xcd = max(1, call(flat(2048, 256, 256, kernel=K_WRES, rgl=1))["cus"] // 8)   # the device's, as the hook reports it: 32 on the MI355X
    bad = {
        "k_gemm3 below 512 rows": flat(500, 64, 64, kernel=K_GEMM3),
        "k_gemm3 with K % 32": flat(520, 64, 40, kernel=K_GEMM3),
        "k_gemm3 with a bias on split-K": flat(520, 64, 256, kernel=K_GEMM3, kslice=128, zstride=520 * 64, c_elems=2 * 520 * 64, bias=z(64)),
        "k_gemm3 cfg 5": flat(520, 64, 64, kernel=K_GEMM3, cfg=5),
        "k_gemm3 <256,8,64> at N = 132": flat(520, 132, 64, kernel=K_GEMM3, cfg=4),
        "k_gemm5 with f32 weights": flat(1030, 128, 64, kernel=K_GEMM5, w_bf16=False),
        "k_gemm5 with N % 128": flat(1030, 132, 64, kernel=K_GEMM5),
        "k_gemm5 256-column form at N = 384": flat(1030, 384, 64, kernel=K_GEMM5, cfg=1),
        "k_gemm5 cfg 7": flat(1030, 128, 64, kernel=K_GEMM5, cfg=7),
        "k_gemm5 RoPE with 32-wide heads": flat(1030, 128, 64, kernel=K_GEMM5, rope=(z(60, 16), z(60, 16)), rope_hd=32, rope_cols=64, rope_rows_per_seg=50),
        "k_gemm_wres below 2048 rows": flat(2000, 256, 256, kernel=K_WRES),
        "k_gemm_wres<256,256> rgl CUs / 8 + 1": flat(2048, 256, 256, kernel=K_WRES, rgl=per_xcd + 1),
        "k_gemm_wres<128,512> rgl CUs / 8 / 4 tiles + 1": flat(16384, 512, 288, kernel=K_WRES, rgl=max(1, per_xcd // 4) + 1),
        "k_gemm_wres<128,512> rgl CUs / 8 / 5 tiles + 1": flat(16384, 640, 288, kernel=K_WRES, rgl=max(1, per_xcd // 5) + 1),
        "k_gemm_wres with a negative rgl": flat(2048, 256, 256, kernel=K_WRES, rgl=-1),
        "k_gemm_wres with a cfg": flat(2048, 256, 256, kernel=K_WRES, cfg=1),
        "k_gemm3 with an rgl": flat(520, 64, 64, kernel=K_GEMM3, rgl=1),
        "k_gemm5 with an rgl": flat(1030, 128, 64, kernel=K_GEMM5, rgl=1),
        "k_gemm2 with an rgl": flat(300, 64, 64, kernel=K_GEMM2, rgl=1),
        "k_gemm with an rgl": flat(300, 64, 30, kernel=K_GEMM, w_bf16=False, rgl=1),
        "dispatch with an rgl": flat(2048, 256, 256, kernel=DISPATCH, rgl=1),
        "k_gemm_wres with RESADD": flat(2048, 256, 256, kernel=K_WRES, epi=4, residual=z(2048 * 256)),
        "k_gemm2 with RoPE": flat(300, 64, 64, kernel=K_GEMM2, rope=tabs, rope_cols=64, rope_rows_per_seg=50),
        "k_gemm at a shape k_gemm2 takes": flat(300, 64, 64, kernel=K_GEMM),
        "kernel 6": flat(520, 64, 64, kernel=6),
        "dispatch with a cfg": flat(520, 64, 64, kernel=DISPATCH, cfg=1),
        "A one element short": flat(520, 64, 64, kernel=K_GEMM3, a_buf=z(520 * 64 - 1)),
        "A's last window past the buffer": flat(520, 64, 192, kernel=K_GEMM3, a_buf=z(521 * 64), amap=(64, 0, 0, 0)),
        "C one element short": flat(520, 64, 64, kernel=K_GEMM3, c_elems=520 * 64 - 1),
        "C's last segment past the buffer": flat(520, 64, 64, kernel=K_GEMM3, cmap=(64, 100, 103 * 64, 3 * 64), c_elems=(3 + 5 * 103 + 20) * 64 - 1),
        "a split plane past the buffer": flat(520, 64, 256, kernel=K_GEMM3, kslice=128, zstride=520 * 64, c_elems=2 * 520 * 64 - 1),
        "C's rows overlap (c_ld < N)": flat(520, 64, 64, kernel=K_GEMM3, cmap=(60, 0, 0, 0)),
        "C's segments overlap": flat(520, 64, 64, kernel=K_GEMM3, cmap=(64, 100, 99 * 64, 0)),
        "split planes overlap (zstride one short)": flat(520, 64, 256, kernel=K_GEMM3, kslice=128, zstride=520 * 64 - 1, c_elems=2 * 520 * 64),
        "split planes on top of each other (zstride 0)": flat(520, 64, 256, kernel=K_GEMM3, kslice=128, zstride=0, c_elems=2 * 520 * 64),
        "a zstride without kslice": flat(520, 64, 64, kernel=K_GEMM3, zstride=520 * 64, c_elems=2 * 520 * 64),
        "a position past the tables": flat(520, 64, 64, kernel=K_GEMM3, rope=tabs, rope_cols=64, rope_rows_per_seg=58, rope_pos0=3),
        "rope_row_pos past the tables": flat(520, 64, 64, kernel=K_GEMM3, rope=tabs, rope_cols=64, rope_row_pos=np.full(520, 60, np.int32)),
        "a negative position": flat(520, 64, 64, kernel=K_GEMM3, rope=tabs, rope_cols=64, rope_row_pos=np.full(520, -1, np.int32)),
        "GATE_RESADD without a gate": flat(520, 64, 64, kernel=K_GEMM3, epi=6, residual=z(520 * 64)),
    }
    pkg.runtime.launch_counts(True)
    try:
        for what, kw in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                call(kw)
            assert e.value.code == pkg.runtime.PTTS_EINVAL, what
        assert pkg.runtime.launch_counts(True) == {}
        # and their neighbours are taken (a caller's census sees the hook's launch)
        ok = [flat(520, 64, 64, kernel=K_GEMM3, rope=tabs, rope_cols=64, rope_rows_per_seg=57, rope_pos0=3), flat(1030, 512, 64, kernel=K_GEMM5, cfg=1),
              flat(520, 64, 192, kernel=K_GEMM3, a_buf=z(522 * 64), amap=(64, 0, 0, 0)), flat(2048, 256, 256, kernel=K_WRES, rgl=per_xcd),
              flat(16384, 512, 288, kernel=K_WRES, rgl=max(1, per_xcd // 4)), flat(520, 64, 64, kernel=K_GEMM3, cmap=(64, 100, 100 * 64, 0)),
              flat(520, 64, 256, kernel=K_GEMM3, kslice=128, zstride=520 * 64, c_elems=2 * 520 * 64)]
        for kw in ok:
            assert np.isfinite(call(kw)["out"]).all()
        assert pkg.runtime.launch_counts(False) == {"k_gemm3+rope": 1, "k_gemm5": 1, "k_gemm3": 2, "k_gemm_wres<256,256>": 1, "k_gemm_wres<128,512>": 1, "k_gemm3+splitk": 1}
    finally:
        pkg.runtime.launch_counts(False)
