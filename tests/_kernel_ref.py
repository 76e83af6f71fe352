"""What the value-level kernel tests share (test_gpu_step_linear, _attn_step, _attn_window, _many_row_gemm, _mimi_fused, _seanet_block,
_flow_cluster_values, _step_edge with its reference module _step_edge_ref: ptts_debug_step_edge, and _tall with its reference module _tall_ref, itself checked
without a GPU by test_tall_ref: ptts_debug_tall): the bf16 number format as the kernels round it, the activation functions in float64, the 0xff fill the hooks put
into every output buffer before a launch, and the error-against-bound check.  A helper that one file needs in another form (scipy's erf, a
bound taken at the worst element, an f32 restatement of a kernel's own function) stays in that file."""
import math

import numpy as np

from _parity import record

F32 = np.float32


# ------------------------------------------------------------------------------------------------ number formats
def bf16_round(a):
    """f32 values rounded to bf16, nearest even (finite values: a NaN is not kept a NaN)."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32)


def bf16_bits(a):
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def split(a):
    """the kernels' operand split: hi = bf16(a), lo = bf16(a - hi)"""
    hi = bf16_round(a)
    return hi, bf16_round(a - hi)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def untouched(a):
    """every byte still the 0xff of the hooks' fill"""
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


# ------------------------------------------------------------------------------------------------ functions in float64
def erf64(v):
    return np.vectorize(math.erf, otypes=[np.float64])(v)


def gelu64(v):
    return 0.5 * v * (1.0 + erf64(v / math.sqrt(2.0)))


def silu64(v):
    return v / (1.0 + np.exp(-v))


def elu64(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))


# ------------------------------------------------------------------------------------------------ the check
def check_bound(name, got, want, bound, tol):
    """every element's error against its own bound; the record's max_rel slot holds the worst error / bound ratio"""
    got = np.asarray(got)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max()) if err.size else 0.0
    record(name, float(err.max()) if err.size else 0.0, worst, float(np.abs(want).max()) if err.size else 0.0, (tol, 0))
    print(f"{name}: max abs {float(err.max()) if err.size else 0.0:.3e}, error / bound {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0, (name, float(err.max()), worst)
