"""ctypes face of ``libqg_host.so`` (include/qg/qg_host.h): the reference's CPU entry points
(include/gemm_reference.h, include/quantize.h) as host-only C-ABI twins, on numpy arrays.

Independent of the GPU library and of the test oracle; needs no GPU and no torch.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libqg_host.so")
P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
SIGNATURES = {
    "qg_gemm_w4a8_q4_0_cpu": ([P, P, P, I, I, I], I),
    "qg_vec_dot_q4_0_q8_1_cpu": ([I, P, P, P], None),
    "qg_vec_dot_q8_0_q8_1_cpu": ([I, P, P, P], None),
    "qg_gemm_w8a8_cpu": ([P, P, P, I, I, I], I),
    "qg_gemm_w4a8_cpu_mt": ([P, P, P, I, I, I, I, I], I),
    "qg_gemm_w4a8_moe_cpu": ([P, I, P, I, P, I64, P, I64, I, I, I, I, I, I], I),
    "qg_gemm_w4a8_moe_bias_cpu": ([P, I, P, P, I64, I, P, I64, P, I64, I, I, I, I, I, I], I),
    "qg_gemm_w4a8_moe_glu_cpu": ([P, P, P, I, P, I64, P, I64, I, I, I, I, I, I, I], I),
    "qg_gemm_w4a8_moe_down_cpu": ([P, P, I, P, I64, P, I64, P, I64, I, I, I, I, I, I], I),
    "qg_gemm_w4a8_moe_glu_bias_cpu": ([P, P, P, P, P, I64, I, P, I64, P, I64, I, I, I, I, I, I, F, F, I], I),
    "qg_gemm_w4a8_moe_down_bias_cpu": ([P, P, P, I64, I, P, I64, P, I64, P, I64, I, I, I, I, I, I], I),
    "qg_gemm_fp32_cpu": ([P, P, P, I, I, I], I),
    "qg_quantize_row_q8_1_cpu": ([P, P, I64], I),
    "qg_quantize_row_q4_0_cpu": ([P, P, I64], I),
    "qg_dequantize_row_mxfp4_cpu": ([P, P, I64], I),
    "qg_fill_step4_cpu": ([ctypes.c_uint, I, I, I, I, I, P, P], I),
}
# 12: Q4_K, 14: Q6_K, 256-element super-blocks; 39: MXFP4, 32-element blocks of 17 bytes
BLOCK_BYTES = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34, 9: 36, 12: 144, 14: 210, 39: 17}
GLU_REGLU, GLU_SWIGLU, GLU_SWIGLU_OAI = 0, 2, 3  # QG_GLU_* of qg.h
_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"quant_gemm.host: {LIB_PATH} not built (make -C llama.cpp-quant-gemm_amd/host)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        _lib = lib
    return _lib


def _p(a: np.ndarray) -> ctypes.c_void_p:
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def _ok(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what}: status {rc}")


def fill_step4(m: int, n: int, k: int, seed: int = 42, row0: int = 0, row1: int | None = None):
    """A[m, k], B[row0:row1, k] of the step4 recipe (glibc srand(seed), U[-1, 1], A first)."""
    row1 = n if row1 is None else row1
    a = np.empty((m, k), np.float32)
    b = np.empty((row1 - row0, k), np.float32)
    _ok(load().qg_fill_step4_cpu(seed, m, n, k, row0, row1, _p(a), _p(b)), "fill_step4")
    return a, b


def quantize_q8_1(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape[:-1] + (x.shape[-1] // 32, 36), np.uint8)
    _ok(load().qg_quantize_row_q8_1_cpu(_p(x), _p(out), x.size), "quantize_row_q8_1")
    return out


def quantize_q4_0(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape[:-1] + (x.shape[-1] // 32, 18), np.uint8)
    _ok(load().qg_quantize_row_q4_0_cpu(_p(x), _p(out), x.size), "quantize_row_q4_0")
    return out


def dequantize_mxfp4(x_q: np.ndarray) -> np.ndarray:
    """float32 [..., 32 * blocks] of block_mxfp4 bytes [..., blocks, 17] (qg_dequantize_row_mxfp4_cpu)."""
    x_q = np.ascontiguousarray(x_q, np.uint8)
    assert x_q.shape[-1] == 17
    out = np.empty(x_q.shape[:-2] + (x_q.shape[-2] * 32,), np.float32)
    _ok(load().qg_dequantize_row_mxfp4_cpu(_p(x_q), _p(out), out.size), "dequantize_row_mxfp4")
    return out


def gemm_w4a8(a_q: np.ndarray, b_q: np.ndarray, m: int, n: int, k: int, wtype: int = 2, threads: int = 1) -> np.ndarray:
    """C[m, n] (gemm_w4a8_reference for Q4_0; the corrected block formulas for the other formats)."""
    c = np.empty((m, n), np.float32)
    a_q, b_q = np.ascontiguousarray(a_q), np.ascontiguousarray(b_q)
    _ok(load().qg_gemm_w4a8_cpu_mt(_p(a_q), _p(b_q), _p(c), m, n, k, wtype, threads), "gemm_w4a8_cpu")
    return c


def gemm_w4a8_moe(a_q: np.ndarray, experts_q: np.ndarray, ids: np.ndarray, t: int, n_used: int, n: int, k: int,
                  wtype: int = 2, a_rows: int = 1, threads: int = 1, ids_stride: int | None = None) -> np.ndarray:
    """C[t, n_used, n] of qg_gemm_w4a8_moe_cpu: slot (t, u) = activation row t * a_rows + u % a_rows times expert
    ids[t, u] of ``experts_q`` (n_expert matrices, one after another). ``ids``: int32 [t, ids_stride] (the
    stride defaults to the array's row length); an id outside [0, n_expert) gives zeros."""
    a_q, experts_q = np.ascontiguousarray(a_q), np.ascontiguousarray(experts_q)
    ids = np.ascontiguousarray(ids, np.int32)
    be = 256 if wtype in (12, 14) else 32
    n_expert = experts_q.size // (n * (k // be) * BLOCK_BYTES[wtype])
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    c = np.empty((t, n_used, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_cpu(_p(a_q), a_rows, _p(experts_q), n_expert, _p(ids), ids_stride, _p(c), n, t, n_used, n,
                                    k, wtype, threads), "gemm_w4a8_moe_cpu")
    return c


def gemm_w4a8_moe_glu(a_q: np.ndarray, gate_q: np.ndarray, up_q: np.ndarray, ids: np.ndarray, t: int, n_used: int, n: int,
                      k: int, wtype: int = 12, glu_op: int = GLU_SWIGLU, threads: int = 1,
                      ids_stride: int | None = None) -> np.ndarray:
    """C[t, n_used, n] of qg_gemm_w4a8_moe_glu_cpu: slot (t, u) = glu_op(g) * u with g, u the products of activation
    row t with expert ids[t, u] of ``gate_q`` and of ``up_q`` (n_expert Q4_K / Q6_K matrices each). ``ids``: int32
    [t, ids_stride] (the stride defaults to the array's row length); an id outside [0, n_expert) gives zeros."""
    a_q, gate_q, up_q = np.ascontiguousarray(a_q), np.ascontiguousarray(gate_q), np.ascontiguousarray(up_q)
    ids = np.ascontiguousarray(ids, np.int32)
    if gate_q.size != up_q.size:
        raise RuntimeError("gemm_w4a8_moe_glu_cpu: gate and up experts differ in size")
    n_expert = gate_q.size // (n * (k // 256) * BLOCK_BYTES[wtype])
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    c = np.empty((t, n_used, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_glu_cpu(_p(a_q), _p(gate_q), _p(up_q), n_expert, _p(ids), ids_stride, _p(c), n, t, n_used, n,
                                        k, wtype, glu_op, threads), "gemm_w4a8_moe_glu_cpu")
    return c


def gemm_w4a8_moe_down(a_q: np.ndarray, experts_q: np.ndarray, ids: np.ndarray, weights: np.ndarray | None, t: int,
                       n_used: int, n: int, k: int, wtype: int = 12, threads: int = 1, ids_stride: int | None = None,
                       w_stride: int | None = None) -> np.ndarray:
    """C[t, n] of qg_gemm_w4a8_moe_down_cpu: token t = the sum over u, in ascending order, of weights[t, u] times the
    product of activation row t * n_used + u with expert ids[t, u] of ``experts_q`` (n_expert Q4_K / Q6_K matrices).
    ``ids``: int32 [t, ids_stride], ``weights``: float32 [t, w_stride] or None for ones (the strides default to the
    arrays' row lengths); a slot whose id is outside [0, n_expert) contributes nothing and its weight is not read."""
    a_q, experts_q = np.ascontiguousarray(a_q), np.ascontiguousarray(experts_q)
    ids = np.ascontiguousarray(ids, np.int32)
    n_expert = experts_q.size // (n * (k // 256) * BLOCK_BYTES[wtype])
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
        if w_stride is None:
            w_stride = weights.size // t if t else n_used
    c = np.empty((t, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_down_cpu(_p(a_q), _p(experts_q), n_expert, _p(ids), ids_stride,
                                         None if weights is None else _p(weights), w_stride or n_used, _p(c), n, t, n_used,
                                         n, k, wtype, threads), "gemm_w4a8_moe_down_cpu")
    return c


def _bias(b: np.ndarray | None, n_expert: int, n: int, what: str):
    """A bias of the _bias twins: None, or float32 [n_expert, >= n] -> (array or None, its row stride)."""
    if b is None:
        return None, 0
    b = np.ascontiguousarray(b, np.float32)
    if b.ndim != 2 or b.shape[0] != n_expert or b.shape[1] < n:
        raise RuntimeError(f"{what}: a bias must be [n_expert, >= n]")
    return b, b.shape[1]


def gemm_w4a8_moe_bias(a_q: np.ndarray, experts_q: np.ndarray, bias: np.ndarray | None, ids: np.ndarray, t: int,
                       n_used: int, n: int, k: int, wtype: int = 39, a_rows: int = 1, threads: int = 1,
                       ids_stride: int | None = None) -> np.ndarray:
    """C[t, n_used, n] of qg_gemm_w4a8_moe_bias_cpu: ``gemm_w4a8_moe`` for Q4_K / Q6_K / MXFP4 experts, then the expert's
    bias row (float32 [n_expert, >= n], or None: no add) added to every slot with a valid id."""
    a_q, experts_q = np.ascontiguousarray(a_q), np.ascontiguousarray(experts_q)
    ids = np.ascontiguousarray(ids, np.int32)
    n_expert = experts_q.size // (n * (k // (32 if wtype == 39 else 256)) * BLOCK_BYTES[wtype])
    b, sb = _bias(bias, n_expert, n, "gemm_w4a8_moe_bias_cpu")
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    c = np.empty((t, n_used, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_bias_cpu(_p(a_q), a_rows, _p(experts_q), None if b is None else _p(b), sb, n_expert, _p(ids),
                                         ids_stride, _p(c), n, t, n_used, n, k, wtype, threads), "gemm_w4a8_moe_bias_cpu")
    return c


def gemm_w4a8_moe_glu_bias(a_q: np.ndarray, gate_q: np.ndarray, up_q: np.ndarray, bias_gate: np.ndarray | None,
                           bias_up: np.ndarray | None, ids: np.ndarray, t: int, n_used: int, n: int, k: int,
                           wtype: int = 39, glu_op: int = GLU_SWIGLU_OAI, alpha: float = 1.702, limit: float = 7.0,
                           threads: int = 1, ids_stride: int | None = None) -> np.ndarray:
    """C[t, n_used, n] of qg_gemm_w4a8_moe_glu_bias_cpu: ``gemm_w4a8_moe_glu`` with the per-expert bias rows
    (float32 [n_expert, >= n] of one row length, or None) added to g and to u ahead of the op, GLU_SWIGLU_OAI among the
    ops, and Q4_K / Q6_K / MXFP4 experts."""
    a_q, gate_q, up_q = np.ascontiguousarray(a_q), np.ascontiguousarray(gate_q), np.ascontiguousarray(up_q)
    ids = np.ascontiguousarray(ids, np.int32)
    if gate_q.size != up_q.size:
        raise RuntimeError("gemm_w4a8_moe_glu_bias_cpu: gate and up experts differ in size")
    n_expert = gate_q.size // (n * (k // (32 if wtype == 39 else 256)) * BLOCK_BYTES[wtype])
    bg, sg = _bias(bias_gate, n_expert, n, "gemm_w4a8_moe_glu_bias_cpu")
    bu, su = _bias(bias_up, n_expert, n, "gemm_w4a8_moe_glu_bias_cpu")
    if bg is not None and bu is not None and sg != su:
        raise RuntimeError("gemm_w4a8_moe_glu_bias_cpu: the two biases differ in row length")
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    c = np.empty((t, n_used, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_glu_bias_cpu(_p(a_q), _p(gate_q), _p(up_q), None if bg is None else _p(bg),
                                             None if bu is None else _p(bu), sg or su, n_expert, _p(ids), ids_stride, _p(c),
                                             n, t, n_used, n, k, wtype, glu_op, alpha, limit, threads),
        "gemm_w4a8_moe_glu_bias_cpu")
    return c


def gemm_w4a8_moe_down_bias(a_q: np.ndarray, experts_q: np.ndarray, bias: np.ndarray | None, ids: np.ndarray,
                            weights: np.ndarray | None, t: int, n_used: int, n: int, k: int, wtype: int = 39,
                            threads: int = 1, ids_stride: int | None = None, w_stride: int | None = None) -> np.ndarray:
    """C[t, n] of qg_gemm_w4a8_moe_down_bias_cpu: ``gemm_w4a8_moe_down`` with the per-expert bias row (float32
    [n_expert, >= n], or None) added to every product ahead of the fold, and Q4_K / Q6_K / MXFP4 experts."""
    a_q, experts_q = np.ascontiguousarray(a_q), np.ascontiguousarray(experts_q)
    ids = np.ascontiguousarray(ids, np.int32)
    n_expert = experts_q.size // (n * (k // (32 if wtype == 39 else 256)) * BLOCK_BYTES[wtype])
    b, sb = _bias(bias, n_expert, n, "gemm_w4a8_moe_down_bias_cpu")
    if ids_stride is None:
        ids_stride = ids.size // t if t else n_used
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
        if w_stride is None:
            w_stride = weights.size // t if t else n_used
    c = np.empty((t, n), np.float32)
    _ok(load().qg_gemm_w4a8_moe_down_bias_cpu(_p(a_q), _p(experts_q), None if b is None else _p(b), sb, n_expert, _p(ids),
                                              ids_stride, None if weights is None else _p(weights), w_stride or n_used,
                                              _p(c), n, t, n_used, n, k, wtype, threads), "gemm_w4a8_moe_down_bias_cpu")
    return c


def gemm_fp32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    c = np.empty((a.shape[0], b.shape[0]), np.float32)
    _ok(load().qg_gemm_fp32_cpu(_p(a), _p(b), _p(c), a.shape[0], b.shape[0], a.shape[1]), "gemm_fp32_cpu")
    return c
