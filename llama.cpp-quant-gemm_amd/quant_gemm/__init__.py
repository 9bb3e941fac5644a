"""quant_gemm — MI355X (gfx950) W4A8 quantized GEMM, drop-in for the reference's Python face.

Same names, argument meaning, tensor layouts and error behaviour as the reference package
(python/quant_gemm/__init__.py:33-89, python/quant_gemm/csrc/bindings.cpp:19-91):

    weight_q     = quant_gemm.quantize_q4_0(weight)        # f32 [..., K] -> u8 [..., K/32, 18]
    activation_q = quant_gemm.quantize_q8_1(activation)    # f32 [..., K] -> u8 [..., K/32, 36]
    out = quant_gemm.gemm_q4_0_q8_1(weight_q, activation_q, M, N, K)   # f32 [M, N] (weight-major)
    x   = quant_gemm.dequantize_q4_0(weight_q, K)

Differences, all deliberate: kernels run on torch's *current* HIP stream (the reference launches
on the legacy default stream, gemm_ops.cu:250); validation errors raise RuntimeError like
TORCH_CHECK does. Extra entry points expose the rest of the C-ABI: the activation-major
``gemm_w4a8`` (include/gemm_reference.h convention), Q4_1/Q5_0/Q5_1, Q4_K, Q6_K and MXFP4 weights, every quantizer and
the per-block ``debug_sumi`` parity hook. Every call goes to HIP kernels in ``libqg_hip.so``;
there is no CPU path.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

__version__ = "0.1.0"

QK4_0 = 32
QK8_1 = 32
BLOCK_Q4_0_BYTES = 18
BLOCK_Q8_1_BYTES = 36

# ggml_type ids (compat/ggml_types.h:199-215)
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q8_1 = 2, 3, 6, 7, 8, 9
Q4_K = 12  # 256-element super-blocks of 144 bytes (qg.h "Q4_K weights")
Q6_K = 14  # 256-element super-blocks of 210 bytes (qg.h "Q6_K weights")
MXFP4 = 39  # 32-element blocks of 17 bytes: an E8M0 scale byte and E2M1 codes (qg.h "MXFP4 weights")
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q8_1: 36, Q4_K: 144, Q6_K: 210, MXFP4: 17}
GLU_REGLU, GLU_SWIGLU = 0, 2  # QG_GLU_* (numbered as ggml_glu_op): the ops of gemm_w4a8_moe_glu
GLU_SWIGLU_OAI = 3  # gpt-oss's clamped SwiGLU: gemm_w4a8_moe_glu_bias alone
ALGO_AUTO, ALGO_GEMV, ALGO_MFMA, ALGO_GENERIC, ALGO_RAGGED = 0, 1, 2, 3, 4
WEIGHT_TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
# what gemm_w4a8 / gemm_w4a8_f32 / debug_sumi take; the layout entries (tiled, repacked, grouped, batched) keep
# WEIGHT_TYPES
GEMM_WEIGHT_TYPES = WEIGHT_TYPES + (Q4_K, Q6_K, MXFP4)


def block_elems(qtype: int) -> int:
    """Elements per block of a type (qg_block_elems): 32, or 256 for Q4_K / Q6_K; 0 if unknown."""
    return _lib.load().qg_block_elems(qtype)


def _require(cond: bool, msg: str) -> None:
    if not cond:
        raise RuntimeError(msg)


def _stream(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------- quantizers
def quantize(x: torch.Tensor, qtype: int, variant: int = 0) -> torch.Tensor:
    """FP32 [..., K] -> uint8 [..., K/32, block_bytes(qtype)], bytes identical to the reference
    CPU quantizers (include/quantize.h; tests/framework/test_framework.cuh for Q4_1/Q5_x and
    Q8_1 variant 1)."""
    _require(x.is_cuda, "Input must be a CUDA tensor")
    _require(x.dtype == torch.float32, "Input must be float32")
    _require(x.dim() >= 1, "Input must have at least 1 dimension")
    K = x.size(-1)
    _require(K % 32 == 0, f"Last dimension must be divisible by 32, got {K}")
    _require(qtype in BLOCK_BYTES and qtype not in (Q4_K, Q6_K, MXFP4), f"unknown quant type {qtype}")
    x = x.contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (K // 32, BLOCK_BYTES[qtype]), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().qg_quantize(qtype, variant, _ptr(x), _ptr(out), x.numel(), _stream(x.device)),
                   "quantize")
    return out


def quantize_q4_0(x: torch.Tensor) -> torch.Tensor:
    """Quantize FP32 tensor to Q4_0: [..., K] -> uint8 [..., K//32, 18]."""
    return quantize(x, Q4_0)


def quantize_q8_1(x: torch.Tensor) -> torch.Tensor:
    """Quantize FP32 tensor to Q8_1: [..., K] -> uint8 [..., K//32, 36]."""
    return quantize(x, Q8_1)


def dequantize(x_q: torch.Tensor, qtype: int) -> torch.Tensor:
    _require(x_q.is_cuda, "Input must be a CUDA tensor")
    _require(x_q.dtype == torch.uint8, "Input must be uint8")
    _require(qtype in BLOCK_BYTES, f"unknown quant type {qtype}")
    bb = BLOCK_BYTES[qtype]
    _require(x_q.numel() % bb == 0, f"Input size {x_q.numel()} is not a multiple of {bb}-byte blocks")
    x_q = x_q.contiguous()
    nblocks = x_q.numel() // bb
    be = block_elems(qtype)
    shape = tuple(x_q.shape[:-2]) + (x_q.shape[-2] * be,) if x_q.dim() >= 2 else (nblocks * be,)
    out = torch.empty(shape, dtype=torch.float32, device=x_q.device)
    with torch.cuda.device(x_q.device):
        _lib.check(_lib.load().qg_dequantize(qtype, _ptr(x_q), _ptr(out), nblocks * be, _stream(x_q.device)),
                   "dequantize")
    return out


def dequantize_q4_0(x_q: torch.Tensor, K: int) -> torch.Tensor:
    """Dequantize Q4_0 [..., K//32, 18] back to FP32 [..., K]."""
    _require(x_q.is_cuda, "Input must be a CUDA tensor")
    _require(x_q.dtype == torch.uint8, "Input must be uint8")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    out = dequantize(x_q, Q4_0)
    return out.reshape(tuple(x_q.shape[:-2]) + (K,))


# ---------------------------------------------------------------------------- GEMMs
def _check_blocks(t: torch.Tensor, what: str, rows: int, K: int, bb: int, be: int = 32) -> None:
    """rows x K elements in blocks of be elements and bb bytes (be = block_elems(type): 256 for Q4_K)."""
    _require(t.is_cuda, f"{what} must be a CUDA tensor")
    _require(t.dtype == torch.uint8, f"{what} must be uint8")
    expect = rows * (K // be) * bb
    _require(t.numel() == expect, f"{what} shape mismatch: expected {expect} elements, got {t.numel()}")


def _check_layout(t: torch.Tensor, what: str, nbytes: int, device) -> None:
    """A load-time layout buffer (tiled / packed weights, tiled activations) handed to the C-ABI as a raw
    pointer: the exact byte count, uint8, contiguous, on the product's device (a strided view
    or a non-uint8 tensor of matching numel would otherwise be read as the wrong bytes)."""
    _require(t.dtype == torch.uint8, f"{what} must be a uint8 tensor, got {t.dtype}")
    _require(t.is_contiguous(), f"{what} must be contiguous")
    _require(t.is_cuda and t.device == device, f"{what} must be on {device}, got {t.device}")
    _require(t.numel() == nbytes, f"{what} shape mismatch: expected {nbytes} bytes, got {t.numel()}")


def gemm_w4a8(activation_q: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int,
              wtype: int = Q4_0, algo: int = ALGO_AUTO, out: torch.Tensor | None = None) -> torch.Tensor:
    """Activation-major C[M, N] = A_q8_1[M, K] . B_w[N, K]^T (include/gemm_reference.h:175-222;
    include/llama_adapter.h). M = tokens, N = weight rows.

    ``out``: optional float32 [M, N] destination; its rows may be strided (``out.stride(1) == 1``,
    ``out.stride(0) >= N``, e.g. a column slice of a wider buffer), written through
    ``qg_gemm_w4a8_ldc``."""
    _require(wtype in GEMM_WEIGHT_TYPES, f"unsupported weight type {wtype}")
    be = block_elems(wtype)
    _require(K % be == 0, f"K must be divisible by {be}, got {K}")
    _check_blocks(activation_q, "Activation", M, K, 36)
    _check_blocks(weight_q, "Weight", N, K, BLOCK_BYTES[wtype], be)
    a = activation_q.contiguous()
    w = weight_q.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    else:
        _require(out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (M, N), "bad out tensor")
        _require(out.device == w.device, "out must be on the weights' device")
        _require(M * N == 0 or out.stride(1) == 1 or N == 1, "bad out tensor: rows must be dense")
    ldc = out.stride(0) if M > 1 else N
    _require(ldc >= N, "bad out tensor: row stride below N")
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_ldc(_ptr(a), _ptr(w), _ptr(out), M, N, K, ldc, wtype, algo,
                                                _stream(w.device)), "gemm_w4a8")
    return out


def gemm_w4a8_batched(activation_q: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int,
                      wtype: int = Q4_0) -> torch.Tensor:
    """Strided batch of independent activation-major products: activation_q [B, M, K/32, 36],
    weight_q [B, N, K/32, bb] -> C [B, M, N]. One launch on the GEMV path (M <= 8)."""
    _require(activation_q.is_cuda and weight_q.is_cuda, "Inputs must be CUDA tensors")
    _require(activation_q.dtype == torch.uint8 and weight_q.dtype == torch.uint8, "Inputs must be uint8")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    B = weight_q.shape[0]
    bb = BLOCK_BYTES[wtype]
    _require(activation_q.shape[0] == B, "batch mismatch")
    _require(activation_q[0].numel() == M * (K // 32) * 36, "Activation shape mismatch")
    _require(weight_q[0].numel() == N * (K // 32) * bb, "Weight shape mismatch")
    a = activation_q.contiguous()
    w = weight_q.contiguous()
    out = torch.empty((B, M, N), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_strided_batched(
            _ptr(a), a[0].numel(), _ptr(w), w[0].numel(), _ptr(out), M * N, B, M, N, K, wtype,
            _stream(w.device)), "gemm_w4a8_batched")
    return out


class _GemvItem(ctypes.Structure):
    _fields_ = [("A_q8_1", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p),
                ("N", ctypes.c_int), ("ldc", ctypes.c_int)]


def gemm_w4a8_grouped(activations_q, weights_q, Ns, M: int, K: int, wtype: int = Q4_0, outs=None):
    """Grouped activation-major products with independent pointers and row counts
    (qg_gemm_w4a8_grouped): item i = activations_q[i] [M, K/32, 36] (items may share one tensor) x
    weights_q[i] [Ns[i], K/32, bb] -> outs[i] [M, Ns[i]] (allocated unless given; a given out may be
    a row-strided view, e.g. a column slice of a wider buffer). One launch for up to 64 items on the
    GEMV path; each output bit-identical to gemm_w4a8 on its item."""
    n = len(weights_q)
    _require(len(activations_q) == n and len(Ns) == n, "item count mismatch")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    bb = BLOCK_BYTES[wtype]
    items = (_GemvItem * max(n, 1))()
    res, keep = [], []
    dev = weights_q[0].device if n else torch.device("cuda")
    for i in range(n):
        a, w, N = activations_q[i], weights_q[i], int(Ns[i])
        _require(a.is_cuda and w.is_cuda, "Inputs must be CUDA tensors")
        _require(a.dtype == torch.uint8 and w.dtype == torch.uint8, "Inputs must be uint8")
        _require(a.numel() == M * (K // 32) * 36, "Activation shape mismatch")
        _require(w.numel() == N * (K // 32) * bb, "Weight shape mismatch")
        a, w = a.contiguous(), w.contiguous()
        if outs is None:
            o = torch.empty((M, N), dtype=torch.float32, device=w.device)
        else:
            o = outs[i]
            _require(o.dtype == torch.float32 and o.shape == (M, N) and (N <= 1 or o.stride(1) == 1),
                     "out must be float32 [M, N] with unit column stride")
        keep += [a, w]
        ldc = o.stride(0) if M > 1 else N
        items[i] = _GemvItem(a.data_ptr(), w.data_ptr(), o.data_ptr(), N, ldc)
        res.append(o)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().qg_gemm_w4a8_grouped(items, n, M, K, wtype, _stream(dev)), "gemm_w4a8_grouped")
    return res


def _moe_operands(activation_q, experts_q, ids, T: int, n_used: int, N: int, K: int, wtype: int, a_rows: int, out,
                  per_token: bool = False):
    """What the mul_mat_id wrappers check alike, after the weight type: the contiguous operands, n_expert,
    ids_stride, ``out`` (allocated unless given) and its ldc. per_token: ``out`` is [T, N], a row per token
    (gemm_w4a8_moe_down), not [T, n_used, N]."""
    be = block_elems(wtype)
    _require(K % be == 0, f"K must be divisible by {be}, got {K}")
    _require(a_rows in (1, n_used), f"a_rows must be 1 or n_used, got {a_rows}")
    _check_blocks(activation_q, "Activation", T * a_rows, K, 36)
    _require(experts_q.is_cuda and experts_q.dtype == torch.uint8, "Experts must be a CUDA uint8 tensor")
    per = N * (K // be) * BLOCK_BYTES[wtype]
    _require(per > 0 and experts_q.numel() % per == 0 and experts_q.numel() >= per,
             f"Experts shape mismatch: {experts_q.numel()} bytes is no multiple of {per}")
    n_expert = experts_q.numel() // per
    _require(ids.is_cuda and ids.dtype == torch.int32 and ids.device == experts_q.device, "ids must be an int32 tensor on the experts' device")
    _require(ids.dim() == 2 and tuple(ids.shape) == (T, n_used) and (n_used <= 1 or ids.stride(1) == 1),
             "ids must be [T, n_used] with unit column stride")
    ids_stride = ids.stride(0) if T > 1 else n_used
    _require(ids_stride >= n_used, "ids row stride below n_used")
    a, w = activation_q.contiguous(), experts_q.contiguous()
    if per_token:
        if out is None:
            out = torch.empty((T, N), dtype=torch.float32, device=w.device)
        else:
            _require(out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (T, N), "bad out tensor")
            _require(out.device == w.device, "out must be on the experts' device")
            _require(N <= 1 or out.stride(1) == 1, "bad out tensor: rows must be dense")
        ldc = out.stride(0) if T > 1 else N
        _require(ldc >= N, "bad out tensor: rows overlap")
        return a, w, n_expert, ids_stride, out, ldc
    if out is None:
        out = torch.empty((T, n_used, N), dtype=torch.float32, device=w.device)
    else:
        _require(out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (T, n_used, N), "bad out tensor")
        _require(out.device == w.device, "out must be on the experts' device")
        _require(N <= 1 or out.stride(2) == 1, "bad out tensor: rows must be dense")
    ldc = out.stride(1) if n_used > 1 else out.stride(0) if T > 1 else N
    _require(ldc >= N and (T <= 1 or n_used <= 1 or out.stride(0) == n_used * ldc), "bad out tensor: slots must be evenly spaced")
    return a, w, n_expert, ids_stride, out, ldc


def _moe_workspace(workspace, nbytes: int, dev: torch.device) -> torch.Tensor:
    """The caller's workspace checked, or one of nbytes allocated."""
    if workspace is None:
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    _require(workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous(),
             "workspace must be a contiguous CUDA uint8 tensor")
    _require(workspace.device == dev, "workspace must be on the experts' device")
    return workspace


def _config(sym: str, *args) -> str:
    """The config line a qg_*_config symbol writes for args."""
    buf = ctypes.create_string_buffer(256)
    _lib.check(getattr(_lib.load(), sym)(*args, buf, 256), sym[3:])
    return buf.value.decode()


def gemm_w4a8_moe(activation_q: torch.Tensor, experts_q: torch.Tensor, ids: torch.Tensor, T: int, n_used: int, N: int,
                  K: int, wtype: int = Q4_0, a_rows: int = 1, out: torch.Tensor | None = None) -> torch.Tensor:
    """ggml's mul_mat_id for a decode step in ONE launch, the expert ids read on the device (qg_gemm_w4a8_moe):
    C[t, u, :] = experts_q[ids[t, u]] . activation_q[t, u % a_rows], float32 [T, n_used, N].

    ``activation_q``: Q8_1 [T, a_rows, K/32, 36], a_rows 1 (one row per token) or n_used (one per slot).
    ``experts_q``: [n_expert, N, K/bs, block bytes] of ``wtype`` (any of GEMM_WEIGHT_TYPES), dense.
    ``ids``: int32 CUDA tensor [T, n_used]; a view with a row stride is fine (``ids.stride(1) == 1``). Never copied
    to the host: a captured graph follows the ids each replay finds. An id outside [0, n_expert) gives zeros.
    ``out``: optional float32 [T, n_used, N] with ``out.stride(2) == 1``, ``out.stride(1) >= N`` floats between
    slots and ``out.stride(0) == n_used * out.stride(1)``.
    Each slot is bit-identical to ``gemm_w4a8`` on its row and expert. Shapes the expert-indexed GEMV does not
    serve (odd K/32, more than 65535 slots, ...) raise."""
    _require(wtype in GEMM_WEIGHT_TYPES, f"unsupported weight type {wtype}")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, a_rows, out)
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe(_ptr(a), a_rows, _ptr(w), n_expert, _ptr(ids), ids_stride, _ptr(out), ldc,
                                                T, n_used, N, K, wtype, _stream(w.device)), "gemm_w4a8_moe")
    return out


def moe_config(T: int, n_used: int, N: int, K: int, wtype: int = Q4_0) -> str:
    """The kernel ``gemm_w4a8_moe`` launches for this shape ("moe:<family> ..." with the family and the LPR / BPL /
    ONE(U) of ``debug_config(1, N, K, wtype)``); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_config", T, n_used, N, K, wtype)


def moe_prefill_workspace_size(T: int, n_used: int, n_expert: int) -> int:
    """Bytes of the workspace ``gemm_w4a8_moe_prefill`` needs (qg_gemm_w4a8_moe_prefill_workspace_size)."""
    return int(_lib.load().qg_gemm_w4a8_moe_prefill_workspace_size(T, n_used, n_expert))


def gemm_w4a8_moe_prefill(activation_q: torch.Tensor, experts_q: torch.Tensor, ids: torch.Tensor, T: int, n_used: int,
                          N: int, K: int, wtype: int = Q4_K, a_rows: int = 1, workspace: torch.Tensor | None = None,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """ggml's mul_mat_id at prompt sizes (qg_gemm_w4a8_moe_prefill): the slots are sorted by expert id on the device and
    every expert's rows go through the Q4_K / Q6_K MFMA prefill in tiles, so an expert's matrix is read once per tile
    of slots, not once per slot. The operands, the result and ``out`` are those of ``gemm_w4a8_moe``; ``wtype`` is
    Q4_K or Q6_K.

    ``workspace``: a contiguous CUDA uint8 tensor of ``moe_prefill_workspace_size(T, n_used, n_expert)`` bytes or more,
    16-B aligned, its content arbitrary; allocated here when None. Calls on one stream may share one.
    The ids are never copied to the host: a captured graph follows the ids each replay finds."""
    _require(wtype in (Q4_K, Q6_K), f"unsupported weight type {wtype}: the expert-grouped prefill takes Q4_K and Q6_K")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, a_rows, out)
    workspace = _moe_workspace(workspace, moe_prefill_workspace_size(T, n_used, n_expert), w.device)
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_prefill(_ptr(a), a_rows, _ptr(w), n_expert, _ptr(ids), ids_stride, _ptr(out),
                                                        ldc, T, n_used, N, K, wtype, _ptr(workspace), workspace.numel(),
                                                        _stream(w.device)), "gemm_w4a8_moe_prefill")
    return out


def moe_prefill_config(T: int, n_used: int, n_expert: int, N: int, K: int, wtype: int = Q4_K) -> str:
    """The launch ``gemm_w4a8_moe_prefill`` makes for this shape ("moe:q4k_mmq TT=.. RG=.. KS=.. R=.. grid=XxY", Y the
    host's upper bound on the tiles); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_prefill_config", T, n_used, n_expert, N, K, wtype)


def debug_moe_prefill_plan(ids: torch.Tensor, n_expert: int, N: int, K: int, wtype: int = Q4_K, a_rows: int = 1,
                           workspace: torch.Tensor | None = None):
    """The plan of ``gemm_w4a8_moe_prefill`` alone (qg_debug_moe_prefill_plan; for tests): int32 counts [n_expert + 1]
    (the last: ids that name no expert) and the T * n_used slots in expert order (those of the invalid bin last)."""
    _require(ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2, "ids must be a CUDA int32 [T, n_used] tensor")
    T, n_used = ids.shape
    _require(n_used <= 1 or ids.stride(1) == 1, "ids must have unit column stride")
    ids_stride = ids.stride(0) if T > 1 else n_used
    if workspace is None:
        workspace = torch.empty(max(moe_prefill_workspace_size(T, n_used, n_expert), 16), dtype=torch.uint8, device=ids.device)
    counts = torch.empty(n_expert + 1, dtype=torch.int32, device=ids.device)
    order = torch.empty(T * n_used, dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.load().qg_debug_moe_prefill_plan(_ptr(ids), ids_stride, T, n_used, n_expert, a_rows, N, K, wtype,
                                                         _ptr(counts), _ptr(order), _ptr(workspace), workspace.numel(),
                                                         _stream(ids.device)), "debug_moe_prefill_plan")
    return counts, order


def moe_batch_workspace_size(T: int, n_used: int, n_expert: int) -> int:
    """Bytes of the workspace ``gemm_w4a8_moe_batch`` needs (qg_gemm_w4a8_moe_batch_workspace_size)."""
    return int(_lib.load().qg_gemm_w4a8_moe_batch_workspace_size(T, n_used, n_expert))


def gemm_w4a8_moe_batch(activation_q: torch.Tensor, experts_q: torch.Tensor, ids: torch.Tensor, T: int, n_used: int,
                        N: int, K: int, wtype: int = Q4_K, a_rows: int = 1, workspace: torch.Tensor | None = None,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """ggml's mul_mat_id for batched decode (qg_gemm_w4a8_moe_batch): the slots are sorted by expert id on the device
    and every expert's rows go through the Q4_K / Q6_K decode GEMV in tiles of 2, 4 or 8, so tokens that chose the same
    expert share one pass over its matrix. The operands, the result and ``out`` are those of ``gemm_w4a8_moe``, and every
    slot is bit-identical to it; ``wtype`` is Q4_K or Q6_K.

    ``workspace``: a contiguous CUDA uint8 tensor of ``moe_batch_workspace_size(T, n_used, n_expert)`` bytes or more,
    16-B aligned, its content arbitrary; allocated here when None. Calls on one stream may share one.
    The ids are never copied to the host: a captured graph follows the ids each replay finds."""
    _require(wtype in (Q4_K, Q6_K), f"unsupported weight type {wtype}: the expert-grouped decode GEMV takes Q4_K and Q6_K")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, a_rows, out)
    workspace = _moe_workspace(workspace, moe_batch_workspace_size(T, n_used, n_expert), w.device)
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_batch(_ptr(a), a_rows, _ptr(w), n_expert, _ptr(ids), ids_stride, _ptr(out),
                                                      ldc, T, n_used, N, K, wtype, _ptr(workspace), workspace.numel(),
                                                      _stream(w.device)), "gemm_w4a8_moe_batch")
    return out


def moe_batch_config(T: int, n_used: int, n_expert: int, N: int, K: int, wtype: int = Q4_K) -> str:
    """The launch ``gemm_w4a8_moe_batch`` makes for this shape ("moeb:q4k_gemv R=.. LPR=.. WGS=.. ONE=.. grid=XxY lds=..",
    R the rows per tile, Y the host's upper bound on the tiles); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_batch_config", T, n_used, n_expert, N, K, wtype)


def gemm_w4a8_moe_glu(activation_q: torch.Tensor, gate_q: torch.Tensor, up_q: torch.Tensor, ids: torch.Tensor, T: int,
                      n_used: int, N: int, K: int, wtype: int = Q4_K, glu_op: int = GLU_SWIGLU,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """The first half of an MoE FFN block in ONE launch (qg_gemm_w4a8_moe_glu): C[t, u, :] = glu_op(g) * u with
    g = gate_q[ids[t, u]] . activation_q[t] and u = up_q[ids[t, u]] . activation_q[t], float32 [T, n_used, N]. It
    replaces two ``gemm_w4a8_moe`` calls and the activation kernel between them and the down product.

    ``activation_q``: Q8_1 [T, K/32, 36], one row per token. ``gate_q``, ``up_q``: [n_expert, N, K/256, block bytes]
    of ``wtype``, Q4_K or Q6_K, dense, of one size; they may be the same tensor. ``ids`` and ``out``: as ``gemm_w4a8_moe``.
    ``glu_op``: GLU_SWIGLU, (g / (1 + expf(-g))) * u, or GLU_REGLU, max(g, 0) * u. g and u have the bits ``gemm_w4a8_moe``
    gives on either tensor. Shapes the decode GEMV does not serve raise."""
    _require(wtype in (Q4_K, Q6_K), f"unsupported weight type {wtype}: the fused gate / up entry takes Q4_K and Q6_K")
    _require(glu_op in (GLU_REGLU, GLU_SWIGLU), f"unsupported glu_op {glu_op}")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, gate_q, ids, T, n_used, N, K, wtype, 1, out)
    _require(up_q.is_cuda and up_q.dtype == torch.uint8 and up_q.device == w.device and up_q.numel() == w.numel(),
             "Up experts must be a CUDA uint8 tensor of the gate experts' size, on their device")
    up = up_q.contiguous()
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_glu(_ptr(a), _ptr(w), _ptr(up), n_expert, _ptr(ids), ids_stride, _ptr(out),
                                                    ldc, T, n_used, N, K, wtype, glu_op, _stream(w.device)),
                   "gemm_w4a8_moe_glu")
    return out


def moe_glu_config(T: int, n_used: int, N: int, K: int, wtype: int = Q4_K) -> str:
    """The launch ``gemm_w4a8_moe_glu`` makes for this shape ("moe_glu:q4k_gemv LPR=.. WGS=.. ONE=.. grid=XxY lds=..", the
    LPR / WGS / ONE of ``moe_config``); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_glu_config", T, n_used, N, K, wtype)


def gemm_w4a8_moe_down(activation_q: torch.Tensor, experts_q: torch.Tensor, ids: torch.Tensor,
                       weights: torch.Tensor | None, T: int, n_used: int, N: int, K: int, wtype: int = Q4_K,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """The second half of an MoE FFN block in ONE launch (qg_gemm_w4a8_moe_down): C[t, :] = sum over u, in ascending
    order, of weights[t, u] * (experts_q[ids[t, u]] . activation_q[t, u]), float32 [T, N]. It replaces ``gemm_w4a8_moe``
    at ``a_rows = n_used``, the multiply by the router weights and the sum over the token's experts.

    ``activation_q``: Q8_1 [T, n_used, K/32, 36], one row per slot. ``experts_q``: [n_expert, N, K/256, block bytes] of
    ``wtype``, Q4_K or Q6_K, dense. ``ids``: as ``gemm_w4a8_moe``; a slot whose id is outside [0, n_expert) contributes
    nothing and its weight is not read. ``weights``: float32 CUDA tensor [T, n_used] (a view with a row stride is fine,
    ``weights.stride(1) == 1``), or None for the plain sum (every weight 1). Neither ids nor weights is copied to the
    host: a captured graph follows what each replay finds. ``out``: optional float32 [T, N] with ``out.stride(1) == 1``
    and ``out.stride(0) >= N``. Every product has the bits ``gemm_w4a8_moe`` gives the slot; the fold is one rounded
    fp32 multiplication and addition per slot. Shapes the entry does not serve raise."""
    _require(wtype in (Q4_K, Q6_K), f"unsupported weight type {wtype}: the down entry with the expert sum takes Q4_K and Q6_K")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, n_used, out,
                                                        per_token=True)
    w_stride = n_used
    if weights is not None:
        _require(weights.is_cuda and weights.dtype == torch.float32 and weights.device == w.device,
                 "weights must be a float32 tensor on the experts' device")
        _require(weights.dim() == 2 and tuple(weights.shape) == (T, n_used) and (n_used <= 1 or weights.stride(1) == 1),
                 "weights must be [T, n_used] with unit column stride")
        w_stride = weights.stride(0) if T > 1 else n_used
        _require(w_stride >= n_used, "weights row stride below n_used")
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_down(_ptr(a), _ptr(w), n_expert, _ptr(ids), ids_stride,
                                                     None if weights is None else _ptr(weights), w_stride, _ptr(out), ldc,
                                                     T, n_used, N, K, wtype, _stream(w.device)), "gemm_w4a8_moe_down")
    return out


def moe_down_config(T: int, n_used: int, N: int, K: int, wtype: int = Q4_K) -> str:
    """The launch ``gemm_w4a8_moe_down`` makes for this shape ("moe_down:q4k_gemv LPR=.. WGS=.. ONE=.. SW=.. grid=XxY
    lds=..", the LPR / WGS / ONE of ``moe_config``, SW waves side by side on the slots of a row group, Y = T); nothing
    is launched. Raises where the shape is not served."""
    return _config("qg_moe_down_config", T, n_used, N, K, wtype)


def _moe_bias(bias, n_expert: int, N: int, device, what: str):
    """A bias of the two _bias entries: None, or float32 [n_expert, N] on the experts' device with unit column stride
    (a view with a row stride is fine) -> (tensor or None, its row stride; 0: none)."""
    if bias is None:
        return None, 0
    _require(bias.is_cuda and bias.dtype == torch.float32 and bias.device == device,
             f"{what} must be a float32 tensor on the experts' device")
    _require(bias.dim() == 2 and tuple(bias.shape) == (n_expert, N) and (N <= 1 or bias.stride(1) == 1),
             f"{what} must be [n_expert, N] with unit column stride")
    stride = bias.stride(0) if n_expert > 1 else N
    _require(stride >= N, f"{what}: row stride below N")
    return bias, stride


def gemm_w4a8_moe_glu_bias(activation_q: torch.Tensor, gate_q: torch.Tensor, up_q: torch.Tensor,
                           bias_gate: torch.Tensor | None, bias_up: torch.Tensor | None, ids: torch.Tensor, T: int,
                           n_used: int, N: int, K: int, wtype: int = MXFP4, glu_op: int = GLU_SWIGLU_OAI,
                           alpha: float = 1.702, limit: float = 7.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gemm_w4a8_moe_glu`` with per-expert biases and gpt-oss's clamped SwiGLU, for Q4_K / Q6_K / MXFP4 experts, in ONE
    launch (qg_gemm_w4a8_moe_glu_bias): g = gate product + bias_gate[e], u = up product + bias_up[e], then ``glu_op``.

    ``gate_q``, ``up_q``: [n_expert, N, K/32, 17] for MXFP4 (at any byte address), as ``gemm_w4a8_moe_glu`` otherwise.
    ``bias_gate``, ``bias_up``: float32 [n_expert, N] CUDA tensors of one row stride (``stride(1) == 1``), or None: no
    add. ``glu_op``: GLU_REGLU, GLU_SWIGLU, or GLU_SWIGLU_OAI, with x = min(g, limit), y = clamp(u, -limit, limit):
    (x / (1 + expf(alpha * -x))) * (y + 1); ``alpha`` and ``limit`` are read for it alone. A slot whose id is outside
    [0, n_expert) gets zeros, no bias applied."""
    _require(wtype in (Q4_K, Q6_K, MXFP4), f"unsupported weight type {wtype}: the biased gate / up entry takes Q4_K, Q6_K and MXFP4")
    _require(glu_op in (GLU_REGLU, GLU_SWIGLU, GLU_SWIGLU_OAI), f"unsupported glu_op {glu_op}")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, gate_q, ids, T, n_used, N, K, wtype, 1, out)
    _require(up_q.is_cuda and up_q.dtype == torch.uint8 and up_q.device == w.device and up_q.numel() == w.numel(),
             "Up experts must be a CUDA uint8 tensor of the gate experts' size, on their device")
    up = up_q.contiguous()
    bg, sg = _moe_bias(bias_gate, n_expert, N, w.device, "bias_gate")
    bu, su = _moe_bias(bias_up, n_expert, N, w.device, "bias_up")
    _require(bg is None or bu is None or sg == su, "bias_gate and bias_up must have one row stride")
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_glu_bias(_ptr(a), _ptr(w), _ptr(up), None if bg is None else _ptr(bg),
                                                         None if bu is None else _ptr(bu), sg or su, n_expert, _ptr(ids),
                                                         ids_stride, _ptr(out), ldc, T, n_used, N, K, wtype, glu_op, alpha,
                                                         limit, _stream(w.device)), "gemm_w4a8_moe_glu_bias")
    return out


def moe_glu_bias_config(T: int, n_used: int, N: int, K: int, wtype: int = MXFP4) -> str:
    """The launch ``gemm_w4a8_moe_glu_bias`` makes for this shape ("moe_glu:mxfp4_gemv LPR=.. WGS=.. ONE=.. grid=XxY
    lds=..", ``moe_glu_config``'s string for Q4_K / Q6_K); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_glu_bias_config", T, n_used, N, K, wtype)


def gemm_w4a8_moe_down_bias(activation_q: torch.Tensor, experts_q: torch.Tensor, bias: torch.Tensor | None,
                            ids: torch.Tensor, weights: torch.Tensor | None, T: int, n_used: int, N: int, K: int,
                            wtype: int = MXFP4, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gemm_w4a8_moe_down`` with a per-expert bias, for Q4_K / Q6_K / MXFP4 experts, in ONE launch
    (qg_gemm_w4a8_moe_down_bias): C[t, :] = sum over u of weights[t, u] * (product of slot (t, u) + bias[ids[t, u]]).

    ``bias``: float32 [n_expert, N] CUDA tensor (``stride(1) == 1``), or None: no add. Everything else as
    ``gemm_w4a8_moe_down``; a slot whose id is outside [0, n_expert) contributes nothing, its bias and weight unread."""
    _require(wtype in (Q4_K, Q6_K, MXFP4), f"unsupported weight type {wtype}: the biased down entry takes Q4_K, Q6_K and MXFP4")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, n_used, out,
                                                        per_token=True)
    b, b_stride = _moe_bias(bias, n_expert, N, w.device, "bias")
    w_stride = n_used
    if weights is not None:
        _require(weights.is_cuda and weights.dtype == torch.float32 and weights.device == w.device,
                 "weights must be a float32 tensor on the experts' device")
        _require(weights.dim() == 2 and tuple(weights.shape) == (T, n_used) and (n_used <= 1 or weights.stride(1) == 1),
                 "weights must be [T, n_used] with unit column stride")
        w_stride = weights.stride(0) if T > 1 else n_used
        _require(w_stride >= n_used, "weights row stride below n_used")
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_moe_down_bias(_ptr(a), _ptr(w), None if b is None else _ptr(b), b_stride, n_expert,
                                                          _ptr(ids), ids_stride, None if weights is None else _ptr(weights),
                                                          w_stride, _ptr(out), ldc, T, n_used, N, K, wtype,
                                                          _stream(w.device)), "gemm_w4a8_moe_down_bias")
    return out


def moe_down_bias_config(T: int, n_used: int, N: int, K: int, wtype: int = MXFP4) -> str:
    """The launch ``gemm_w4a8_moe_down_bias`` makes for this shape ("moe_down:mxfp4_gemv LPR=.. WGS=.. ONE=.. SW=..
    grid=XxY lds=..", ``moe_down_config``'s string for Q4_K / Q6_K); nothing is launched. Raises where the shape is not
    served."""
    return _config("qg_moe_down_bias_config", T, n_used, N, K, wtype)


def _moe_grouped_bias(sym: str, size_fn, activation_q, experts_q, bias, ids, T, n_used, N, K, wtype, a_rows, workspace, out):
    """The call of the two expert-grouped _bias entries, which take the same arguments."""
    _require(wtype in (Q4_K, Q6_K, MXFP4), f"unsupported weight type {wtype}: the entry takes Q4_K, Q6_K and MXFP4")
    a, w, n_expert, ids_stride, out, ldc = _moe_operands(activation_q, experts_q, ids, T, n_used, N, K, wtype, a_rows, out)
    b, b_stride = _moe_bias(bias, n_expert, N, w.device, "bias")
    workspace = _moe_workspace(workspace, size_fn(T, n_used, n_expert), w.device)
    with torch.cuda.device(w.device):
        _lib.check(getattr(_lib.load(), sym)(_ptr(a), a_rows, _ptr(w), None if b is None else _ptr(b), b_stride, n_expert,
                                             _ptr(ids), ids_stride, _ptr(out), ldc, T, n_used, N, K, wtype, _ptr(workspace),
                                             workspace.numel(), _stream(w.device)), sym[3:])
    return out


def gemm_w4a8_moe_prefill_bias(activation_q: torch.Tensor, experts_q: torch.Tensor, bias: torch.Tensor | None,
                               ids: torch.Tensor, T: int, n_used: int, N: int, K: int, wtype: int = MXFP4, a_rows: int = 1,
                               workspace: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gemm_w4a8_moe_prefill`` with a per-expert bias (ggml's add_id) added to the finished product, for Q4_K / Q6_K /
    MXFP4 experts (qg_gemm_w4a8_moe_prefill_bias): C[t, u, :] = experts_q[e] . activation_q[t, u % a_rows] + bias[e],
    e = ids[t, u].

    ``experts_q``: [n_expert, N, K/32, 17] for MXFP4 (at any byte address), as ``gemm_w4a8_moe_prefill`` otherwise.
    ``bias``: float32 [n_expert, N] CUDA tensor (``stride(1) == 1``; a view with a row stride is fine), or None: no add.
    A slot whose id is outside [0, n_expert) gets zeros, no bias applied. ``workspace``: as ``gemm_w4a8_moe_prefill``
    (``moe_prefill_workspace_size``)."""
    return _moe_grouped_bias("qg_gemm_w4a8_moe_prefill_bias", moe_prefill_workspace_size, activation_q, experts_q, bias, ids,
                             T, n_used, N, K, wtype, a_rows, workspace, out)


def moe_prefill_bias_config(T: int, n_used: int, n_expert: int, N: int, K: int, wtype: int = MXFP4) -> str:
    """The launch ``gemm_w4a8_moe_prefill_bias`` makes for this shape ("moe:mxfp4_mmq TT=.. RG=.. KS=.. R=.. grid=XxY",
    ``moe_prefill_config``'s string for Q4_K / Q6_K); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_prefill_bias_config", T, n_used, n_expert, N, K, wtype)


def gemm_w4a8_moe_batch_bias(activation_q: torch.Tensor, experts_q: torch.Tensor, bias: torch.Tensor | None,
                             ids: torch.Tensor, T: int, n_used: int, N: int, K: int, wtype: int = MXFP4, a_rows: int = 1,
                             workspace: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """``gemm_w4a8_moe_batch`` with a per-expert bias (ggml's add_id) added to the finished product, for Q4_K / Q6_K /
    MXFP4 experts (qg_gemm_w4a8_moe_batch_bias). Operands as ``gemm_w4a8_moe_prefill_bias``; ``workspace``: as
    ``gemm_w4a8_moe_batch`` (``moe_batch_workspace_size``). Every product is bit-identical to ``gemm_w4a8_moe``."""
    return _moe_grouped_bias("qg_gemm_w4a8_moe_batch_bias", moe_batch_workspace_size, activation_q, experts_q, bias, ids,
                             T, n_used, N, K, wtype, a_rows, workspace, out)


def moe_batch_bias_config(T: int, n_used: int, n_expert: int, N: int, K: int, wtype: int = MXFP4) -> str:
    """The launch ``gemm_w4a8_moe_batch_bias`` makes for this shape ("moeb:mxfp4_gemv R=.. LPR=.. WGS=.. ONE=.. grid=XxY
    lds=..", ``moe_batch_config``'s string for Q4_K / Q6_K); nothing is launched. Raises where the shape is not served."""
    return _config("qg_moe_batch_bias_config", T, n_used, n_expert, N, K, wtype)


def repack_weights(weight_q: torch.Tensor, N: int, K: int, wtype: int = Q4_0) -> torch.Tensor:
    """Load-time layout for K/32 not a multiple of 8 (qg_repack_weights): [N, K'/32, bb] uint8,
    the real blocks then zero blocks (K'/32 = round_up(K/32, 8)). Feed it to gemm_w4a8_prepacked."""
    _require(weight_q.is_cuda and weight_q.dtype == torch.uint8, "weight_q must be a CUDA uint8 tensor")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    bb = BLOCK_BYTES[wtype]
    _require(weight_q.numel() == N * (K // 32) * bb, "Weight shape mismatch")
    lib = _lib.load()
    nbytes = lib.qg_repack_weights_bytes(N, K, wtype)
    out = torch.empty((N, nbytes // max(N * bb, 1), bb), dtype=torch.uint8, device=weight_q.device)
    w = weight_q.contiguous()
    with torch.cuda.device(w.device):
        _lib.check(lib.qg_repack_weights(_ptr(w), _ptr(out), N, K, wtype, _stream(w.device)), "repack_weights")
    return out


def gemm_w4a8_prepacked(activation_q: torch.Tensor, weight_packed: torch.Tensor, M: int, N: int, K: int,
                        wtype: int = Q4_0) -> torch.Tensor:
    """C [M, N] = the same product as gemm_w4a8(activation_q, weight_q, ...) from
    repack_weights(weight_q) (qg_gemm_w4a8_prepacked; K is the logical K)."""
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _check_blocks(activation_q, "Activation", M, K, 36)
    lib = _lib.load()
    _check_layout(weight_packed, "weight_packed", lib.qg_repack_weights_bytes(N, K, wtype), activation_q.device)
    a = activation_q.contiguous()
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    wsb = lib.qg_gemm_w4a8_prepacked_workspace_size(M, K)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.qg_gemm_w4a8_prepacked(_ptr(a), _ptr(weight_packed), _ptr(out), M, N, K, wtype, _ptr(ws), wsb,
                                              _stream(a.device)), "gemm_w4a8_prepacked")
    return out


def tile_weights(weight_q: torch.Tensor, N: int, K: int, wtype: int = Q4_0) -> torch.Tensor:
    """Load-time tiled layout (qg_tile_weights): 1-D uint8 of qg_tile_weights_bytes(N, K, wtype) —
    rows in tiles of 32, K/32 in stages of 4 blocks, each (tile, stage) one contiguous run in the
    prefill kernel's operand order. Feed it to gemm_w4a8_tiled."""
    _require(weight_q.is_cuda and weight_q.dtype == torch.uint8, "weight_q must be a CUDA uint8 tensor")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _require(weight_q.numel() == N * (K // 32) * BLOCK_BYTES[wtype], "Weight shape mismatch")
    lib = _lib.load()
    out = torch.empty(lib.qg_tile_weights_bytes(N, K, wtype), dtype=torch.uint8, device=weight_q.device)
    w = weight_q.contiguous()
    with torch.cuda.device(w.device):
        _lib.check(lib.qg_tile_weights(_ptr(w), _ptr(out), N, K, wtype, _stream(w.device)), "tile_weights")
    return out


def gemm_w4a8_tiled(activation_q: torch.Tensor, weight_tiled: torch.Tensor, M: int, N: int, K: int,
                    wtype: int = Q4_0, out: torch.Tensor | None = None) -> torch.Tensor:
    """C [M, N] = the same product as gemm_w4a8(activation_q, weight_q, ...) from
    tile_weights(weight_q) (qg_gemm_w4a8_tiled; any K % 32 == 0)."""
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _check_blocks(activation_q, "Activation", M, K, 36)
    lib = _lib.load()
    _check_layout(weight_tiled, "weight_tiled", lib.qg_tile_weights_bytes(N, K, wtype), activation_q.device)
    a = activation_q.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _require(out.is_cuda and out.dtype == torch.float32 and out.shape == (M, N) and out.is_contiguous(),
             "out must be a contiguous CUDA float32 [M, N] tensor")
    with torch.cuda.device(a.device):
        _lib.check(lib.qg_gemm_w4a8_tiled(_ptr(a), _ptr(weight_tiled), _ptr(out), M, N, K, wtype, _stream(a.device)),
                   "gemm_w4a8_tiled")
    return out


def quantize_q8_1_tiled(x: torch.Tensor) -> torch.Tensor:
    """FP32 [M, K] -> the tiled activation layout (qg_quantize_q8_1_tiled): 1-D uint8 of
    qg_activations_tiled_bytes(M, K) — 16-token tiles x 4-block stages, each a contiguous 2304-B run, zero
    padded. Feed it to gemm_w4a8_tiled_act."""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2, "x must be a 2-D CUDA float32 tensor")
    M, K = x.shape
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    lib = _lib.load()
    xc = x.contiguous()
    out = torch.empty(lib.qg_activations_tiled_bytes(M, K), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.qg_quantize_q8_1_tiled(_ptr(xc), _ptr(out), M, K, _stream(x.device)), "quantize_q8_1_tiled")
    return out


def tile_activations(activation_q: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """Q8_1 rows [M, K/32] -> the tiled activation layout (qg_tile_activations)."""
    _require(activation_q.is_cuda and activation_q.dtype == torch.uint8, "activation_q must be a CUDA uint8 tensor")
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _require(activation_q.numel() == M * (K // 32) * 36, "Activation shape mismatch")
    lib = _lib.load()
    a = activation_q.contiguous()
    out = torch.empty(lib.qg_activations_tiled_bytes(M, K), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.qg_tile_activations(_ptr(a), _ptr(out), M, K, _stream(a.device)), "tile_activations")
    return out


def gemm_w4a8_tiled_act(activation_tiled: torch.Tensor, weight_tiled: torch.Tensor, M: int, N: int, K: int,
                        wtype: int = Q4_0, out: torch.Tensor | None = None) -> torch.Tensor:
    """C [M, N] = gemm_w4a8_tiled's product with the activations in the tiled layout too
    (qg_gemm_w4a8_tiled_act)."""
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    lib = _lib.load()
    _require(weight_tiled.is_cuda, "weight_tiled must be a CUDA tensor")
    _check_layout(activation_tiled, "activation_tiled", lib.qg_activations_tiled_bytes(M, K), weight_tiled.device)
    _check_layout(weight_tiled, "weight_tiled", lib.qg_tile_weights_bytes(N, K, wtype), weight_tiled.device)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=weight_tiled.device)
    _require(out.is_cuda and out.dtype == torch.float32 and out.shape == (M, N) and out.is_contiguous(),
             "out must be a contiguous CUDA float32 [M, N] tensor")
    with torch.cuda.device(weight_tiled.device):
        _lib.check(lib.qg_gemm_w4a8_tiled_act(_ptr(activation_tiled), _ptr(weight_tiled), _ptr(out), M, N, K, wtype,
                                              _stream(weight_tiled.device)), "gemm_w4a8_tiled_act")
    return out


def quantize_q8_1_padded(x: torch.Tensor) -> torch.Tensor:
    """x float32 [M, K] -> uint8 [M, K'/32, 36] (qg_quantize_q8_1_padded): each row's blocks as
    quantize_q8_1, then zero blocks up to K'/32 = round_up(K/32, 8) — the activation side of the
    repack_weights layout."""
    _require(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2, "x must be a 2-D CUDA float32 tensor")
    M, K = x.shape
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    nbp = (K // 32 + 7) // 8 * 8
    x = x.contiguous()
    out = torch.empty((M, nbp, 36), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().qg_quantize_q8_1_padded(_ptr(x), _ptr(out), M, K, _stream(x.device)), "quantize_q8_1_padded")
    return out


def gemm_w4a8_padded(activation_padded: torch.Tensor, weight_packed: torch.Tensor, M: int, N: int, K: int,
                     wtype: int = Q4_0) -> torch.Tensor:
    """C [M, N] from quantize_q8_1_padded activations and repack_weights weights, one launch
    (qg_gemm_w4a8_padded; K is the logical K)."""
    _require(weight_packed.is_cuda, "weight_packed must be a CUDA tensor")
    nbp = (K // 32 + 7) // 8 * 8
    _check_layout(activation_padded.contiguous(), "activation_padded", M * nbp * 36, weight_packed.device)
    _check_layout(weight_packed, "weight_packed", N * nbp * BLOCK_BYTES[wtype], weight_packed.device)
    out = torch.empty((M, N), dtype=torch.float32, device=weight_packed.device)
    with torch.cuda.device(weight_packed.device):
        _lib.check(_lib.load().qg_gemm_w4a8_padded(_ptr(activation_padded.contiguous()), _ptr(weight_packed), _ptr(out),
                                                   M, N, K, wtype, _stream(weight_packed.device)), "gemm_w4a8_padded")
    return out


def _gemm_weight_major(sym: str, wtype: int, weight_q, activation_q, M, N, K):
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _check_blocks(weight_q, "Weight", M, K, BLOCK_BYTES[wtype])
    _check_blocks(activation_q, "Activation", N, K, 36)
    w = weight_q.contiguous()
    a = activation_q.contiguous()
    out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(getattr(_lib.load(), sym)(_ptr(w), _ptr(a), _ptr(out), M, N, K, _stream(w.device)), sym)
    return out


def gemm_q4_0_q8_1(weight_q: torch.Tensor, activation_q: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """Quantized GEMM C[M,N] = W[M,K] @ A[N,K]^T (weight-major: M = weight rows, N = tokens).

    weight_q: uint8 [M, K//32, 18]; activation_q: uint8 [N, K//32, 36]; returns f32 [M, N]."""
    return _gemm_weight_major("qg_gemm_q4_0_q8_1", Q4_0, weight_q, activation_q, M, N, K)


def gemm_q4_1_q8_1(weight_q, activation_q, M: int, N: int, K: int) -> torch.Tensor:
    return _gemm_weight_major("qg_gemm_q4_1_q8_1", Q4_1, weight_q, activation_q, M, N, K)


def gemm_q5_0_q8_1(weight_q, activation_q, M: int, N: int, K: int) -> torch.Tensor:
    return _gemm_weight_major("qg_gemm_q5_0_q8_1", Q5_0, weight_q, activation_q, M, N, K)


def gemm_q5_1_q8_1(weight_q, activation_q, M: int, N: int, K: int) -> torch.Tensor:
    return _gemm_weight_major("qg_gemm_q5_1_q8_1", Q5_1, weight_q, activation_q, M, N, K)


# ---------------------------------------------------------------------------- fused activation quantization
def _workspace(rows: int, K: int, dev: torch.device):
    nbytes = _lib.load().qg_gemm_w4a8_f32_workspace_size(rows, K)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def gemm_w4a8_f32(x: torch.Tensor, weight_q: torch.Tensor, wtype: int = Q4_0, workspace: bool = True,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Activation-major C[M, N] = Q8_1(x)[M, K] . B_w[N, K]^T for FP32 x [M, K]: identical to
    ``gemm_w4a8(quantize_q8_1(x), weight_q, ...)``. M <= 4: one launch, x quantized in the GEMV
    prologue. Larger M (or a K the GEMV does not take): through a Q8_1 workspace (``workspace=True``, from torch's caching
    allocator) or the fused GEMV per 8-row chunk (``workspace=False``)."""
    _require(x.is_cuda, "Input must be a CUDA tensor")
    _require(x.dtype == torch.float32 and x.dim() == 2, "x must be float32 [M, K]")
    M, K = x.shape
    _require(wtype in GEMM_WEIGHT_TYPES, f"unsupported weight type {wtype}")
    be = block_elems(wtype)
    _require(K % be == 0, f"K must be divisible by {be}, got {K}")
    _require(wtype not in (Q4_K, Q6_K, MXFP4) or workspace,
             "Q4_K / Q6_K / MXFP4 weights need the Q8_1 workspace (workspace=True)")
    N = weight_q.numel() // ((K // be) * BLOCK_BYTES[wtype]) if K else 0
    _check_blocks(weight_q, "Weight", N, K, BLOCK_BYTES[wtype], be)
    x = x.contiguous()
    w = weight_q.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    else:
        _require(out.is_contiguous() and out.dtype == torch.float32 and out.numel() == M * N, "bad out tensor")
    ws = _workspace(M, K, w.device) if workspace else None
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_w4a8_f32(_ptr(x), _ptr(w), _ptr(out), M, N, K, wtype,
                                                _ptr(ws) if ws is not None else None,
                                                ws.numel() if ws is not None else 0, _stream(w.device)),
                   "gemm_w4a8_f32")
    return out


def gemm_q4_0_fp16_fused(weight_q: torch.Tensor, fp16_activation: torch.Tensor, M: int, N: int, K: int,
                         workspace: bool = True) -> torch.Tensor:
    """Weight-major out[M, N] = W_q4_0[M, K] . Q8_1(act[N, K])^T with the FP16 activations quantized
    inside the product (kernels/gemm/gemm_fused.cuh:311-338 gemm_q4_0_fp16_fused; quantizer
    semantics of gemm_fused.cuh:76-143)."""
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _check_blocks(weight_q, "Weight", M, K, 18)
    _require(fp16_activation.is_cuda and fp16_activation.dtype == torch.float16, "Activation must be CUDA float16")
    _require(fp16_activation.numel() == N * K, f"Activation shape mismatch: expected {N * K} elements")
    w = weight_q.contiguous()
    a = fp16_activation.contiguous()
    out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    ws = _workspace(N, K, w.device) if workspace else None
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().qg_gemm_q4_0_fp16_fused_ws(_ptr(w), _ptr(a), _ptr(out), M, N, K,
                                                          _ptr(ws) if ws is not None else None,
                                                          ws.numel() if ws is not None else 0, _stream(w.device)),
                   "gemm_q4_0_fp16_fused")
    return out


def quantize_q8_1_f16_fused(x: torch.Tensor) -> torch.Tensor:
    """FP16 [..., K] -> Q8_1 uint8 [..., K/32, 36] with the fused kernel's quantizer semantics."""
    _require(x.is_cuda and x.dtype == torch.float16, "Input must be a CUDA float16 tensor")
    K = x.size(-1)
    _require(K % 32 == 0, f"Last dimension must be divisible by 32, got {K}")
    x = x.contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (K // 32, 36), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().qg_quantize_q8_1_f16_fused(_ptr(x), _ptr(out), x.numel(), _stream(x.device)),
                   "quantize_q8_1_f16_fused")
    return out


def gemm_q8_0_q8_1(weight_q, activation_q, M: int, N: int, K: int) -> torch.Tensor:
    """W8A8, weight-major (kernels/gemm/gemm_quant_formats.cuh:415-428)."""
    return _gemm_weight_major("qg_gemm_q8_0_q8_1", Q8_0, weight_q, activation_q, M, N, K)


def gemm_w8a8(activation_q: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """W8A8, activation-major C[M, N] = A_q8_1 . B_q8_0^T (include/gemm_reference.h:233-267)."""
    return gemm_w4a8(activation_q, weight_q, M, N, K, wtype=Q8_0)


# ---------------------------------------------------------------------------- W4A16 / W8A16
def _gemm_w16(sym: str, wtype: int, activation: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int):
    _require(K % 32 == 0, f"K must be divisible by 32, got {K}")
    _require(activation.is_cuda and activation.dtype == torch.float32, "Activation must be a CUDA float32 tensor")
    _require(activation.numel() == M * K, f"Activation shape mismatch: expected {M * K} elements")
    _check_blocks(weight_q, "Weight", N, K, BLOCK_BYTES[wtype])
    a = activation.contiguous()
    w = weight_q.contiguous()
    out = torch.empty((M, N), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(getattr(_lib.load(), sym)(_ptr(a), _ptr(w), _ptr(out), M, N, K, _stream(w.device)), sym)
    return out


def gemm_w4a16(activation: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """C[M, N] = A_f32[M, K] . dequant(W_q4_0[N, K])^T (include/gemm_reference.h:73-112)."""
    return _gemm_w16("qg_gemm_w4a16", Q4_0, activation, weight_q, M, N, K)


def gemm_w8a16(activation: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """C[M, N] = A_f32[M, K] . dequant(W_q8_0[N, K])^T (include/gemm_cuda_naive.cuh:276-283)."""
    return _gemm_w16("qg_gemm_w8a16", Q8_0, activation, weight_q, M, N, K)


def gemm_q4_0_fp32(weight_q: torch.Tensor, activation: torch.Tensor, M: int, N: int, K: int) -> torch.Tensor:
    """python/quant_gemm/csrc/gemm_ops.cu:431-466: weight_q [N, K/32, 18], activation [M, K] -> [M, N]."""
    return _gemm_w16("qg_gemm_w4a16", Q4_0, activation, weight_q, M, N, K)


def debug_sumi(activation_q: torch.Tensor, weight_q: torch.Tensor, M: int, N: int, K: int,
               wtype: int = Q4_0, algo: int = ALGO_AUTO) -> torch.Tensor:
    """Per-block int32 dots [M, N, K/32] through the same decode path as ``algo``."""
    _require(wtype in GEMM_WEIGHT_TYPES, f"unsupported weight type {wtype}")
    _check_blocks(activation_q, "Activation", M, K, 36)
    _check_blocks(weight_q, "Weight", N, K, BLOCK_BYTES[wtype], block_elems(wtype))
    out = torch.empty((M, N, K // 32), dtype=torch.int32, device=weight_q.device)
    with torch.cuda.device(weight_q.device):
        _lib.check(_lib.load().qg_debug_sumi(_ptr(activation_q.contiguous()), _ptr(weight_q.contiguous()),
                                             _ptr(out), M, N, K, wtype, algo, _stream(weight_q.device)),
                   "debug_sumi")
    return out


def debug_config(M: int, N: int, K: int, wtype: int = Q4_0, algo: int = ALGO_AUTO, sumi: bool = False) -> str:
    """The kernel instantiation ``gemm_w4a8`` (or ``debug_sumi`` with sumi=True) launches for this
    shape on aligned buffers (family, template parameters, grid); nothing is launched."""
    return _config("qg_debug_config", M, N, K, wtype, algo, int(sumi))


def debug_sumi_tiled(activation_q: torch.Tensor, weight_tiled: torch.Tensor, M: int, N: int, K: int,
                     wtype: int = Q4_0) -> torch.Tensor:
    """Per-block int32 dots [M, N, K/32] from the instantiation gemm_w4a8_tiled launches."""
    _check_blocks(activation_q, "Activation", M, K, 36)
    lib = _lib.load()
    _check_layout(weight_tiled, "weight_tiled", lib.qg_tile_weights_bytes(N, K, wtype), activation_q.device)
    out = torch.empty((M, N, K // 32), dtype=torch.int32, device=weight_tiled.device)
    with torch.cuda.device(weight_tiled.device):
        _lib.check(lib.qg_debug_sumi_tiled(_ptr(activation_q.contiguous()), _ptr(weight_tiled), _ptr(out), M, N, K, wtype,
                                           _stream(weight_tiled.device)), "debug_sumi_tiled")
    return out


def debug_sumi_tiled_act(activation_tiled: torch.Tensor, weight_tiled: torch.Tensor, M: int, N: int, K: int,
                         wtype: int = Q4_0) -> torch.Tensor:
    """Per-block int32 dots [M, N, K/32] from the instantiation gemm_w4a8_tiled_act launches."""
    lib = _lib.load()
    _require(weight_tiled.is_cuda, "weight_tiled must be a CUDA tensor")
    _check_layout(activation_tiled, "activation_tiled", lib.qg_activations_tiled_bytes(M, K), weight_tiled.device)
    _check_layout(weight_tiled, "weight_tiled", lib.qg_tile_weights_bytes(N, K, wtype), weight_tiled.device)
    out = torch.empty((M, N, K // 32), dtype=torch.int32, device=weight_tiled.device)
    with torch.cuda.device(weight_tiled.device):
        _lib.check(lib.qg_debug_sumi_tiled_act(_ptr(activation_tiled), _ptr(weight_tiled), _ptr(out), M, N, K, wtype,
                                               _stream(weight_tiled.device)), "debug_sumi_tiled_act")
    return out


def debug_config_tiled_act(M: int, N: int, K: int, wtype: int = Q4_0, sumi: bool = False) -> str:
    """The instantiation gemm_w4a8_tiled_act (or debug_sumi_tiled_act) launches; nothing runs."""
    return _config("qg_debug_config_tiled_act", M, N, K, wtype, int(sumi))


def debug_config_tiled(M: int, N: int, K: int, wtype: int = Q4_0, sumi: bool = False) -> str:
    """The instantiation gemm_w4a8_tiled (or debug_sumi_tiled with sumi=True) launches; nothing runs."""
    return _config("qg_debug_config_tiled", M, N, K, wtype, int(sumi))


def select_algo(M: int, N: int, K: int, wtype: int = Q4_0) -> int:
    return _lib.load().qg_select_algo(M, N, K, wtype)


def set_capture_fusion(on) -> None:
    """The capture-time GEMV merge (qg.h at qg_gemm_w4a8): False / 0 off, True / 1 on (default), 2 on for
    every shape class (A/B runs)."""
    _lib.load().qg_set_capture_fusion(int(on))


def set_group_affine(mode) -> None:
    """Affine grouped launches as the strided batch (qg.h at qg_set_group_affine): 0 off, 1 the measured
    shape classes (default), 2 every class."""
    _lib.load().qg_set_group_affine(int(mode))


def group_config(items, M: int, K: int, wtype: int = Q4_0) -> str:
    """The route gemm_w4a8_grouped would take for items = [(A_ptr, B_ptr, C_ptr, N, ldc), ...] (device addresses
    as ints, ldc 0 = N): "gemvg ..." the grouped kernel, "gemvb ..." the strided batch's kernel (an affine
    group). Nothing runs and no pointer is dereferenced (qg_group_config)."""
    n = len(items)
    arr = (_GemvItem * max(n, 1))(*[_GemvItem(*it) for it in items])
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().qg_group_config(arr, n, M, K, wtype, buf, len(buf)), "group_config")
    return buf.value.decode()


def capture_fusion_stats() -> "tuple[int, int]":
    """(merged, nodes): captured GEMV calls merged into an existing graph node, and GEMV nodes started."""
    merged, nodes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.load().qg_capture_fusion_stats(ctypes.byref(merged), ctypes.byref(nodes))
    return int(merged.value), int(nodes.value)


def version() -> str:
    return _lib.load().qg_version().decode()


_lib.load()  # fail loudly at import if the HIP library is absent

__all__ = [
    "quantize_q4_0", "quantize_q8_1", "gemm_q4_0_q8_1", "dequantize_q4_0",
    "QK4_0", "QK8_1", "BLOCK_Q4_0_BYTES", "BLOCK_Q8_1_BYTES",
    "quantize", "dequantize", "gemm_w4a8", "gemm_q4_1_q8_1", "gemm_q5_0_q8_1", "gemm_q5_1_q8_1",
    "gemm_w4a8_batched", "debug_sumi", "debug_config", "select_algo", "version",
    "gemm_w4a8_f32", "gemm_q4_0_fp16_fused", "quantize_q8_1_f16_fused", "gemm_w8a8", "gemm_q8_0_q8_1",
    "gemm_w4a16", "gemm_w8a16", "gemm_q4_0_fp32",
    "tile_weights", "gemm_w4a8_tiled", "debug_sumi_tiled", "debug_config_tiled",
    "quantize_q8_1_tiled", "tile_activations", "gemm_w4a8_tiled_act", "debug_sumi_tiled_act", "debug_config_tiled_act",
    "Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0", "Q8_1", "Q4_K", "Q6_K", "MXFP4", "block_elems",
    "set_capture_fusion", "capture_fusion_stats", "set_group_affine", "group_config",
    "gemm_w4a8_moe", "moe_config",
    "gemm_w4a8_moe_prefill", "moe_prefill_workspace_size", "moe_prefill_config", "debug_moe_prefill_plan",
    "gemm_w4a8_moe_batch", "moe_batch_workspace_size", "moe_batch_config",
    "gemm_w4a8_moe_glu", "moe_glu_config", "GLU_REGLU", "GLU_SWIGLU", "gemm_w4a8_moe_down", "moe_down_config",
    "gemm_w4a8_moe_glu_bias", "moe_glu_bias_config", "gemm_w4a8_moe_down_bias", "moe_down_bias_config", "GLU_SWIGLU_OAI",
    "gemm_w4a8_moe_prefill_bias", "moe_prefill_bias_config", "gemm_w4a8_moe_batch_bias", "moe_batch_bias_config",
]
