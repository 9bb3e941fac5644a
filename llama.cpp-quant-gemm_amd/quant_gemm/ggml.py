"""ggml-facing adapter (include/llama_adapter.h) and GGUF weight files, over the C-ABI.

    with GGUFFile("model.gguf") as f:
        w = f.to_device("blk.0.attn_q.weight")           # uint8 [N, K/32, 18] for Q4_0, on cuda
        out = gemm_w4a8_from_ggml(act_view, f.view("blk.0.attn_q.weight", w), out_view)

``TensorView`` mirrors ``qg_tensor_view`` (ne[0] = K contiguous, ne[1] = rows, nb[] byte strides),
the part of ggml_tensor the reference adapter reads (llama_adapter.h:49-61). The GGUF reader maps
the file read-only in the library (qg_gguf.hip); nothing in the file is executed.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q8_1 = 0, 1, 2, 3, 6, 7, 8, 9
Q4_K, Q6_K = 12, 14
MXFP4 = 39
I32 = 26  # the ids of mul_mat_id_from_ggml
_BB = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q8_1: 36, Q4_K: 144, Q6_K: 210, MXFP4: 17}
_BE = {Q4_K: 256, Q6_K: 256}  # elements per block where it is not 32 (qg_block_elems)
# the block types the GGUF reader serves (its own list: a Q6_K tensor is listed, not readable); views of bytes the
# caller loaded (view_of) take every type of _BB
_GGUF_BB = {t: bb for t, bb in _BB.items() if t != Q6_K}


class TensorView(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("type", ctypes.c_int), ("ne", ctypes.c_int64 * 4),
                ("nb", ctypes.c_size_t * 4)]


def view_of(t: torch.Tensor, qtype: int, k: int) -> TensorView:
    """ggml-ordered view of a dense row-major tensor holding rows of K elements of ``qtype``."""
    row = k * 4 if qtype == F32 else k * 2 if qtype == F16 else (k // _BE.get(qtype, 32)) * _BB[qtype]
    rows = t.numel() * t.element_size() // row
    v = TensorView()
    v.data, v.type = t.data_ptr(), qtype
    v.ne[:] = [k, rows, 1, 1]
    v.nb[:] = [4 if qtype == F32 else 2 if qtype == F16 else _BB[qtype], row, row * rows, row * rows]
    return v


def _call(sym: str, act: TensorView, w: TensorView, out: TensorView, kernel_type: str | None) -> None:
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kt = kernel_type.encode() if kernel_type else None
    _lib.check(getattr(_lib.load(), sym)(ctypes.byref(act), ctypes.byref(w), ctypes.byref(out), kt, st), sym)


def gemm_w4a8_from_ggml(act: TensorView, w: TensorView, out: TensorView, kernel_type: str | None = "naive") -> None:
    """include/llama_adapter.h:63-76: Q8_1 activation [K, M] x quantized weights [K, N] -> F32 [N, M]."""
    _call("qg_gemm_w4a8_from_view", act, w, out, kernel_type)


def gemm_w4a16_from_ggml(act: TensorView, w: TensorView, out: TensorView, kernel_type: str | None = "naive") -> None:
    """include/llama_adapter.h:78-90: F32 activation x Q4_0 / Q8_0 weights -> F32."""
    _call("qg_gemm_w4a16_from_view", act, w, out, kernel_type)


def gemm_fp32_from_ggml(act: TensorView, w: TensorView, out: TensorView, kernel_type: str | None = "naive") -> None:
    """include/llama_adapter.h:92-103: all F32."""
    _call("qg_gemm_fp32_from_view", act, w, out, kernel_type)


def _mul_mat_id(sym: str, experts: TensorView, act: TensorView, ids: TensorView, out: TensorView,
                workspace: torch.Tensor | None = None) -> None:
    ws = ()
    if workspace is not None:
        if not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
            raise RuntimeError("workspace must be a contiguous CUDA uint8 tensor")
        ws = (ctypes.c_void_p(workspace.data_ptr()), workspace.numel())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(_lib.load(), sym)(ctypes.byref(experts), ctypes.byref(act), ctypes.byref(ids), ctypes.byref(out),
                                         *ws, st), sym)


def mul_mat_id_from_ggml(experts: TensorView, act: TensorView, ids: TensorView, out: TensorView) -> None:
    """ggml_mul_mat_id on views (qg_mul_mat_id_from_view): experts [K, N, n_expert], Q8_1 act [K, a_rows, T], I32
    ids [n_used, T] on the device (a strided top-k view is fine), F32 out [N, n_used, T]."""
    _mul_mat_id("qg_mul_mat_id_from_view", experts, act, ids, out)


def mul_mat_id_from_ggml_ws(experts: TensorView, act: TensorView, ids: TensorView, out: TensorView,
                            workspace: torch.Tensor) -> None:
    """The same views through the expert-grouped MFMA prefill (qg_mul_mat_id_from_view_ws): Q4_K / Q6_K experts at
    prompt sizes. ``workspace``: a CUDA uint8 tensor of quant_gemm.moe_prefill_workspace_size(T, n_used, n_expert)
    bytes or more."""
    _mul_mat_id("qg_mul_mat_id_from_view_ws", experts, act, ids, out, workspace)


def mul_mat_id_from_ggml_batch(experts: TensorView, act: TensorView, ids: TensorView, out: TensorView,
                               workspace: torch.Tensor) -> None:
    """The same views through the expert-grouped decode GEMV (qg_mul_mat_id_from_view_batch): Q4_K / Q6_K experts for
    batched decode. ``workspace``: a CUDA uint8 tensor of quant_gemm.moe_batch_workspace_size(T, n_used, n_expert)
    bytes or more."""
    _mul_mat_id("qg_mul_mat_id_from_view_batch", experts, act, ids, out, workspace)


def mul_mat_id_glu_from_ggml(gate: TensorView, up: TensorView, act: TensorView, ids: TensorView, out: TensorView,
                             glu_op: int = 2) -> None:
    """The fused gate / up pair of an MoE FFN block on views (qg_mul_mat_id_glu_from_view): out = glu_op(gate x act) *
    (up x act), the views of ``mul_mat_id_from_ggml`` with Q4_K / Q6_K experts, act [K, 1, T] and ``up`` matching
    ``gate`` in type, ne and nb. ``glu_op``: 2 SwiGLU, 0 ReGLU (ggml_glu_op's numbers)."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().qg_mul_mat_id_glu_from_view(ctypes.byref(gate), ctypes.byref(up), ctypes.byref(act),
                                                       ctypes.byref(ids), ctypes.byref(out), glu_op, st),
               "qg_mul_mat_id_glu_from_view")


def mul_mat_id_down_from_ggml(experts: TensorView, act: TensorView, ids: TensorView, weights: TensorView | None,
                              out: TensorView) -> None:
    """The down product of an MoE FFN block with the weighted sum over the token's experts on views
    (qg_mul_mat_id_down_from_view): out[t] = sum_u weights[t, u] * (experts[ids[t, u]] x act[t, u]), Q4_K / Q6_K experts,
    act [K, n_used, T], weights F32 [n_used, T] or [1, n_used, T] or None (every weight 1), out F32 [N, T]."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().qg_mul_mat_id_down_from_view(ctypes.byref(experts), ctypes.byref(act), ctypes.byref(ids),
                                                        None if weights is None else ctypes.byref(weights),
                                                        ctypes.byref(out), st),
               "qg_mul_mat_id_down_from_view")


def mul_mat_id_glu_bias_from_ggml(gate: TensorView, up: TensorView, bias_gate: TensorView | None,
                                  bias_up: TensorView | None, act: TensorView, ids: TensorView, out: TensorView,
                                  glu_op: int = 3, alpha: float = 1.702, limit: float = 7.0) -> None:
    """``mul_mat_id_glu_from_ggml`` with per-expert biases and gpt-oss's clamped SwiGLU (``glu_op`` 3), for Q4_K /
    Q6_K / MXFP4 experts (qg_mul_mat_id_glu_bias_from_view). A bias: F32 [N, n_expert] with nb[0] = 4, or None."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = lambda v: None if v is None else ctypes.byref(v)
    _lib.check(_lib.load().qg_mul_mat_id_glu_bias_from_view(ctypes.byref(gate), ctypes.byref(up), ref(bias_gate),
                                                            ref(bias_up), ctypes.byref(act), ctypes.byref(ids),
                                                            ctypes.byref(out), glu_op, alpha, limit, st),
               "qg_mul_mat_id_glu_bias_from_view")


def mul_mat_id_down_bias_from_ggml(experts: TensorView, bias: TensorView | None, act: TensorView, ids: TensorView,
                                   weights: TensorView | None, out: TensorView) -> None:
    """``mul_mat_id_down_from_ggml`` with a per-expert bias added to every product ahead of the weighted sum, for
    Q4_K / Q6_K / MXFP4 experts (qg_mul_mat_id_down_bias_from_view). ``bias``: F32 [N, n_expert] with nb[0] = 4, or None."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = lambda v: None if v is None else ctypes.byref(v)
    _lib.check(_lib.load().qg_mul_mat_id_down_bias_from_view(ctypes.byref(experts), ref(bias), ctypes.byref(act),
                                                             ctypes.byref(ids), ref(weights), ctypes.byref(out), st),
               "qg_mul_mat_id_down_bias_from_view")


def _mul_mat_id_bias(sym: str, experts, bias, act, ids, out, workspace: torch.Tensor) -> None:
    if not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise RuntimeError("workspace must be a contiguous CUDA uint8 tensor")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(_lib.load(), sym)(ctypes.byref(experts), None if bias is None else ctypes.byref(bias),
                                         ctypes.byref(act), ctypes.byref(ids), ctypes.byref(out),
                                         ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), st), sym)


def mul_mat_id_bias_from_ggml_ws(experts: TensorView, bias: TensorView | None, act: TensorView, ids: TensorView,
                                 out: TensorView, workspace: torch.Tensor) -> None:
    """``mul_mat_id_from_ggml_ws`` with ggml's add_id folded in, for Q4_K / Q6_K / MXFP4 experts
    (qg_mul_mat_id_bias_from_view_ws). ``bias``: F32 [N, n_expert] with nb[0] = 4, or None: no add."""
    _mul_mat_id_bias("qg_mul_mat_id_bias_from_view_ws", experts, bias, act, ids, out, workspace)


def mul_mat_id_bias_from_ggml_batch(experts: TensorView, bias: TensorView | None, act: TensorView, ids: TensorView,
                                    out: TensorView, workspace: torch.Tensor) -> None:
    """``mul_mat_id_from_ggml_batch`` with ggml's add_id folded in, for Q4_K / Q6_K / MXFP4 experts
    (qg_mul_mat_id_bias_from_view_batch). ``bias``: F32 [N, n_expert] with nb[0] = 4, or None: no add."""
    _mul_mat_id_bias("qg_mul_mat_id_bias_from_view_batch", experts, bias, act, ids, out, workspace)


def validate_tensor_types(act: TensorView, w: TensorView, out: TensorView, ea: int, ew: int, eo: int) -> bool:
    """include/llama_adapter.h:110-117."""
    return bool(_lib.load().qg_validate_view_types(ctypes.byref(act), ctypes.byref(w), ctypes.byref(out), ea, ew, eo))


class GGUFTensor:
    def __init__(self, index: int, name: str, qtype: int, ne: list[int], nbytes: int):
        self.index, self.name, self.type, self.ne, self.nbytes = index, name, qtype, ne, nbytes

    @property
    def shape(self) -> tuple:
        """torch-order shape of the data: [.., rows, K/32, block bytes] (quantized; Q4_K: [.., rows, K/256, 144])
        or [.., rows, K]."""
        dims = [d for d in reversed(self.ne)]
        while len(dims) > 1 and dims[0] == 1:
            dims = dims[1:]
        if self.type in _GGUF_BB:
            return tuple(dims[:-1]) + (dims[-1] // _BE.get(self.type, 32), _GGUF_BB[self.type])
        return tuple(dims)

    def __repr__(self) -> str:
        return f"GGUFTensor({self.name!r}, type={self.type}, ne={self.ne}, nbytes={self.nbytes})"


class GGUFFile:
    """Read-only GGUF v2/v3 file (metadata, tensor directory, tensor bytes)."""

    def __init__(self, path: str | os.PathLike):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.qg_gguf_open(os.fsencode(path), ctypes.byref(h)), f"gguf open {path}")
        self._h = h
        self.version = self._lib.qg_gguf_version(h)
        self.alignment = self._lib.qg_gguf_alignment(h)
        self.tensors: dict[str, GGUFTensor] = {}
        for i in range(self._lib.qg_gguf_tensor_count(h)):
            name, t, nd = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
            ne, nb = (ctypes.c_int64 * 4)(), ctypes.c_uint64()
            _lib.check(self._lib.qg_gguf_tensor_info(h, i, ctypes.byref(name), ctypes.byref(t), ctypes.byref(nd), ne,
                                                     ctypes.byref(nb)), "gguf tensor info")
            n = name.value.decode()
            self.tensors[n] = GGUFTensor(i, n, t.value, list(ne)[:nd.value], nb.value)
        self.metadata: dict[str, object] = {}
        for i in range(self._lib.qg_gguf_kv_count(h)):
            key, t, cnt, et = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_int()
            _lib.check(self._lib.qg_gguf_kv_info(h, i, ctypes.byref(key), ctypes.byref(t), ctypes.byref(cnt),
                                                 ctypes.byref(et)), "gguf kv info")
            self.metadata[key.value.decode()] = self._value(i, t.value, cnt.value, et.value)

    def _value(self, i: int, t: int, count: int, elem: int):
        if t == 8:
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            _lib.check(self._lib.qg_gguf_kv_string(self._h, i, ctypes.byref(p), ctypes.byref(n)), "gguf kv")
            return ctypes.string_at(p, n.value).decode("utf-8", "replace")
        if t == 9:
            return ("array", elem, count)
        if t in (6, 12):
            v = ctypes.c_double()
            _lib.check(self._lib.qg_gguf_kv_float(self._h, i, ctypes.byref(v)), "gguf kv")
            return v.value
        v = ctypes.c_int64()
        _lib.check(self._lib.qg_gguf_kv_int(self._h, i, ctypes.byref(v)), "gguf kv")
        return bool(v.value) if t == 7 else v.value

    def close(self) -> None:
        if self._h:
            self._lib.qg_gguf_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _t(self, name: str) -> GGUFTensor:
        if name not in self.tensors:
            raise KeyError(name)
        t = self.tensors[name]
        if t.nbytes == 0:
            raise RuntimeError(f"{name}: tensor type {t.type} not supported")
        return t

    def host_bytes(self, name: str) -> np.ndarray:
        """A copy of the tensor's bytes (uint8, torch-order shape)."""
        t = self._t(name)
        p = self._lib.qg_gguf_tensor_data(self._h, t.index)
        raw = np.frombuffer(ctypes.string_at(p, t.nbytes), np.uint8)
        if t.type in _GGUF_BB:
            return raw.reshape(t.shape)
        return raw.view(np.float32 if t.type == F32 else np.float16).reshape(t.shape)

    def to_device(self, name: str, device: str | torch.device = "cuda") -> torch.Tensor:
        """Upload the tensor (uint8 [.., rows, K/32, bb] for quantized types, float32/float16 otherwise)."""
        t = self._t(name)
        dtype = torch.uint8 if t.type in _GGUF_BB else torch.float32 if t.type == F32 else torch.float16
        out = torch.empty(t.shape, dtype=dtype, device=device)
        with torch.cuda.device(out.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
            _lib.check(self._lib.qg_gguf_upload_tensor(self._h, t.index, ctypes.c_void_p(out.data_ptr()),
                                                       out.numel() * out.element_size(), st), "gguf upload")
        return out

    def view(self, name: str, device_tensor: torch.Tensor) -> TensorView:
        """The ggml-ordered view of ``name``'s bytes held in ``device_tensor``."""
        t = self._t(name)
        v = TensorView()
        _lib.check(self._lib.qg_gguf_tensor_view(self._h, t.index, ctypes.c_void_p(device_tensor.data_ptr()),
                                                 ctypes.byref(v)), "gguf view")
        return v
