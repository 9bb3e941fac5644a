"""qg_gemm_w4a8_moe_down without a GPU: the exported symbols, the kernel file's includes of the two decode GEMV bodies,
the validation codes and their order (on fake pointers that every call refuses before a launch), qg_moe_down_config
against qg_moe_config and the documented grid / LDS formulas, and the host twin qg_gemm_w4a8_moe_down_cpu against
qg_gemm_w4a8_moe_cpu at a_rows = n_used folded in NumPy float32 (moe_down_ref.fold), bit for bit."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import moe_down_ref as DR
import moe_ref as MR
from moe_down_ref import bits
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
CONFIG_K = (256, 512, 1024, 1280, 4096, 4352)  # LPR 4 / 16 / 64, each loop-free and with the unit loop
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llama.cpp-quant-gemm_amd", "csrc")
# the largest K the entry serves, by n_used (qg.h)
K_LIMIT = {Q4_K: {1: 124672, 2: 62208, 4: 30976, 6: 20736, 8: 15360, 10: 12288, 16: 7680, 32: 3840},
           Q6_K: {1: 137728, 2: 68864, 4: 34304, 6: 22784, 8: 17152, 10: 13568, 16: 8448, 32: 4096}}


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


@pytest.fixture(scope="module")
def H():
    import quant_gemm.host as H
    H.load()
    return H


# ---------------------------------------------------------------------------- surface
def test_new_symbols_are_exported(H):
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    new = {"qg_gemm_w4a8_moe_down", "qg_moe_down_config", "qg_mul_mat_id_down_from_view"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert new <= set(re.findall(r" T (qg_\w+)", nm)) and new <= set(L.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qg_gemm_w4a8_moe_down_cpu" in set(re.findall(r" T (qg_\w+)", nm))
    assert "qg_gemm_w4a8_moe_down_cpu" in H.SIGNATURES and hasattr(H.load(), "qg_gemm_w4a8_moe_down_cpu")
    assert {"gemm_w4a8_moe_down", "moe_down_config"} <= set(quant_gemm.__all__)
    assert callable(quant_gemm.gemm_w4a8_moe_down) and callable(quant_gemm.moe_down_config)
    assert callable(G.mul_mat_id_down_from_ggml) and callable(H.gemm_w4a8_moe_down)
    hdr = open(os.path.join(REPO, "include", "qg", "qg.h")).read()
    for sym in new:
        assert re.search(rf"\bint {sym}\(", hdr), sym
    assert re.search(r"\bint qg_gemm_w4a8_moe_down_cpu\(", open(os.path.join(REPO, "include", "qg", "qg_host.h")).read())


@pytest.mark.parametrize("tag", ["q4k", "q6k"])
def test_kernel_file_includes_the_decode_body(tag):
    """qg_moe_down.hip runs the decode GEMV's own text and carries no copy of it: each body is included for the staging
    prologue (QG_KQ_STAGE_ONLY) and for the product, nothing of it is written out, and the three hooks are defined
    nowhere else under csrc/, so the shipped includers see the text they saw. The file is built into the library."""
    import glob
    text = open(os.path.join(CSRC, "qg_moe_down.hip")).read()
    assert text.count(f'#include "qg_{tag}_gemv_body.inc"\n') == 2
    assert "auto do_unit" not in text and "auto load_unit" not in text and "auto put_ablk" not in text
    for hook in ("QG_KQ_STAGE_ONLY", "QG_KQ_ROW", "QG_KQ_RECS"):
        holders = {os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.h*"))
                   if re.search(rf"#define {hook}\b", open(f).read())}
        assert holders == {"qg_moe_down.hip"}, (hook, holders)
        assert f"#undef {hook}\n" in text
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " qg_moe_down.hip " in mk and " qg_moe_down.hpp " in mk
    assert '"qg_moe_down"' in open(os.path.join(REPO, "tools", "kq_asm_compare.py")).read()


def test_barriers_stand_outside_the_slot_loop():
    """The kernel's own barrier comes after the per-slot loop, at the kernel's top level; the loop holds none (its trip
    count differs between the waves of a workgroup)."""
    text = open(os.path.join(CSRC, "qg_moe_down.hip")).read()
    kernel = text[text.index("void kq_moe_down_kernel("):text.index("// ---- host side")]
    loop = kernel[kernel.index("for (int u = wave"):]
    loop = loop[:loop.index("\n    }\n") + 7]
    assert "__syncthreads" not in loop and "_stage<" not in loop
    assert kernel.count("__syncthreads();") == 1
    assert kernel.index("_stage<") < kernel.index("for (int u = wave") < kernel.index("\n    __syncthreads();\n")


# ---------------------------------------------------------------------------- validation
def down(so, A=4096, B=4096, n_expert=4, ids=4096, ids_stride=2, W=4096, w_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256,
         t=Q4_K):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_down(p(A), p(B), n_expert, p(ids), ids_stride, p(W), w_stride, p(C), ldc, T, n_used, N, K, t,
                                    None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    # 1 negative size, before K
    for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}):
        assert down(so, K=33, t=9, **kw) == -1
    # 2 K granule, before the type: 256 for Q4_K / Q6_K, 32 for every other type id
    assert down(so, K=33, t=9) == -2 and down(so, K=0) == -2 and down(so, K=-256) == -2
    assert down(so, K=288, t=Q4_K) == -2 and down(so, K=4128, t=Q6_K) == -2 and down(so, K=33, t=ROW_TYPES[0]) == -2
    # 3 type, before the empty call: the five 32-element types are none of this entry's
    for t in ROW_TYPES + (9, 13, 26, 0, 1, 5):
        assert down(so, K=256, t=t, T=0, A=None) == -3, t
        assert down(so, K=256, t=t) == -3, t
    # 4 empty: nothing touched, whatever the rest is
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        for t in (Q4_K, Q6_K):
            assert down(so, A=None, B=None, ids=None, W=None, C=None, n_expert=0, ids_stride=-3, w_stride=-5, ldc=-1, t=t,
                        **kw) == 0
            assert down(so, A=4097, B=4097, ids=4097, W=4097, C=None, t=t, **kw) == 0
    # 5 null pointer, before alignment; weights may be null
    for kw in ({"A": None}, {"B": None}, {"ids": None}, {"C": None}):
        other = {"B": 4097} if "B" not in kw else {"A": 4098}
        assert down(so, **kw, **other) == -1, kw
        assert down(so, W=4098, **kw) == -1, kw
    assert down(so, W=None, B=4104) == -4 and down(so, W=None, A=4098) == -4  # a null weights is no null-pointer error
    # 6 alignment: A, ids and weights 4 B; B 16 B (Q4_K), 2 B (Q6_K); before the entry's own checks
    assert down(so, A=4098, n_expert=0) == -4 and down(so, ids=4098, n_expert=0) == -4
    for w in (4097, 4098, 4099):
        assert down(so, W=w, n_expert=0, w_stride=0, T=65536) == -4, w
    for b in (4104, 4100, 4098):
        assert down(so, t=Q4_K, B=b, ldc=3) == -4, b
    assert down(so, B=4097, t=Q6_K, ids_stride=1) == -4
    assert down(so, B=4098, t=Q6_K, ids_stride=1) == -1  # 4n + 2 is enough for Q6_K
    # the arguments: INVALID_ARG, before the unsupported shapes
    for big in ({}, {"T": 65536}, {"K": 62464}):
        assert down(so, ids_stride=1, **big) == -1 and down(so, ids_stride=-1, **big) == -1
        assert down(so, n_expert=0, **big) == -1 and down(so, n_expert=-2, **big) == -1
        assert down(so, ldc=7, **big) == -1 and down(so, ldc=-8, **big) == -1
        assert down(so, w_stride=1, **big) == -1 and down(so, w_stride=0, **big) == -1 and down(so, w_stride=-2, **big) == -1
    # w_stride is not looked at without weights: the call goes on to the next refusal
    assert down(so, W=None, w_stride=0, T=65536) == -3 and down(so, W=None, w_stride=-7, K=62464) == -3
    # the entry's own refusals, all UNSUPPORTED with nothing launched
    for t in (Q4_K, Q6_K):
        assert down(so, T=65536, t=t) == -3 and down(so, T=65536, n_used=1, ids_stride=1, w_stride=1, t=t) == -3
        k1 = (160 * 1024 // MR.KQ_REC_BYTES[t] + 1) * 256  # the records of one row beyond 160 KiB: off the GEMV
        assert down(so, K=k1, n_used=1, ids_stride=1, w_stride=1, t=t) == -3
        for n_used, k in K_LIMIT[t].items():                # the records of n_used rows and the products beyond it
            assert down(so, K=k + 256, n_used=n_used, ids_stride=n_used, w_stride=n_used, t=t) == -3, (t, n_used)
        assert down(so, K=256, n_used=2 ** 31 - 1, ids_stride=2 ** 31, w_stride=2 ** 31, t=t) == -3


# ---------------------------------------------------------------------------- the config line
def down_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_down_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


def moe_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("k", CONFIG_K)
def test_down_config_names_the_decode_entrys_form_and_the_documented_launch(so, t, k):
    import quant_gemm as qg
    fam = "q4k_gemv" if t == Q4_K else "q6k_gemv"
    seen = set()
    for n_used in (1, 2, 3, 4, 8, 9, 16, 20):
        for n in (1, 63, 64, 65, 300, 4096):
            rc, cfg = down_cfg(so, 3, n_used, n, k, t)
            assert rc == 0 and cfg.startswith(f"moe_down:{fam} "), (rc, cfg)
            assert set(MR.cfg_fields(cfg)[1]) == {"LPR", "WGS", "ONE", "SW", "grid", "lds"}
            f = DR.launch(cfg)
            ref = MR.cfg_fields(moe_cfg(so, 3, n_used, n, k, t)[1])[1]
            assert (f["LPR"], f["WGS"], f["ONE"]) == (int(ref["LPR"]), int(ref["WGS"]), int(ref["ONE"])), (cfg, ref)
            # SW: a power of two of the workgroup's waves, never more than the slots
            sw = f["SW"]
            assert sw >= 1 and sw & (sw - 1) == 0 and f["W"] % sw == 0 and sw <= max(1, n_used), cfg
            assert sw == max(s for s in (1, 2, 4, 8, 16) if s <= min(n_used, f["W"])), cfg  # the rule qg.h states
            rpb = f["RPB"]
            assert 1 <= rpb <= 64
            assert f["grid"] == f"{(n + rpb - 1) // rpb}x3", cfg
            assert f["lds"] == DR.lds_bytes(t, n_used, k, rpb), cfg
            assert qg.moe_down_config(3, n_used, n, k, t) == cfg
            seen.add(sw)
    assert seen == ({1, 2, 4} if k < 1024 else {1, 2, 4, 8} if k < 4096 else {1, 2, 4, 8, 16})


def test_down_config_codes(so):
    assert so.qg_moe_down_config(1, 1, 8, 256, Q4_K, None, 0) == -1
    assert down_cfg(so, -1, 1, 8, 33, Q4_K)[0] == -1 and down_cfg(so, 1, 1, 8, 288, Q4_K)[0] == -2
    for t in ROW_TYPES + (9,):
        assert down_cfg(so, 1, 1, 8, 256, t) == (-3, "")
    assert down_cfg(so, 0, 2, 8, 256, Q6_K) == (0, "")
    # the token is the grid's y: 65535 tokens of any number of slots, not 65535 slots
    assert down_cfg(so, 65535, 1, 8, 256, Q4_K)[0] == 0 and down_cfg(so, 65536, 1, 8, 256, Q4_K) == (-3, "")
    rc, cfg = down_cfg(so, 65535, 8, 8, 256, Q4_K)
    assert rc == 0 and DR.launch(cfg)["grid"].endswith("x65535")
    for t in (Q4_K, Q6_K):
        for n_used, k in K_LIMIT[t].items():
            rc, cfg = down_cfg(so, 2, n_used, 8, k, t)
            assert rc == 0, (t, n_used, k)
            f = DR.launch(cfg)
            assert f["lds"] == DR.lds_bytes(t, n_used, k, f["RPB"]) <= 160 * 1024
            assert down_cfg(so, 2, n_used, 8, k + 256, t) == (-3, ""), (t, n_used, k)


# ---------------------------------------------------------------------------- the host twin
def host_case(t, seed=0, n_used=3, T=4):
    """Experts, one activation row per slot, ids with a row stride n_expert > n_used (repeated inside a token and across
    tokens, -1 and n_expert, token 3 with no id in range) and weights with a row stride n_used + 2; the weights at the
    slots whose id is out of range are NaN, inf and -inf."""
    n_expert, n, k = 5, 7, 512
    rng = np.random.default_rng([t, seed, 23])
    experts = MR.random_experts(rng, t, n_expert, n, k)
    a = MR.random_act(rng, T * n_used, k).reshape(T, n_used, k // 32, 36)
    ids = rng.integers(0, n_expert, (T, n_expert)).astype(np.int32)
    ids[0, :2] = (3, 3)
    ids[2, 0] = ids[1, 0]
    ids[1, 1] = -1
    ids[2, n_used - 1] = n_expert
    ids[3, :n_used] = (-1, n_expert, 2 ** 31 - 1, -2 ** 31)[:n_used]
    w = rng.uniform(-1.0, 1.0, (T, n_used + 2)).astype(np.float32)
    w[0, 0] = 0.0
    bad = [(tt, u) for tt in range(T) for u in range(n_used) if not 0 <= ids[tt, u] < n_expert]
    for i, (tt, u) in enumerate(bad):
        w[tt, u] = (np.nan, np.inf, -np.inf)[i % 3]
    return T, n_used, n_expert, n, k, experts, a, ids, w


def reference(H, case, t, weights):
    T, n_used, n_expert, n, k, experts, a, ids, w = case
    d = H.gemm_w4a8_moe(a, experts, ids, T, n_used, n, k, t, a_rows=n_used)
    return DR.fold(d, ids, weights, n_expert), d


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("n_used", [1, 3, 4])
def test_host_twin_bits(H, t, n_used):
    case = host_case(t, n_used=n_used)
    T, n_used, n_expert, n, k, experts, a, ids, w = case
    ref, d = reference(H, case, t, w)
    c = H.gemm_w4a8_moe_down(a, experts, ids, w, T, n_used, n, k, t)
    assert c.shape == (T, n) and c.dtype == np.float32
    assert np.array_equal(bits(c), bits(ref))
    assert np.isfinite(c).all() and (c[:3] != 0).any()  # the NaN and inf weights of the out-of-range slots reach nothing
    assert (bits(c[3]) == 0).all()                      # no id in range: +0.0f
    if n_used >= 4:  # the order matters: three or more rounded additions
        assert not np.array_equal(bits(ref), bits(DR.fold(d[:, ::-1], ids[:, n_used - 1::-1], w[:, n_used - 1::-1], n_expert)))


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_host_twin_null_weights_are_ones(H, t):
    case = host_case(t, seed=1)
    T, n_used, n_expert, n, k, experts, a, ids, w = case
    none = H.gemm_w4a8_moe_down(a, experts, ids, None, T, n_used, n, k, t)
    ones = H.gemm_w4a8_moe_down(a, experts, ids, np.ones((T, n_used), np.float32), T, n_used, n, k, t)
    assert np.array_equal(bits(none), bits(ones)) and np.array_equal(bits(none), bits(reference(H, case, t, None)[0]))
    assert not np.array_equal(bits(none), bits(H.gemm_w4a8_moe_down(a, experts, ids, w, T, n_used, n, k, t)))


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_host_twin_threads(H, t):
    T, n_used, n_expert, n, k, experts, a, ids, w = host_case(t, seed=2)
    c = H.gemm_w4a8_moe_down(a, experts, ids, w, T, n_used, n, k, t, threads=1)
    for threads in (2, 7):
        assert np.array_equal(bits(c), bits(H.gemm_w4a8_moe_down(a, experts, ids, w, T, n_used, n, k, t, threads=threads)))


def test_host_twin_strided_output_and_codes(H):
    t = Q4_K
    T, n_used, n_expert, n, k, experts, a, ids, w = host_case(t, seed=3)
    dense = H.gemm_w4a8_moe_down(a, experts, ids, w, T, n_used, n, k, t)
    ldc = n + 3
    buf = np.full((T + 2, ldc), -7.0, np.float32)
    fn = H.load().qg_gemm_w4a8_moe_down_cpu
    p = lambda x: P(x.ctypes.data)
    args = lambda **kw: dict(dict(A=p(a), B=p(experts), n_expert=n_expert, ids=p(ids), ids_stride=n_expert, W=p(w),
                                  w_stride=n_used + 2, C=P(buf.ctypes.data + 4 * ldc), ldc=ldc, T=T, n_used=n_used, N=n, K=k,
                                  t=t, threads=2), **kw)
    call = lambda **kw: fn(*args(**kw).values())
    assert call() == 0
    assert np.array_equal(bits(buf[1:-1, :n]), bits(dense))
    assert (buf[0] == -7.0).all() and (buf[-1] == -7.0).all() and (buf[:, n:] == -7.0).all()
    assert call(T=-1, K=33) == -1 and call(K=33, t=9) == -2 and call(K=288) == -2
    assert call(t=9, T=0) == -3 and call(t=2) == -3 and call(t=8, T=0) == -3
    assert call(T=0, A=None, w_stride=-1) == 0
    assert call(A=None) == -1 and call(B=None) == -1 and call(ids=None) == -1 and call(C=None) == -1
    assert call(ids_stride=1) == -1 and call(n_expert=0) == -1 and call(ldc=n - 1) == -1 and call(ldc=-1) == -1
    assert call(w_stride=n_used - 1) == -1
    buf[:] = -7.0
    assert call(W=None, w_stride=0) == 0
    assert np.array_equal(bits(buf[1:-1, :n]), bits(H.gemm_w4a8_moe_down(a, experts, ids, None, T, n_used, n, k, t)))
