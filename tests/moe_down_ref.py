"""Shared by tests/test_moe_down_cpu.py and tests/test_gpu_moe_down.py: the fold of qg_gemm_w4a8_moe_down in NumPy
float32 and the launch the config line names. Imports without torch."""
import numpy as np

import moe_ref as MR


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def fold(d, ids, weights, n_expert):
    """d float32 [T, n_used, N] (the slots' products), ids int [T, >= n_used], weights float32 [T, >= n_used] or None
    (ones) -> float32 [T, N]: acc = +0.0f, then acc = acc + w * d_u for u ascending where 0 <= id < n_expert. Every
    NumPy float32 operation is one rounding, so the entry must give these bits. The weight of a slot whose id is out of
    range is never touched."""
    T, n_used, N = d.shape
    d = np.ascontiguousarray(d, np.float32)
    out = np.zeros((T, N), np.float32)
    for t in range(T):
        acc = np.zeros(N, np.float32)
        for u in range(n_used):
            if not 0 <= int(ids[t, u]) < n_expert:
                continue
            w = np.float32(1.0) if weights is None else np.float32(weights[t, u])
            prod = w * d[t, u]
            acc = acc + prod
            assert prod.dtype == np.float32 and acc.dtype == np.float32
        out[t] = acc
    return out


def launch(cfg):
    """The config line's fields as ints, with W the waves of a workgroup and RPB its rows."""
    fam, f = MR.cfg_fields(cfg)
    v = {k: int(f[k]) for k in ("LPR", "WGS", "ONE", "SW", "lds")}
    v["W"] = v["WGS"] // 64
    v["RPB"] = v["W"] // v["SW"] * (64 // v["LPR"])
    v["grid"] = f["grid"]
    v["family"] = fam
    return v


def lds_bytes(t, n_used, k, rpb):
    return n_used * (k // 256 * MR.KQ_REC_BYTES[t] + 4 * rpb)
