"""Shared by tests/test_moe_cpu.py and tests/test_gpu_moe.py: random expert tensors of the seven weight types, the
NumPy / oracle models of one slot with their W = 0 bounds, and the qg_moe_config / qg_debug_config field parser.
Imports without torch."""
import re

import numpy as np

import kquant_ref as KR
import q6k_ref as QR

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q6_K = 2, 3, 6, 7, 8, 12, 14
ROW_TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
ALL_TYPES = ROW_TYPES + (Q4_K, Q6_K)
BB = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q4_K: 144, Q6_K: 210}
BE = {Q4_K: 256, Q6_K: 256}
KQ_REC_BYTES = {Q4_K: 336, Q6_K: 304}  # LDS bytes per (token, super-block) of the decode GEMVs (qg.h)


def be(t):
    return BE.get(t, 32)


def expert_bytes(t, n, k):
    return n * (k // be(t)) * BB[t]


def random_experts(rng, t, n_expert, n, k):
    """uint8 [n_expert, n, k / bs, block bytes], every expert different."""
    if t == Q4_K:
        return KR.random_q4k(rng, n_expert * n, k).reshape(n_expert, n, k // 256, 144)
    if t == Q6_K:
        return QR.random_q6k(rng, n_expert * n, k).reshape(n_expert, n, k // 256, 210)
    from test_gpu_product import random_blocks
    return random_blocks(rng, 1, n_expert * n, k, t)[1].reshape(n_expert, n, k // 32, BB[t])


def random_act(rng, rows, k):
    """Q8_1 uint8 [rows, k/32, 36]."""
    return KR.random_q8_1(rng, rows, k)


def assert_close_to_model(O, c, aq_row, bq_e, t):
    """One slot (c float32 [N]) against the type's model with the decode GEMV's bound (W = 0): the NumPy contract for
    Q4_K / Q6_K, the C oracle's summation bound for the 32-element types."""
    aq_row = aq_row.reshape(1, -1, 36)
    k = 32 * aq_row.shape[1]
    if t in (Q4_K, Q6_K):
        R = KR if t == Q4_K else QR
        c64, _, mag = R.gemm(aq_row, bq_e)
        tol = R.tol(mag, k, 0)
    else:
        c64, s = O.gemm_w4a8(aq_row, bq_e, t, want_sumi=True)
        tol = O.summation_tol(aq_row, bq_e, s, t)
    err = np.abs(c.reshape(1, -1).astype(np.float64) - c64)
    assert (err <= tol).all(), float((err / tol).max())


def cfg_fields(cfg):
    """'moe:gemv F=2 BPL=2 ...' or 'gemv F=2 MT=1 ...' -> (family, {key: value})."""
    head, *rest = cfg.split(" ")
    return head.split(":")[-1], dict(re.findall(r"(\w+)=(\w+)", " ".join(rest)))


def kernel_choice(cfg):
    """What must agree between qg_moe_config and qg_debug_config(1, N, K, t): the family and BPL / LPR / ONEU of the
    row GEMV, LPR / ONE of the super-block ones."""
    fam, f = cfg_fields(cfg)
    keys = ("BPL", "LPR", "ONEU") if fam == "gemv" else ("LPR", "ONE")
    return (fam,) + tuple(f[x] for x in keys)
