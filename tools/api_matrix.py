#!/usr/bin/env python3
"""Status and dispatch matrix of the C ABI (include/qg/qg.h), taken without a GPU.

Everything qg_api.hip decides, it decides before anything is enqueued: a rejected call returns its code, an
empty one returns QG_OK, and the configuration queries (qg_debug_config*, qg_select_algo,
qg_gemm_w4a8_workspace_size) launch nothing by construction. This tool runs both kinds of call against a
library and records what comes back, so that two builds of the library can be compared case by case.

* dispatch half: the queries over weight type x algo x sumi x M x N x K -> (status, describe string);
* status half: every pointer-taking entry point with one defect at a time (negative / zero size, bad K, weight
  type, null or misaligned pointer, ldc, batch strides, workspace, view fields) and with the pairs whose
  precedence matters. Only calls the library rejects or treats as empty belong here: `would_launch` keeps
  out the calls that pass validation, and a recorded QG_ERR_HIP (a call that did reach a launch) is dropped
  and counted -- the count must be 0.

The library is driven in a fresh child process with no device visible (HIP_VISIBLE_DEVICES=-1). The child
asks the HIP runtime for the device count first and, if it sees one, runs only the launch-free dispatch half:
a validation regression must show up as a wrong code, never as a kernel launched on a made-up address.

  api_matrix.py --record LIB          write tests/golden/api_matrix.json (the committed grid) from LIB
  api_matrix.py --check LIB           replay the committed grid against LIB, print the differing cases
  api_matrix.py --compare A.so B.so   run the full grid live against both, print the differing cases
"""
from __future__ import annotations

import argparse
import base64
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "api_matrix.json")

ERR_HIP = -5
TYPES = [2, 3, 6, 7, 8, 12, 9, 99]  # the weight formats, Q4_K, Q8_1 (not a weight format), an unknown id
W32 = (2, 3, 6, 7, 8)
ALGOS = [0, 1, 2, 3, 4]

# ---- the grids -------------------------------------------------------------------------------------------
FULL = dict(M=[0, 1, 2, 3, 4, 5, 8, 9, 16, 32, 33, 64, 65, 128, 512], N=[1, 31, 64, 4000, 4096, 11008, 32000],
            K=[32, 64, 256, 288, 1024, 4096, 4128, 8192, 8224, 14336, 16416])
# committed: every boundary the dispatch code names -- M = 4 | 5 (GEMV | MFMA), 8 | 9 (Q4_K GEMV | MFMA), 64 | 65
# and 512 (the large-M kernel's tiles), K/32 odd (288, 4128), K = 4096 | 8192 (one-unit GEMV forms), K/32 = 256 |
# 257 (8192 | 8224, tiled decode), N = 8192 (row-count split of the GEMV grid) and an N that is no multiple of a tile
COMMITTED = dict(M=[0, 1, 2, 4, 5, 8, 9, 64, 65, 512], N=[4000, 8192], K=[288, 4096, 4128, 8192, 8224])


def dispatch_cases(grid):
    """(entry, args) of the launch-free queries; sumi innermost (it must not change the answer)."""
    mnk = list(itertools.product(grid["M"], grid["N"], grid["K"]))
    for t in TYPES:
        for a in ALGOS:
            for m, n, k in mnk:
                for s in (0, 1):
                    yield "qg_debug_config", (m, n, k, t, a, s)
        for name in ("qg_debug_config_tiled", "qg_debug_config_tiled_act"):
            for m, n, k in mnk:
                for s in (0, 1):
                    yield name, (m, n, k, t, s)
        for m, n, k in mnk:
            yield "qg_select_algo", (m, n, k, t)
        for m, n, k in mnk:
            yield "qg_gemm_w4a8_workspace_size", (m, n, k, t)


# ---- status half: entry points, their parameters and what each requires ------------------------------------
# A parameter is "name:kind[:detail]". Kinds: p<align> pointer (good value 4096; align 0 = never checked),
# n size, k the K argument, t weight type, a algo, l ldc (int64), b batch, s<align> batch stride (int64),
# w workspace pointer (with `z` its byte count), c element count (int64), q type / v variant of qg_quantize,
# st stream. `types`: the weight types the entry accepts. `gran`: its K granule for a type.
class Entry:
    def __init__(self, name, spec, types=W32, fixed_type=None, q4k=None, ws_need=None, k_free=False):
        self.name, self.types, self.fixed_type, self.ws_need, self.k_free = name, types, fixed_type, ws_need, k_free
        self.params = [p.split(":") for p in spec.split()]
        self.q4k = q4k  # pointer alignments when the type is Q4_K (entries that take it)

    def align(self, pname, args):
        if self.q4k and args.get("wtype") == 12:
            return self.q4k.get(pname, 0)
        for p in self.params:
            if p[0] == pname:
                return int(p[1][1:] or 0)
        return 0

    def gran(self, args):
        return 256 if args.get("wtype", self.fixed_type) == 12 and 12 in self.types else 32


PROD = "A:p0 B:p2 C:p0 M:n N:n K:k"
Q4K_AL = {"A": 4, "B": 16}
ALL = W32 + (12,)
ENTRIES = [
    Entry("qg_gemm_w4a8", PROD + " wtype:t st", ALL, q4k=Q4K_AL),
    Entry("qg_gemm_w4a8_ex", PROD + " wtype:t algo:a st", ALL, q4k=Q4K_AL),
    Entry("qg_gemm_w4a8_ldc", PROD + " ldc:l wtype:t algo:a st", ALL, q4k=Q4K_AL),
    Entry("qg_debug_sumi", PROD + " wtype:t algo:a st", ALL, q4k=Q4K_AL),
    Entry("qg_gemm_q4_0_q8_1_w4a8", PROD + " st", fixed_type=2),
    Entry("qg_gemm_w8a8", PROD + " st", fixed_type=8),
    Entry("qg_gemm_w4a8_strided_batched", "A:p0 sA:s4 B:p2 sB:s2 C:p0 sC:s0 batch:b M:n N:n K:k wtype:t st"),
    Entry("qg_gemm_w4a8_ws", PROD + " wtype:t ws:w wsb:z st"),
    Entry("qg_gemm_w4a8_padded", PROD + " wtype:t st"),
    Entry("qg_gemm_w4a8_prepacked", PROD + " wtype:t ws:w wsb:z st", ws_need="prepacked"),
    Entry("qg_gemm_w4a8_tiled", "A:p16 B:p16 C:p0 M:n N:n K:k wtype:t st"),
    Entry("qg_gemm_w4a8_tiled_ldc", "A:p16 B:p16 C:p0 M:n N:n K:k ldc:l wtype:t st"),
    Entry("qg_debug_sumi_tiled", "A:p16 B:p16 C:p0 M:n N:n K:k wtype:t st"),
    Entry("qg_gemm_w4a8_tiled_act", "A:p16 B:p16 C:p0 M:n N:n K:k wtype:t st"),
    Entry("qg_gemm_w4a8_tiled_act_ldc", "A:p16 B:p16 C:p0 M:n N:n K:k ldc:l wtype:t st"),
    Entry("qg_debug_sumi_tiled_act", "A:p16 B:p16 C:p0 M:n N:n K:k wtype:t st"),
    # weight-major twins: (W, A, out, M weight rows, N tokens, K)
    Entry("qg_gemm_q4_0_q8_1", "B:p2 A:p0 C:p0 M:n N:n K:k st", fixed_type=2),
    Entry("qg_gemm_q4_1_q8_1", "B:p2 A:p0 C:p0 M:n N:n K:k st", fixed_type=3),
    Entry("qg_gemm_q5_0_q8_1", "B:p2 A:p0 C:p0 M:n N:n K:k st", fixed_type=6),
    Entry("qg_gemm_q5_1_q8_1", "B:p2 A:p0 C:p0 M:n N:n K:k st", fixed_type=7),
    Entry("qg_gemm_q8_0_q8_1", "B:p2 A:p0 C:p0 M:n N:n K:k st", fixed_type=8),
    # FP32 activations
    Entry("qg_gemm_w4a16", "A:p4 B:p2 C:p0 M:n N:n K:k st", fixed_type=2),
    Entry("qg_gemm_w8a16", "A:p4 B:p2 C:p0 M:n N:n K:k st", fixed_type=8),
    Entry("qg_gemm_q4_0_fp32", "B:p2 A:p4 C:p0 M:n N:n K:k st", fixed_type=2),
    Entry("qg_gemm_w4a16_ws", "A:p4 B:p2 C:p0 M:n N:n K:k ws:w wsb:z st", fixed_type=2),
    Entry("qg_gemm_w8a16_ws", "A:p4 B:p2 C:p0 M:n N:n K:k ws:w wsb:z st", fixed_type=8),
    # fused activation quantization: without a workspace X needs 16 B (qg.h); Q4_K needs the workspace
    Entry("qg_gemm_w4a8_f32", "A:p16 B:p2 C:p0 M:n N:n K:k wtype:t ws:w wsb:z st", ALL, q4k=Q4K_AL, ws_need="f32"),
    Entry("qg_gemm_q4_0_fp16_fused", "B:p2 A:p16 C:p0 M:n N:n K:k st", fixed_type=2),
    Entry("qg_gemm_q4_0_fp16_fused_ws", "B:p2 A:p16 C:p0 M:n N:n K:k ws:w wsb:z st", fixed_type=2, ws_need="f32"),
    Entry("qg_gemm_fp32", "A:p4 B:p4 C:p4 M:n N:n K:n st", fixed_type=0, k_free=True),
    # layout converters and quantizers
    Entry("qg_repack_weights", "B:p2 Bp:p16 N:n K:k wtype:t st"),
    Entry("qg_tile_weights", "B:p2 Bt:p16 N:n K:k wtype:t st"),
    Entry("qg_quantize_q8_1_padded", "x:p4 y:p4 M:n K:k st", fixed_type=9),
    Entry("qg_quantize_q8_1_tiled", "x:p16 y:p16 M:n K:k st", fixed_type=9),
    Entry("qg_tile_activations", "a:p4 y:p16 M:n K:k st", fixed_type=9),
    Entry("qg_quantize_q8_1_f16_fused", "x:p2 y:p4 k:c st", fixed_type=9),
    Entry("qg_quantize", "type:q variant:v x:p4 y:p2 k:c st"),
    Entry("qg_quantize_q8_1", "x:p4 y:p4 k:c st", fixed_type=9),
    Entry("qg_quantize_q4_0", "x:p4 y:p2 k:c st", fixed_type=2),
    Entry("qg_quantize_q8_1_definition", "x:p4 y:p4 k:c st", fixed_type=9),
    Entry("qg_quantize_q4_0_definition", "x:p4 y:p2 k:c st", fixed_type=2),
    Entry("qg_dequantize", "type:q x:p2 y:p4 k:c st"),
    Entry("qg_dequantize_q4_0", "x:p2 y:p4 k:c st", fixed_type=2),
]

GOOD = dict(n=2, k=256, t=2, a=0, b=2, st=None, z=1 << 30, c=256, q=2, v=0)


def baseline(e):
    args = {}
    for p in e.params:
        name, kind = p[0], p[-1] if len(p) == 1 else p[1]
        if name == "st":
            args[name] = None
        elif kind[0] in "pw":
            args[name] = 4096
        elif kind[0] == "l":
            args[name] = GOOD["n"]
        elif kind[0] == "s":
            args[name] = 1 << 16
        else:
            args[name] = GOOD[kind[0]]
    return args


def kind_of(e, name):
    for p in e.params:
        if p[0] == name:
            return "st" if name == "st" else p[1]
    raise KeyError(name)


def would_launch(e, a):
    """The tool's own reading of qg.h: does this call pass validation (and so reach a launch)? Such calls do
    not belong in the status half. Conservative towards keeping a case out."""
    names = [p[0] for p in e.params]
    sizes = [n for n in names if kind_of(e, n) in ("n", "c", "b")]
    if any(a[n] <= 0 for n in sizes if not (e.k_free and n == "K")) or (e.k_free and a["K"] < 0):
        return False
    wt = a.get("wtype", a.get("type", e.fixed_type))
    if "type" in a:  # qg_quantize / qg_dequantize
        ok = (2, 3, 6, 7, 8, 9) if e.name == "qg_quantize" else (2, 3, 6, 7, 8, 9, 12)
        if wt not in ok:
            return False
        gran = 256 if wt == 12 else 32
        if e.name == "qg_quantize" and a["variant"] not in ((0, 1, 2) if wt == 9 else (0, 2) if wt == 2 else (0,)):
            return False
        yal = {"y": 4 if wt == 9 else 2} if e.name == "qg_quantize" else {}
    else:
        if wt not in e.types and e.fixed_type is None:
            return False
        gran, yal = e.gran(a), {}
    kname = "K" if "K" in a else "k"
    if not e.k_free and (a[kname] <= 0 or a[kname] % gran):
        return False
    if a.get("algo", 0) not in (0,):  # an explicit algo can be refused for the shape: keep those cases out only
        if wt == 12 and a["algo"] in (3, 4):  # where the refusal is certain
            return False
    for n in names:
        kd = kind_of(e, n)
        if kd[0] == "p":
            if a[n] == 0:
                return False
            al = yal.get(n) or e.align(n, a)
            if e.ws_need == "prepacked" and (a["K"] // 32) % 8:
                al = 0  # padded rows: the MFMA route takes the pointers as they are
            if e.ws_need == "f32" and al == 16 and a.get("ws") and a["wsb"] >= ws_need(e, a):
                al = 2 if "fp16" in e.name else 4  # served through the workspace: the element's alignment
            if al and a[n] % al:
                return False
        if kd[0] == "l" and a[n] < a["N"]:
            return False
        if kd[0] == "s" and n != "st" and a["batch"] > 1 and int(kd[1:]) and a[n] % int(kd[1:]):
            return False
    if e.ws_need == "f32" and wt == 12 and (a.get("ws", 0) == 0 or a["wsb"] < ws_need(e, a) or a["ws"] % 4):
        return False
    if e.ws_need == "f32" and a.get("ws") and a["ws"] % 4 and a["M"] > 4:
        return False
    return True


def defects(e, full):
    """Single defects of an entry: (class, {param: value}). Classes order the precedence pairs."""
    out = []
    base = baseline(e)
    for p in e.params:
        name = p[0]
        kd = kind_of(e, name)
        if kd in ("n", "b") and not (e.k_free and name == "K"):
            out += [("neg", {name: -1}), ("empty", {name: 0})]
        elif kd == "n":  # qg_gemm_fp32's K: no granule, 0 passes
            out += [("neg", {name: -1})]
        elif kd in ("k", "c"):
            out += [("badk", {name: v}) for v in ((-32, 0, 33, 32, 288) if full else (-32, 0, 33, 288))]
        elif kd in ("t", "q"):
            out += [("type", {name: t}) for t in (TYPES + [0, 1, 5] if kd == "q" else TYPES) if t != base[name]]
        elif kd == "v":
            out += [("type", {name: v}) for v in (1, 2, 3)]
        elif kd == "a":
            out += [("algo", {name: v}) for v in (ALGOS[1:] + [7] if full else (1, 3, 7))]
        elif kd[0] == "p":
            out += [("null", {name: 0})]
            out += [("align", {name: 4096 + o}) for o in (1, 2, 4, 8)]
        elif kd == "l":
            out += [("ldc", {name: 1}), ("ldc", {name: 0}), ("ldc", {name: -1})]
        elif kd[0] == "s" and name != "st":
            out += [("stride", {name: (1 << 16) + 1}), ("stride", {name: (1 << 16) + 8})]
        elif kd == "w":
            out += [("ws", {name: 0}), ("ws", {name: 4097}), ("ws", {name: 4098}), ("ws", {"wsb": "need-1"}),
                    ("ws", {"wsb": 0})]
    return out


PAIRS = {("neg", "badk"), ("badk", "type"), ("type", "null"), ("null", "align"), ("neg", "type"), ("type", "align"),
         ("badk", "null"), ("ws", "null"), ("ws", "align"), ("ws", "type"), ("ldc", "badk"), ("ldc", "neg"),
         ("ldc", "type"), ("stride", "null"), ("stride", "badk"), ("stride", "type"), ("algo", "type"),
         ("algo", "badk"), ("algo", "null"), ("algo", "align")}


def ws_need(e, a):
    if e.ws_need == "prepacked":
        nb = a["K"] // 32
        nbp = (nb + 7) // 8 * 8
        return a["M"] * nbp * 36 if nbp != nb and a["M"] > 0 and a["K"] > 0 and a["K"] % 32 == 0 else 0
    rows = a["N"] if "fp16" in e.name else a["M"]  # the weight-major entry: N tokens
    return max(rows, 0) * max(a["K"] // 32, 0) * 36


def entry_cases(e, full):
    base = baseline(e)
    ds = defects(e, full)
    variants = [base]
    if e.q4k:  # the same defects around a Q4_K call
        variants.append(dict(base, wtype=12))
    if e.ws_need:  # shapes at which the workspace is what decides: K/32 odd, or more rows than the fused GEMV takes
        variants.append(dict(base, K=288, M=9, wsb="need"))
    seen = set()
    for vi, v in enumerate(variants):
        combos = [(d,) for d in ds]
        for d1, d2 in itertools.combinations(ds, 2):
            if set(d1[1]) & set(d2[1]):
                continue
            cl = (d1[0], d2[0])
            if full or "empty" in cl or cl in PAIRS or cl[::-1] in PAIRS:
                if not full and cl[0] == cl[1] and cl[0] != "empty":
                    continue
                combos.append((d1, d2))
        for combo in combos:
            a = dict(v)
            for _, ch in combo:
                a.update(ch)
            if isinstance(a.get("wsb"), str):
                a["wsb"] = max(ws_need(e, a) - (1 if a["wsb"] == "need-1" else 0), 0)
            if would_launch(e, a):
                continue
            key = tuple(a[p[0]] for p in e.params)
            if key not in seen:
                seen.add(key)
                yield e.name, key


# ---- the _from_view entries and qg_gemm_w4a8_grouped: structs, so cases are dicts of field overrides ------
def view_cases(full):
    for name, at, wts in (("qg_gemm_w4a8_from_view", 9, TYPES), ("qg_gemm_w4a16_from_view", 0, [2, 8, 3, 12, 0]),
                          ("qg_gemm_fp32_from_view", 0, [0, 2, 1])):
        good_w = wts[0]
        singles = [dict(kernel_type="bogus"), dict(kernel_type="gemv"), dict(null="act"), dict(null="w"), dict(null="out"),
                   dict(at=2), dict(at=1), dict(ot=2), dict(K=33), dict(K=0), dict(K=-32), dict(K=288), dict(wK=512),
                   dict(oN=3), dict(oM=3), dict(M=0), dict(N=0), dict(a_ne2=2), dict(w_ne3=2), dict(o_ne2=2),
                   dict(a_nb1=1), dict(w_nb1=2), dict(o_nb0=8), dict(o_nb1=4), dict(M=1 << 31), dict(data="act"),
                   dict(data="w"), dict(data="out"), dict(mis="w"), dict(mis="act")]
        singles += [dict(wt=t) for t in wts[1:]]
        combos = [s for s in singles]
        for s1, s2 in itertools.combinations(singles, 2):
            if set(s1) & set(s2):
                continue
            rej = lambda s: any(k in s for k in ("null", "at", "ot", "wK", "oN", "oM", "a_ne2", "w_ne3", "o_ne2", "a_nb1",
                                                 "w_nb1", "o_nb0", "o_nb1")) or s.get("kernel_type") == "bogus" \
                or s.get("K") in (33, 0, -32) or s.get("M", 0) > 4
            if full or (rej(s1) and rej(s2) and ("kernel_type" in s1 or "null" in s1 or "at" in s1 or "K" in s1)):
                combos.append({**s1, **s2})
        for c in combos:
            c = dict(c)
            c.setdefault("wt", good_w)
            c["act_t"] = c.pop("at", at)
            # keep out what passes validation: a well-formed view call launches
            k = c.get("K", 256)
            gran = 1 if name.startswith("qg_gemm_fp32") else 256 if c["wt"] == 12 and "w4a8" in name else 32
            ok_type = c["wt"] in (ALL if "w4a8" in name else (2, 8) if "w4a16" in name else (0,))
            structural = any(x in c for x in ("null", "ot", "wK", "oN", "oM", "a_ne2", "w_ne3", "o_ne2", "a_nb1", "w_nb1",
                                              "o_nb0", "o_nb1", "data")) or c["act_t"] != at or \
                c.get("kernel_type") == "bogus" or c.get("M", 1) == 0 or c.get("N", 1) == 0 or c.get("M", 1) > (1 << 30)
            if c.get("kernel_type") == "gemv" and "w4a8" not in name:
                structural = True
            al = (16 if c["wt"] == 12 else 2) if c.get("mis") == "w" else \
                ((4 if c["wt"] == 12 else 0) if "w4a8" in name else 4) if c.get("mis") == "act" else 0
            if not (structural or not ok_type or k <= 0 or k % gran or al > 1):
                continue
            yield name, tuple(sorted(c.items()))


def call_view(lib, name, fields):
    f = dict(fields)

    class View(ctypes.Structure):
        _fields_ = [("data", ctypes.c_void_p), ("type", ctypes.c_int), ("ne", ctypes.c_int64 * 4),
                    ("nb", ctypes.c_size_t * 4)]

    def row(t, k):
        if k <= 0:
            return 0
        return k * 4 if t == 0 else k * 2 if t == 1 else (k // 256) * 144 if t == 12 else \
            (k // 32) * {2: 18, 3: 20, 6: 22, 7: 24, 8: 34, 9: 36}.get(t, 0)

    M, N, K = f.get("M", 2), f.get("N", 4), f.get("K", 256)
    act, w, out = View(), View(), View()
    act.data = w.data = out.data = 4096
    act.type, w.type, out.type = f["act_t"], f["wt"], f.get("ot", 0)
    act.ne[:] = [K, M, f.get("a_ne2", 1), 1]
    w.ne[:] = [f.get("wK", K), N, 1, f.get("w_ne3", 1)]
    out.ne[:] = [f.get("oN", N), f.get("oM", M), f.get("o_ne2", 1), 1]
    act.nb[:] = [4, row(act.type, K) + f.get("a_nb1", 0), 0, 0]
    w.nb[:] = [4, row(w.type, K) + f.get("w_nb1", 0), 0, 0]
    out.nb[:] = [f.get("o_nb0", 4), max(N, 0) * 4 + f.get("o_nb1", 0), 0, 0]
    views = {"act": act, "w": w, "out": out}
    if "data" in f:
        views[f["data"]].data = None
    if "mis" in f:
        views[f["mis"]].data = 4097
    ptr = lambda k: None if f.get("null") == k else ctypes.byref(views[k])
    kt = f.get("kernel_type")
    return getattr(lib, name)(ptr("act"), ptr("w"), ptr("out"), kt.encode() if kt else None, None)


def grouped_cases():
    top = [dict(count=-1), dict(M=-1), dict(items_null=1), dict(K=33), dict(K=0), dict(K=-32), dict(wtype=12),
           dict(wtype=9), dict(wtype=99), dict(M=0), dict(count=0)]
    its = [dict(N=-1), dict(ldc=-1), dict(ldc=8), dict(A=0), dict(B=0), dict(C=0), dict(B=8193), dict(N=0, A=0)]
    for t in top:
        yield "qg_gemm_w4a8_grouped", (("top", tuple(sorted(t.items()))),)
    for which in (0, 1):  # the defect in the first or in the second of two items: nothing runs before all are checked
        for d in its:
            if d == dict(N=0, A=0):
                continue  # an empty item with a null pointer is skipped: the other item would launch
            yield "qg_gemm_w4a8_grouped", (("item", which, tuple(sorted(d.items()))),)
            for t in top:
                yield "qg_gemm_w4a8_grouped", (("item", which, tuple(sorted(d.items()))), ("top", tuple(sorted(t.items()))))
    # every item empty: a no-op whatever the pointers
    yield "qg_gemm_w4a8_grouped", (("item", 0, (("A", 0), ("N", 0))), ("item", 1, (("B", 0), ("N", 0))))


def call_grouped(lib, spec):
    class Item(ctypes.Structure):
        _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("N", ctypes.c_int),
                    ("ldc", ctypes.c_int)]

    items = (Item * 2)()
    for i in range(2):
        items[i].A, items[i].B, items[i].C, items[i].N, items[i].ldc = 4096, 1 << 20, 1 << 24, 64, 0
    top = dict(count=2, M=1, K=256, wtype=2)
    null_items = False
    for part in spec:
        if part[0] == "top":
            for k, v in part[1]:
                if k == "items_null":
                    null_items = True
                else:
                    top[k] = v
        else:
            for k, v in part[2]:
                setattr(items[part[1]], k, v or None if k in "ABC" else v)
    return lib.qg_gemm_w4a8_grouped(None if null_items else items, top["count"], top["M"], top["K"], top["wtype"], None)


def status_cases(full):
    for e in ENTRIES:
        yield from entry_cases(e, full)
    yield from view_cases(full)
    yield from grouped_cases()


def case_digest(cases):
    return hashlib.sha256(repr(cases).encode()).hexdigest()[:16]


# ---- running a library (child process) --------------------------------------------------------------------
def signatures():
    # _lib.py by path: the signatures, and torch (whose HIP runtime the library binds to), without the
    # package's __init__, which would load the in-tree library next to the one under test
    if "_qg_lib_signatures" not in sys.modules:
        import importlib.util
        spec = importlib.util.spec_from_file_location(
            "_qg_lib_signatures", os.path.join(REPO, "llama.cpp-quant-gemm_amd", "quant_gemm", "_lib.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_qg_lib_signatures"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["_qg_lib_signatures"].SIGNATURES


def load_library(path):
    lib = ctypes.CDLL(path)
    for name, (args, res) in signatures().items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


def visible_devices():
    """The HIP runtime's device count (the runtime torch loaded; no call into the library under test)."""
    signatures()
    for soname in ("libamdhip64.so.7", "libamdhip64.so"):
        try:
            hip = ctypes.CDLL(soname)
            break
        except OSError:
            continue
    else:
        raise RuntimeError("HIP runtime not found")
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


def run_dispatch(lib, cases):
    buf = ctypes.create_string_buffer(512)
    out = []
    for name, args in cases:
        fn = getattr(lib, name)
        if name.startswith("qg_debug_config"):
            st = fn(*args, buf, 512)
            out.append([st, buf.value.decode()])
        else:
            out.append([fn(*args), ""])
    return out


def run_status(lib, cases):
    out = []
    for name, args in cases:
        if name.endswith("_from_view"):
            out.append(call_view(lib, name, args))
        elif name == "qg_gemm_w4a8_grouped":
            out.append(call_grouped(lib, args))
        else:
            out.append(getattr(lib, name)(*args))
    return out


def child_main(path, full):
    ndev = visible_devices()  # before any library call
    lib = load_library(path)
    grid = FULL if full else COMMITTED
    res = {"devices": ndev, "dispatch": run_dispatch(lib, list(dispatch_cases(grid)))}
    if ndev == 0:
        res["status"] = run_status(lib, list(status_cases(full)))
    json.dump(res, sys.stdout)


def run_child(path, full):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path)] + (["--full"] if full else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"api_matrix child failed ({p.returncode}) for {path}:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout)


# ---- fixture: the unique results in the clear, the per-case ids packed (JSON list, zlib, base64) ------------
def pack(ids):
    return base64.b64encode(zlib.compress(json.dumps(ids, separators=(",", ":")).encode(), 9)).decode()


def unpack(blob):
    return json.loads(zlib.decompress(base64.b64decode(blob)))


def record(path):
    res = run_child(path, full=False)
    if res["devices"]:
        raise SystemExit("a device is visible to the child: the status half was not run, nothing recorded")
    dcases, scases = list(dispatch_cases(COMMITTED)), list(status_cases(False))
    launched = [c for c, r in zip(scases, res["status"]) if r == ERR_HIP]
    for c in launched[:40]:
        print("reached a launch (fix the grid):", c)
    table, ids = [], []
    for r in res["dispatch"]:
        if r not in table:
            table.append(r)
        ids.append(table.index(r))
    fix = {"dispatch_cases": len(dcases), "dispatch_digest": case_digest(dcases), "status_cases": len(scases),
           "status_digest": case_digest(scases), "dropped_launching": len(launched), "results": table,
           "dispatch": pack(ids), "status": pack(res["status"])}
    with open(GOLDEN, "w") as f:
        json.dump(fix, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"recorded {len(dcases)} dispatch + {len(scases)} status cases, {len(launched)} dropped, "
          f"{os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")
    return 1 if launched else 0


def check(path):
    """Replay the committed grid against `path`; returns (differences, skipped_status_reason)."""
    fix = json.load(open(GOLDEN))
    dcases, scases = list(dispatch_cases(COMMITTED)), list(status_cases(False))
    assert (len(dcases), case_digest(dcases)) == (fix["dispatch_cases"], fix["dispatch_digest"]), "dispatch grid changed"
    assert (len(scases), case_digest(scases)) == (fix["status_cases"], fix["status_digest"]), "status grid changed"
    res = run_child(path, full=False)
    want = [fix["results"][i] for i in unpack(fix["dispatch"])]
    diffs = [("dispatch", c, w, g) for c, w, g in zip(dcases, want, res["dispatch"]) if w != g]
    skipped = None
    if "status" in res:
        diffs += [("status", c, w, g) for c, w, g in zip(scases, unpack(fix["status"]), res["status"]) if w != g]
    else:
        skipped = f"{res['devices']} device(s) visible despite HIP_VISIBLE_DEVICES=-1: fake-pointer calls not made"
    return diffs, skipped, fix


def compare(a, b):
    ra, rb = run_child(a, full=True), run_child(b, full=True)
    dcases, scases = list(dispatch_cases(FULL)), list(status_cases(True))
    diffs = [("dispatch", c, x, y) for c, x, y in zip(dcases, ra["dispatch"], rb["dispatch"]) if x != y]
    n = len(dcases)
    if "status" in ra and "status" in rb:
        diffs += [("status", c, x, y) for c, x, y in zip(scases, ra["status"], rb["status"]) if x != y]
        n += len(scases)
        launched = sum(1 for r in ra["status"] if r == ERR_HIP)
        print(f"status half: {len(scases)} cases, {launched} reached a launch in A (compared all the same)")
    else:
        print("status half not run: a device is visible")
    for d in diffs[:200]:
        print("DIFF", *d)
    print(f"{n} cases compared ({len(dcases)} dispatch), {len(diffs)} differences")
    return 1 if diffs else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", metavar="LIB")
    ap.add_argument("--check", metavar="LIB")
    ap.add_argument("--compare", nargs=2, metavar=("A.so", "B.so"))
    ap.add_argument("--child", metavar="LIB", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_main(a.child, a.full)
    if a.record:
        return record(a.record)
    if a.compare:
        return compare(*a.compare)
    if a.check:
        diffs, skipped, _ = check(a.check)
        for d in diffs[:200]:
            print("DIFF", *d)
        print(f"{len(diffs)} differences" + (f"; {skipped}" if skipped else ""))
        return 1 if diffs else 0
    ap.error("nothing to do")


if __name__ == "__main__":
    sys.exit(main())
