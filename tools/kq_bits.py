#!/usr/bin/env python3
"""Bit identity of the K-quant products and sumi between another build of the library and the in-tree one, both
loaded in this process (measurement tool, not product).
  make -C llama.cpp-quant-gemm_amd/csrc BUILD=build_parent OUT=../../tools/variants/libqg_parent.so \
       ../../tools/variants/libqg_parent.so                      (in a checkout of the commit to compare against)
  python tools/kq_bits.py [--lib tools/variants/libqg_parent.so] [--out profiles/kq_shared/bits.txt]
Every product shape of tests/test_gpu_q6k.py, tests/test_gpu_q4k.py and the forms / edges of
tests/test_gpu_q4k_paths.py, the extremes, the pointer-offset and fuzz cases, the forced families; per case the
status codes, both qg_debug_config strings, the bits of qg_gemm_w4a8_ex and of qg_debug_sumi."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))

import kquant_ref as KR  # noqa: E402
import q6k_ref as QR  # noqa: E402

P, I = ctypes.c_void_p, ctypes.c_int
Q4_K, Q6_K = 12, 14


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    lib.qg_gemm_w4a8_ex.argtypes = [P, P, P, I, I, I, I, I, P]
    lib.qg_debug_sumi.argtypes = [P, P, P, I, I, I, I, I, P]
    lib.qg_debug_config.argtypes = [I, I, I, I, I, I, ctypes.c_char_p, ctypes.c_size_t]
    return lib


def cfg(lib, m, n, k, t, algo, sumi):
    buf = ctypes.create_string_buffer(256)
    lib.qg_debug_config(m, n, k, t, algo, sumi, buf, 256)
    return buf.value.decode()


def q4k_cases():
    import importlib
    T = importlib.import_module("test_gpu_q4k")
    shapes = list(T.GEMV_SHAPES) + list(T.MMQ_SHAPES)
    shapes += [(m, 70, k) for m in (1, 3, 6, 7) for k in (256, 768, 1024, 1280, 4096, 4352)]
    shapes += [(2, n, k) for k in (256, 768, 1024, 1280, 4096, 4352) for n in (1, 15, 17, 33, 63, 65)]
    shapes += [(8, 40, 6400), (8, 24, 14336), (8, 20, 15616), (5, 20, 25088)]
    shapes += [(65, 8200, k) for k in (768, 1024, 1280)]
    shapes += [(9, 1, 512), (16, 15, 256), (20, 17, 768), (9, 32, 4096), (200, 48, 512), (31, 33, 2304)]
    for m, n, k in shapes:
        rng = np.random.default_rng([m, n, k, 0])
        bq, aq = KR.random_q4k(rng, n, k), KR.random_q8_1(rng, m, k)
        yield f"shape {m}x{n}x{k}", aq, bq, 0, 0, (0,)
    for m in (2, 12, 16):
        aq, bq = KR.extremes(np.random.default_rng([6, m]), m)
        yield f"extremes m={m}", aq, bq, 0, 0, (0,)
    for i, m, n, k, woff, aoff in KR.fuzz_cases():
        rng = np.random.default_rng([m, n, k, i])
        bq, aq = KR.random_q4k(rng, n, k), KR.random_q8_1(rng, m, k)
        yield f"fuzz {i} {m}x{n}x{k} +{woff}/+{aoff}", aq, bq, woff, aoff, (0,)
    for m in (4, 8):  # the forced families either side of the threshold
        rng = np.random.default_rng([m, 200, 1024, 0])
        bq, aq = KR.random_q4k(rng, 200, 1024), KR.random_q8_1(rng, m, 1024)
        yield f"forced {m}x200x1024", aq, bq, 0, 0, (1, 2)


def q6k_cases():
    import importlib
    T = importlib.import_module("test_gpu_q6k")
    for m, n, k in T.all_product_shapes():
        rng = np.random.default_rng([m, n, k, 0])
        bq, aq = QR.random_q6k(rng, n, k), QR.random_q8_1(rng, m, k)
        yield f"shape {m}x{n}x{k}", aq, bq, 0, 0, (0,)
    for m in (3, 12):
        aq, bq = QR.extremes(np.random.default_rng([7, m]), m, 16, 512)
        yield f"extremes m={m}", aq, bq, 0, 0, (0,)
    for m, n, k in ((3, 33, 768), (17, 17, 768)):
        rng = np.random.default_rng([m, n, k, 0])
        bq, aq = QR.random_q6k(rng, n, k), QR.random_q8_1(rng, m, k)
        for woff, aoff in ((2, 4), (18, 8), (2, 12), (18, 4)):
            yield f"offsets {m}x{n}x{k} +{woff}/+{aoff}", aq, bq, woff, aoff, (0,)
    for i, m, n, k, woff, aoff in QR.fuzz_cases():
        rng = np.random.default_rng([m, n, k, i])
        bq, aq = QR.random_q6k(rng, n, k), QR.random_q8_1(rng, m, k)
        yield f"fuzz {i} {m}x{n}x{k} +{woff}/+{aoff}", aq, bq, woff, aoff, (0,)
    rng = np.random.default_rng([8, 33, 768, 0])
    bq, aq = QR.random_q6k(rng, 33, 768), QR.random_q8_1(rng, 8, 768)
    yield "forced 8x33x768", aq, bq, 0, 0, (1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "tools", "variants", "libqg_parent.so"))
    ap.add_argument("--out", default=os.devnull, help="one line per case, then the instantiations reached")
    a = ap.parse_args()
    parent = load(a.lib)
    result = load(os.path.join(REPO, "llama.cpp-quant-gemm_amd", "quant_gemm", "libqg_hip.so"))
    out = open(a.out, "w")
    st = P(torch.cuda.current_stream().cuda_stream)
    total = bad = 0
    seen = set()
    for tname, t, cases in (("Q4_K", Q4_K, q4k_cases()), ("Q6_K", Q6_K, q6k_cases())):
        for name, aq, bq, woff, aoff, algos in cases:
            m, nb = aq.shape[:2]
            n, k = bq.shape[0], 32 * nb
            a, b = KR.dev_at(aq, aoff), KR.dev_at(bq, woff)
            for algo in algos:
                got = []
                for lib in (parent, result):
                    c = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
                    s = torch.full((m, n, nb), -7, dtype=torch.int32, device="cuda")
                    rc = lib.qg_gemm_w4a8_ex(P(a.data_ptr()), P(b.data_ptr()), P(c.data_ptr()), m, n, k, t, algo, st)
                    rs = lib.qg_debug_sumi(P(a.data_ptr()), P(b.data_ptr()), P(s.data_ptr()), m, n, k, t, algo, st)
                    torch.cuda.synchronize()
                    got.append((rc, rs, c.view(torch.int32), s, cfg(lib, m, n, k, t, algo, 0), cfg(lib, m, n, k, t, algo, 1)))
                (rc0, rs0, c0, s0, f0, g0), (rc1, rs1, c1, s1, f1, g1) = got
                same = (rc0, rs0, f0, g0) == (rc1, rs1, f1, g1) and torch.equal(c0, c1) and torch.equal(s0, s1)
                total += 1
                bad += not same
                seen.add(f0.split(" grid")[0])
                line = f"{'same' if same else 'DIFF'} {tname} {name} algo={algo} rc={rc1}/{rs1} [{f1}]"
                print(line, file=out, flush=True)
                if not same:
                    print(line, flush=True)
    tail = f"{total} cases, {bad} differing; {len(seen)} instantiations reached"
    print(tail, file=out)
    for s in sorted(seen):
        print("  reached:", s, file=out)
    print(tail)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
