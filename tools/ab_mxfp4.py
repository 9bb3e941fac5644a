#!/usr/bin/env python3
"""MXFP4 against Q4_0 and Q4_K through qg_gemm_w4a8 in one process, timed as bench.py does: G launches over rotating
resident weight copies (> 600 MB) in a hipGraph, HIP events on the launch stream, interleaved rounds (measurement tool,
not product). Bytes per weight element: MXFP4 0.53125, Q4_0 0.5625, Q4_K 0.5625.
  python tools/ab_mxfp4.py [--shapes 1x4096x4096,...] [--rounds 7] [--out profiles/mxfp4/ab_mxfp4.txt]
  python tools/ab_mxfp4.py --threshold 5,8 [--out profiles/mxfp4/ab_mxfp4_threshold.txt]
  python tools/ab_mxfp4.py --moe 32,128 [--out profiles/mxfp4/ab_mxfp4_moe.txt]
  python tools/ab_mxfp4.py --libs tools/variants/libqg_ub2.so    (a variant build's MXFP4 product in the same rounds:
      make -C llama.cpp-quant-gemm_amd/csrc BUILD=build_ub2 OUT=../../tools/variants/libqg_ub2.so \
           EXTRA=-DQG_MXFP4_UNIT_BLOCKS=2 ../../tools/variants/libqg_ub2.so)
Shapes are MxNxK: M tokens, N weight rows. Captured Q4_0 GEMVs of M <= 4 would merge into one grouped node; MXFP4 and
Q4_K never do, so Q4_0 is timed with the merge off, kernel node against kernel node.
--threshold: the forced decode GEMV (QG_ALGO_GEMV, M <= 8 only) against the forced MFMA prefill (QG_ALGO_MFMA) of MXFP4
at N = K = 4096, interleaved the same way.
--moe: qg_gemm_w4a8_moe with that many MXFP4 experts at gpt-oss's shape (4 used, N = K = 2880), T = 1 and 8, a uniform
router, per slot, against one eager kernel node per slot with the ids on the host (all a caller could do otherwise)."""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from bench import graph_time_us  # noqa: E402

DEFAULT = ("1x4096x4096,4x4096x4096,8x4096x4096,32x4096x4096,512x4096x4096,1x4096x14336,4x4096x14336,"
           "1x2880x2880,4x2880x2880")
TYPES = (("MXFP4", qg.MXFP4), ("Q4_0", qg.Q4_0), ("Q4_K", qg.Q4_K))


def random_weights(t: int, n: int, k: int, gen: torch.Generator, dev: torch.device) -> torch.Tensor:
    """[n, k/bs, block bytes] with uniform code bytes and small finite scales (the timing does not depend on the values;
    the products are checked by the GPU tests). K off Q4_K's 256-element granule: None."""
    be = qg.block_elems(t)
    if k % be:
        return None
    if t == qg.Q4_0:
        return qg.quantize(torch.rand((n, k), generator=gen, device=dev) * 2 - 1, t)
    w = torch.randint(0, 256, (n, k // be, qg.BLOCK_BYTES[t]), generator=gen, device=dev, dtype=torch.uint8)
    if t == qg.MXFP4:
        w[..., 0] = torch.randint(110, 136, (n, k // be), generator=gen, device=dev, dtype=torch.uint8)
    else:
        d = ((torch.rand((n, k // be, 2), generator=gen, device=dev) * 2 - 1) * 0.01).to(torch.float16).view(torch.uint8)
        w[..., 0:4] = d.reshape(n, k // be, 4)
    return w


def rotating(w: torch.Tensor, G: int) -> torch.Tensor:
    R = max(G, math.ceil(600e6 / w.numel()))
    c = torch.empty((R,) + tuple(w.shape), dtype=torch.uint8, device=w.device)
    c.copy_(w.unsqueeze(0).expand_as(c))
    return c


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--threshold", default=None, help="comma-separated M: forced GEMV against forced MFMA, N = K = 4096")
    ap.add_argument("--moe", default=None, help="comma-separated expert counts: the expert entry at gpt-oss's shape")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--libs", nargs="*", default=[],
                    help="variant builds of libqg_hip.so: their MXFP4 product is timed in the same rounds and compared "
                         "bit for bit with the in-tree library's")
    a = ap.parse_args()
    import ctypes
    P = ctypes.c_void_p
    variants = {}
    for path in a.libs:
        lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        lib.qg_gemm_w4a8.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        variants["MXFP4@" + os.path.basename(path).replace("libqg_", "").replace(".so", "")] = lib.qg_gemm_w4a8
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per launch, median of {a.rounds} interleaved rounds (min), G={a.G} launches per "
             "graph over rotating weight copies > 600 MB"]
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    gen = torch.Generator(device=dev)
    if a.threshold:
        N = K = 4096
        gen.manual_seed(N + K)
        cp = rotating(random_weights(qg.MXFP4, N, K, gen, dev), a.G)
        for M in (int(x) for x in a.threshold.split(",")):
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)
            algos = [("gemv", qg.ALGO_GEMV)] * (M <= 8) + [("mfma", qg.ALGO_MFMA)]
            times = {n: [] for n, _ in algos}
            for _ in range(a.rounds):
                for name, algo in algos:
                    run = lambda: [qg.gemm_w4a8(aq, cp[j], M, N, K, qg.MXFP4, algo, out=out[j]) for j in range(a.G)]
                    times[name].append(graph_time_us(run, 10, a.G))
            emit(f"M={M} N={N} K={K}: " + "  ".join(
                f"{n} {statistics.median(v):.3f} us (min {min(v):.3f}) [{qg.debug_config(M, N, K, qg.MXFP4, algo=al)}]"
                for (n, al), v in zip(algos, times.values())) + f"  auto: {qg.debug_config(M, N, K, qg.MXFP4).split()[0]}")
            del out
    elif a.moe:
        n_used, N, K = 4, 2880, 2880
        for n_expert in (int(x) for x in a.moe.split(",")):
            gen.manual_seed(n_expert)
            w = random_weights(qg.MXFP4, n_expert * N, K, gen, dev).reshape(n_expert, N, K // 32, 17)
            R = max(2, math.ceil(600e6 / w.numel()))  # rotating copies of the whole expert set
            cp = torch.empty((R,) + tuple(w.shape), dtype=torch.uint8, device=dev)
            cp.copy_(w.unsqueeze(0).expand_as(cp))
            for T in (1, 8):
                slots = T * n_used
                aq = qg.quantize_q8_1(torch.rand((T, 1, K), generator=gen, device=dev) * 2 - 1)
                ids = torch.randint(0, n_expert, (a.G, T, n_used), generator=gen, device=dev, dtype=torch.int32)
                ids_h = ids.cpu().tolist()
                out = torch.empty((T, n_used, N), dtype=torch.float32, device=dev)

                def one():  # a launch per step, ids on the device
                    for j in range(a.G):
                        qg.gemm_w4a8_moe(aq, cp[j % R], ids[j], T, n_used, N, K, qg.MXFP4, out=out)

                def per_slot():  # a kernel node per slot, ids on the host
                    for j in range(a.G):
                        for t in range(T):
                            for u in range(n_used):
                                qg.gemm_w4a8(aq[t], cp[j % R][ids_h[j][t][u]], 1, N, K, qg.MXFP4, out=out[t, u:u + 1])

                times = {"moe": [], "nodes": []}
                for _ in range(a.rounds):
                    times["moe"].append(graph_time_us(one, 10, a.G * slots))
                    times["nodes"].append(graph_time_us(per_slot, 10, a.G * slots))
                med = {n: statistics.median(v) for n, v in times.items()}
                emit(f"experts={n_expert} used={n_used} T={T} N={N} K={K}: per slot  moe {med['moe']:.3f} us (min "
                     f"{min(times['moe']):.3f})  one node per slot {med['nodes']:.3f} us (min {min(times['nodes']):.3f})  "
                     f"moe/nodes {med['moe'] / med['nodes']:.3f}  cfg {qg.moe_config(T, n_used, N, K, qg.MXFP4)}")
                del out
            del cp, w
    else:
        for spec in a.shapes.split(","):
            M, N, K = (int(x) for x in spec.split("x"))
            gen.manual_seed(M + N + K)
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            copies = {}
            for name, t in TYPES:
                w = random_weights(t, N, K, gen, dev)
                if w is not None:
                    copies[name] = rotating(w, a.G)
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)

            def step_of(name, t):
                if name in variants:
                    f, vc = variants[name], copies["MXFP4"]

                    def run_variant():
                        cs = P(torch.cuda.current_stream().cuda_stream)
                        for j in range(a.G):
                            rc = f(P(aq.data_ptr()), P(vc[j].data_ptr()), P(out[j].data_ptr()), M, N, K, qg.MXFP4, cs)
                            if rc != 0:
                                raise RuntimeError(f"{name}: status {rc}")
                    return run_variant
                cp = copies[name]

                def run():
                    qg.set_capture_fusion(0)  # Q4_0 as kernel nodes, the form MXFP4 and Q4_K are captured in
                    try:
                        for j in range(a.G):
                            qg.gemm_w4a8(aq, cp[j], M, N, K, t, out=out[j])
                    finally:
                        qg.set_capture_fusion(1)
                return run

            runs = [(n, t) for n, t in TYPES if n in copies] + [(n, qg.MXFP4) for n in variants]
            times = {name: [] for name, _ in runs}
            for _ in range(a.rounds):
                for name, t in runs:
                    times[name].append(graph_time_us(step_of(name, t), 10, a.G))
            med = {n: statistics.median(v) for n, v in times.items()}
            ref = qg.gemm_w4a8(aq, copies["MXFP4"][0], M, N, K, qg.MXFP4)
            same = {}
            for name in variants:  # each variant's output against the in-tree library's
                step_of(name, qg.MXFP4)()
                torch.cuda.synchronize()
                same[name] = "==" if torch.equal(out[0], ref) else "max|d| %.3g" % float((out[0] - ref).abs().max())
            gbs = N * K * 0.53125 / med["MXFP4"] / 1e3  # weight bytes only
            emit(f"M={M} N={N} K={K}: " + "  ".join(f"{n} {med[n]:.3f} us (min {min(times[n]):.3f})" for n, _ in runs) +
                 "".join(f"  MXFP4/{n} {med['MXFP4'] / med[n]:.3f}" for n, _ in runs[1:]) +
                 f"  MXFP4 weights {gbs:.0f} GB/s  cfg {qg.debug_config(M, N, K, qg.MXFP4)}" +
                 (f"  variants vs in-tree: {same}" if same else ""))
            del copies, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
