#!/usr/bin/env python3
"""Q6_K against Q4_K and Q8_0 through qg_gemm_w4a8 in one process, timed as bench.py does: G launches over
rotating resident weight copies (> 600 MB) in a hipGraph, HIP events on the launch stream, interleaved rounds
(measurement tool, not product). Bytes per weight element: Q4_K 0.5625, Q6_K 0.8203, Q8_0 1.0625.
  python tools/ab_q6k.py [--shapes 1x4096x4096,...] [--rounds 7] [--out profiles/q6k/ab_q6k.txt]
  python tools/ab_q6k.py --threshold 5,8,9,16 [--out profiles/q6k/ab_q6k_threshold.txt]
  python tools/ab_q6k.py --libs tools/variants/libqg_asum.so    (a variant build's Q6_K product in the same rounds)
Shapes are MxNxK: M tokens, N weight rows. --threshold: the forced decode GEMV (QG_ALGO_GEMV, M <= 8 only) against
the forced MFMA prefill (QG_ALGO_MFMA) of Q6_K at N = K = 4096, interleaved the same way."""
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

DEFAULT = "1x4096x4096,4x4096x4096,8x4096x4096,9x4096x4096,32x4096x4096,512x4096x4096,1x4096x14336"
TYPES = (("Q6_K", qg.Q6_K), ("Q4_K", qg.Q4_K), ("Q8_0", qg.Q8_0))
# Captured Q8_0 GEMVs of M <= 4 merge into one grouped node (qg.h at qg_gemm_w4a8); Q4_K and Q6_K never do. This
# column times Q8_0 with the merge off, kernel node against kernel node.
UNMERGED = "Q8_0(nodes)"


def random_kquant(t: int, n: int, k: int, gen: torch.Generator, dev: torch.device) -> torch.Tensor:
    """[n, k/256, block bytes] with uniform bytes and small finite f16 scales (the timing does not depend on the
    values; the products are checked by tests/test_gpu_q6k.py and tests/test_gpu_q4k.py)."""
    bb = qg.BLOCK_BYTES[t]
    w = torch.randint(0, 256, (n, k // 256, bb), generator=gen, device=dev, dtype=torch.uint8)
    d = ((torch.rand((n, k // 256, 2), generator=gen, device=dev) * 2 - 1) * 0.01).to(torch.float16).view(torch.uint8)
    if t == qg.Q4_K:
        w[..., 0:4] = d.reshape(n, k // 256, 4)
    else:
        w[..., 208:210] = d.reshape(n, k // 256, 4)[..., 0:2]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--libs", nargs="*", default=[],
                    help="variant builds of libqg_hip.so (make BUILD=build_<tag> OUT=... EXTRA=-D...): their Q6_K "
                         "product is timed in the same rounds and compared bit for bit")
    a = ap.parse_args()
    import ctypes
    P = ctypes.c_void_p
    variants = {}
    for path in a.libs:
        lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        lib.qg_gemm_w4a8.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        variants["Q6_K@" + os.path.basename(path).replace("libqg_", "").replace(".so", "")] = lib.qg_gemm_w4a8
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per launch, median of {a.rounds} interleaved rounds (min), G={a.G} launches per "
             "graph over rotating weight copies > 600 MB"]
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    if a.threshold:
        N = K = 4096
        gen = torch.Generator(device=dev)
        gen.manual_seed(N + K)
        cp = rotating(random_kquant(qg.Q6_K, N, K, gen, dev), a.G)
        for M in (int(x) for x in a.threshold.split(",")):
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)
            algos = [("gemv", qg.ALGO_GEMV)] * (M <= 8) + [("mfma", qg.ALGO_MFMA)]
            times = {n: [] for n, _ in algos}
            for _ in range(a.rounds):
                for name, algo in algos:
                    run = lambda: [qg.gemm_w4a8(aq, cp[j], M, N, K, qg.Q6_K, algo, out=out[j]) for j in range(a.G)]
                    times[name].append(graph_time_us(run, 10, a.G))
            emit(f"M={M} N={N} K={K}: " + "  ".join(
                f"{n} {statistics.median(v):.3f} us (min {min(v):.3f}) [{qg.debug_config(M, N, K, qg.Q6_K, algo=al)}]"
                for (n, al), v in zip(algos, times.values())) + f"  auto: {qg.debug_config(M, N, K, qg.Q6_K).split()[0]}")
            del out
    else:
        for spec in a.shapes.split(","):
            M, N, K = (int(x) for x in spec.split("x"))
            gen = torch.Generator(device=dev)
            gen.manual_seed(M + N + K)
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            copies = {}
            for name, t in TYPES:
                w = qg.quantize(torch.rand((N, K), generator=gen, device=dev) * 2 - 1, t) if t == qg.Q8_0 \
                    else random_kquant(t, N, K, gen, dev)
                copies[name] = rotating(w, a.G)
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)

            def step_of(name, t):
                if name in variants:
                    f, cp = variants[name], copies["Q6_K"]

                    def run():
                        cs = P(torch.cuda.current_stream().cuda_stream)
                        for j in range(a.G):
                            rc = f(P(aq.data_ptr()), P(cp[j].data_ptr()), P(out[j].data_ptr()), M, N, K, qg.Q6_K, cs)
                            if rc != 0:
                                raise RuntimeError(f"{name}: status {rc}")
                    return run
                if name == UNMERGED:  # Q8_0 as 64 kernel nodes, the form Q4_K and Q6_K are captured in
                    cp = copies["Q8_0"]

                    def run_nodes():
                        qg.set_capture_fusion(0)
                        try:
                            for j in range(a.G):
                                qg.gemm_w4a8(aq, cp[j], M, N, K, t, out=out[j])
                        finally:
                            qg.set_capture_fusion(1)
                    return run_nodes
                cp = copies[name]
                return lambda: [qg.gemm_w4a8(aq, cp[j], M, N, K, t, out=out[j]) for j in range(a.G)]

            runs = list(TYPES) + [(UNMERGED, qg.Q8_0)] + [(n, qg.Q6_K) for n in variants]
            times = {name: [] for name, _ in runs}
            for _ in range(a.rounds):
                for name, t in runs:
                    times[name].append(graph_time_us(step_of(name, t), 10, a.G))
            med = {n: statistics.median(v) for n, v in times.items()}
            ref = qg.gemm_w4a8(aq, copies["Q6_K"][0], M, N, K, qg.Q6_K)
            same = {}
            for name in variants:  # each variant's output against the in-tree library's
                step_of(name, qg.Q6_K)()
                torch.cuda.synchronize()
                same[name] = "==" if torch.equal(out[0], ref) else "max|d| %.3g" % float((out[0] - ref).abs().max())
            gbs = N * K * 0.8203125 / med["Q6_K"] / 1e3  # weight bytes only
            emit(f"M={M} N={N} K={K}: " + "  ".join(f"{n} {med[n]:.3f} us (min {min(times[n]):.3f})" for n, _ in runs) +
                 f"  Q6_K/Q4_K {med['Q6_K'] / med['Q4_K']:.3f}  Q6_K/Q8_0 {med['Q6_K'] / med['Q8_0']:.3f}"
                 f"  Q6_K/{UNMERGED} {med['Q6_K'] / med[UNMERGED]:.3f}"
                 f"  Q6_K weights {gbs:.0f} GB/s  cfg {qg.debug_config(M, N, K, qg.Q6_K)}" + (f"  variants vs in-tree: {same}" if same else ""))
            del copies, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
