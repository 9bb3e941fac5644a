#!/usr/bin/env python3
"""Q4_K against Q4_0 and Q5_1 through qg_gemm_w4a8 in one process, timed as bench.py does: G launches over
rotating resident weight copies (> 600 MB) in a hipGraph, HIP events on the launch stream, interleaved rounds
(measurement tool, not product). Q4_K streams the Q4_0 byte count; Q5_1 streams a third more with dot4 arithmetic.
  python tools/ab_q4k.py [--shapes 1x4096x4096,...] [--rounds 7] [--out profiles/q4k/ab_q4k.txt]
Shapes are MxNxK: M tokens, N weight rows."""
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

DEFAULT = "1x4096x4096,4x4096x4096,8x4096x4096,32x4096x4096,512x4096x4096,1x4096x14336,4x4096x14336"
TYPES = (("Q4_K", qg.Q4_K), ("Q4_0", qg.Q4_0), ("Q5_1", qg.Q5_1))


def random_q4k(n: int, k: int, gen: torch.Generator, dev: torch.device) -> torch.Tensor:
    """[n, k/256, 144] with uniform scales / qs bytes, d in +-0.01, dmin in +-0.05 (the timing does not depend on
    the values; the product is checked by tests/test_gpu_q4k.py)."""
    w = torch.randint(0, 256, (n, k // 256, 144), generator=gen, device=dev, dtype=torch.uint8)
    d = (torch.rand((n, k // 256, 2), generator=gen, device=dev) * 2 - 1) * torch.tensor([0.01, 0.05], device=dev)
    w[..., 0:4] = d.to(torch.float16).view(torch.uint8).reshape(n, k // 256, 4)
    return w


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--libs", nargs="*", default=[],
                    help="variant builds of libqg_hip.so (make BUILD=build_<tag> OUT=... EXTRA=-D...): their Q4_K "
                         "product is timed in the same rounds and compared bit for bit")
    a = ap.parse_args()
    import ctypes
    P = ctypes.c_void_p
    variants = {}
    for path in a.libs:
        lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        lib.qg_gemm_w4a8.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        variants["Q4_K@" + os.path.basename(path).replace("libqg_", "").replace(".so", "")] = lib.qg_gemm_w4a8
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per launch, median of {a.rounds} interleaved rounds (min), G={a.G} launches per "
             "graph over rotating weight copies > 600 MB"]
    print(lines[0], flush=True)
    for spec in a.shapes.split(","):
        M, N, K = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(M + N + K)
        x = torch.rand((M, K), generator=gen, device=dev) * 2 - 1
        aq = qg.quantize_q8_1(x)
        copies = {}
        for name, t in TYPES:
            w = random_q4k(N, K, gen, dev) if t == qg.Q4_K else qg.quantize(
                torch.rand((N, K), generator=gen, device=dev) * 2 - 1, t)
            R = max(a.G, math.ceil(600e6 / w.numel()))
            c = torch.empty((R,) + tuple(w.shape), dtype=torch.uint8, device=dev)
            c.copy_(w.unsqueeze(0).expand_as(c))
            copies[name] = c
        out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)

        def step_of(name, t):
            if name in variants:
                f, cp = variants[name], copies["Q4_K"]

                def run():
                    cs = P(torch.cuda.current_stream().cuda_stream)
                    for j in range(a.G):
                        rc = f(P(aq.data_ptr()), P(cp[j].data_ptr()), P(out[j].data_ptr()), M, N, K, qg.Q4_K, cs)
                        if rc != 0:
                            raise RuntimeError(f"{name}: status {rc}")
                return run
            cp = copies[name]
            return lambda: [qg.gemm_w4a8(aq, cp[j], M, N, K, t, out=out[j]) for j in range(a.G)]

        runs = list(TYPES) + [(n, qg.Q4_K) for n in variants]
        times = {name: [] for name, _ in runs}
        for _ in range(a.rounds):
            for name, t in runs:
                times[name].append(graph_time_us(step_of(name, t), 10, a.G))
        med = {n: statistics.median(v) for n, v in times.items()}
        ref = qg.gemm_w4a8(aq, copies["Q4_K"][0], M, N, K, qg.Q4_K)
        same = {}
        for name in variants:  # each variant's output against the in-tree library's
            step_of(name, qg.Q4_K)()
            torch.cuda.synchronize()
            same[name] = "==" if torch.equal(out[0], ref) else "max|d| %.3g" % float((out[0] - ref).abs().max())
        line = (f"M={M} N={N} K={K}: " + "  ".join(f"{n} {med[n]:.3f} us (min {min(times[n]):.3f})" for n, _ in runs) +
                f"  Q4_K/Q4_0 {med['Q4_K'] / med['Q4_0']:.3f}  Q5_1/Q4_0 {med['Q5_1'] / med['Q4_0']:.3f}"
                f"  cfg {qg.debug_config(M, N, K, qg.Q4_K)}" + (f"  variants vs in-tree: {same}" if same else ""))
        print(line, flush=True)
        lines.append(line)
        del copies, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
