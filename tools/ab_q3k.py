#!/usr/bin/env python3
"""Q3_K against Q4_K and Q6_K through qg_gemm_w4a8 in one process, timed as bench.py does: G launches over rotating
resident weight copies (> 600 MB) in a hipGraph, HIP events on the launch stream, interleaved rounds (measurement tool,
not product). Bytes per weight element: Q3_K 0.4297, Q4_K 0.5625, Q6_K 0.8203. Every figure is the median of the
rounds with their spread (min .. max).
  python tools/ab_q3k.py [--shapes 1x4096x4096,...] [--rounds 7] [--out profiles/q3k/ab_q3k.txt]
  python tools/ab_q3k.py --threshold 8 [--out profiles/q3k/ab_q3k_threshold.txt]
  python tools/ab_q3k.py --moe [--out profiles/q3k/ab_q3k_moe.txt]
Shapes are MxNxK: M tokens, N weight rows. None of the three types is merged in capture: kernel node against kernel node.
--threshold: the forced decode GEMV (QG_ALGO_GEMV) against the forced MFMA prefill (QG_ALGO_MFMA) of Q3_K at
N = K = 4096, interleaved the same way.
--moe: qg_gemm_w4a8_moe with Q3_K experts at Mixtral's (N = 14336, K = 4096, 2 of 8) and Qwen3-MoE's (N = 768,
K = 2048, 8 of 128) gate / up shape, T = 1 and 8, a uniform router, per slot, against one kernel node per slot with the
ids on the host (all a caller could do otherwise)."""
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

DEFAULT = "1x4096x4096,8x4096x4096,32x4096x4096,512x4096x4096,1x4096x14336"
TYPES = (("Q3_K", qg.Q3_K), ("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K))
MOE_SHAPES = (("mixtral", 8, 2, 14336, 4096), ("qwen3-moe", 128, 8, 768, 2048))  # name, experts, used, N, K


def random_weights(t: int, n: int, k: int, gen: torch.Generator, dev: torch.device) -> torch.Tensor:
    """[n, k/bs, block bytes] with uniform code bytes and small finite scales (the timing does not depend on the values;
    the products are checked by the GPU tests)."""
    nsb = k // qg.block_elems(t)
    w = torch.randint(0, 256, (n, nsb, qg.BLOCK_BYTES[t]), generator=gen, device=dev, dtype=torch.uint8)
    d = ((torch.rand((n, nsb, 2), generator=gen, device=dev) * 2 - 1) * 0.01).to(torch.float16).view(torch.uint8)
    if t == qg.Q4_K:  # d and dmin lead the block; Q3_K and Q6_K end in d
        w[..., 0:4] = d.reshape(n, nsb, 4)
    else:
        w[..., -2:] = d.reshape(n, nsb, 4)[..., :2]
    return w


def rotating(w: torch.Tensor, G: int, least: int) -> torch.Tensor:
    R = max(least, math.ceil(600e6 / w.numel()))
    c = torch.empty((R,) + tuple(w.shape), dtype=torch.uint8, device=w.device)
    c.copy_(w.unsqueeze(0).expand_as(c))
    return c


def stat(v) -> str:
    return f"{statistics.median(v):.3f} us ({min(v):.3f} .. {max(v):.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--threshold", default=None, help="comma-separated M: forced GEMV against forced MFMA, N = K = 4096")
    ap.add_argument("--moe", action="store_true", help="the expert entry at Mixtral's and Qwen3-MoE's shapes")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per launch, median of {a.rounds} interleaved rounds (min .. max), G={a.G} launches "
             "per graph over rotating weight copies > 600 MB"]
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    gen = torch.Generator(device=dev)
    if a.threshold:
        N = K = 4096
        gen.manual_seed(N + K)
        cp = rotating(random_weights(qg.Q3_K, N, K, gen, dev), a.G, a.G)
        for M in (int(x) for x in a.threshold.split(",")):
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)
            algos = [("gemv", qg.ALGO_GEMV)] * (M <= 8) + [("mfma", qg.ALGO_MFMA)]
            times = {n: [] for n, _ in algos}
            for _ in range(a.rounds):
                for name, algo in algos:
                    run = lambda: [qg.gemm_w4a8(aq, cp[j], M, N, K, qg.Q3_K, algo, out=out[j]) for j in range(a.G)]
                    times[name].append(graph_time_us(run, 10, a.G))
            emit(f"M={M} N={N} K={K}: " + "  ".join(
                f"{n} {stat(v)} [{qg.debug_config(M, N, K, qg.Q3_K, algo=al)}]"
                for (n, al), v in zip(algos, times.values())) + f"  auto: {qg.debug_config(M, N, K, qg.Q3_K).split()[0]}")
            del out
    elif a.moe:
        for name, n_expert, n_used, N, K in MOE_SHAPES:
            gen.manual_seed(n_expert)
            w = random_weights(qg.Q3_K, n_expert * N, K, gen, dev).reshape(n_expert, N, K // 256, 110)
            cp = rotating(w, a.G, 2)  # rotating copies of the whole expert set
            R = cp.shape[0]
            for T in (1, 8):
                slots = T * n_used
                aq = qg.quantize_q8_1(torch.rand((T, 1, K), generator=gen, device=dev) * 2 - 1)
                ids = torch.randint(0, n_expert, (a.G, T, n_used), generator=gen, device=dev, dtype=torch.int32)
                ids_h = ids.cpu().tolist()
                out = torch.empty((T, n_used, N), dtype=torch.float32, device=dev)

                def one():  # a launch per step, ids on the device
                    for j in range(a.G):
                        qg.gemm_w4a8_moe(aq, cp[j % R], ids[j], T, n_used, N, K, qg.Q3_K, out=out)

                def per_slot():  # a kernel node per slot, ids on the host
                    for j in range(a.G):
                        for t in range(T):
                            for u in range(n_used):
                                qg.gemm_w4a8(aq[t], cp[j % R][ids_h[j][t][u]], 1, N, K, qg.Q3_K, out=out[t, u:u + 1])

                times = {"moe": [], "nodes": []}
                for _ in range(a.rounds):
                    times["moe"].append(graph_time_us(one, 10, a.G * slots))
                    times["nodes"].append(graph_time_us(per_slot, 10, a.G * slots))
                ratio = statistics.median(times["moe"]) / statistics.median(times["nodes"])
                emit(f"{name} experts={n_expert} used={n_used} T={T} N={N} K={K}: per slot  moe {stat(times['moe'])}  "
                     f"one node per slot {stat(times['nodes'])}  moe/nodes {ratio:.3f}  "
                     f"cfg {qg.moe_config(T, n_used, N, K, qg.Q3_K)}")
                del out
            del cp, w
    else:
        for spec in a.shapes.split(","):
            M, N, K = (int(x) for x in spec.split("x"))
            gen.manual_seed(M + N + K)
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            copies = {name: rotating(random_weights(t, N, K, gen, dev), a.G, a.G) for name, t in TYPES}
            out = torch.empty((a.G, M, N), dtype=torch.float32, device=dev)

            def step_of(name, t):
                cp = copies[name]

                def run():
                    for j in range(a.G):
                        qg.gemm_w4a8(aq, cp[j], M, N, K, t, out=out[j])
                return run

            times = {name: [] for name, _ in TYPES}
            for _ in range(a.rounds):
                for name, t in TYPES:
                    times[name].append(graph_time_us(step_of(name, t), 10, a.G))
            med = {n: statistics.median(v) for n, v in times.items()}
            gbs = N * K * (110 / 256) / med["Q3_K"] / 1e3  # weight bytes only
            emit(f"M={M} N={N} K={K}: " + "  ".join(f"{n} {stat(times[n])}" for n, _ in TYPES) +
                 "".join(f"  Q3_K/{n} {med['Q3_K'] / med[n]:.3f}" for n, _ in TYPES[1:]) +
                 f"  Q3_K weights {gbs:.0f} GB/s  cfg {qg.debug_config(M, N, K, qg.Q3_K)}")
            del copies, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
