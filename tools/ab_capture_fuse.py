#!/usr/bin/env python3
"""A/B of the capture-time GEMV merge (qg_set_capture_fusion), tools/ab_lib.py's protocol in ONE process:
per shape, G qg_gemm_w4a8 calls on distinct resident weight copies (> 600 MB, so every launch streams from
HBM) are captured twice into a hipGraph — merge off (G kernel nodes) and merge on for every shape class
(mode 2: ceil(G / 64) grouped nodes) — and replayed in interleaved rounds, HIP events on the launch stream.
Outputs must agree bit for bit between the arms. The gate in csrc/qg_capture_fuse.hip (fuse_class_enabled) enables
the classes where "fused" beats "unfused" by more than the unfused arm's own spread.

  python tools/ab_capture_fuse.py [--shapes 1x4096x4096:2,...] [--rounds 7] [--reps 20] [--out table.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402

# bench.py --full side shapes whose form is "single" with M <= 4, the headline shape, and Q8_0 (MxNxK:wtype)
DEFAULT = ("1x4096x4096:2,2x4096x4096:2,4x4096x4096:2,1x4096x4096:3,1x4096x4096:6,1x4096x4096:7,1x4096x4096:8,"
           "1x32000x4096:2,1x4096x14336:2,2x4096x14336:2,3x4096x14336:2,4x4096x14336:2,2x8192x14336:2")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; G={a.G} GEMVs per step, {a.rounds} interleaved rounds x {a.reps} replays; us per GEMV, "
             "median (min .. max); gain = unfused / fused; spread = (max - min) / median of the unfused arm"]
    print(lines[0], flush=True)
    for spec in a.shapes.split(","):
        dims, wt = spec.split(":")
        M, N, K = (int(x) for x in dims.split("x"))
        wt = int(wt)
        gen = torch.Generator(device=dev)
        gen.manual_seed(M * 7 + N)
        aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
        wq = qg.quantize(torch.rand((N, K), generator=gen, device=dev) * 2 - 1, wt)
        R = max(a.G, math.ceil(600e6 / wq.numel()))
        copies = torch.empty((R,) + tuple(wq.shape), dtype=torch.uint8, device=dev)
        copies.copy_(wq.unsqueeze(0).expand_as(copies))
        outs = torch.zeros((2, a.G, M, N), dtype=torch.float32, device=dev)
        graphs, merged = [], []
        for arm, mode in enumerate((0, 2)):
            qg.set_capture_fusion(mode)

            def step(arm=arm):
                for j in range(a.G):
                    qg.gemm_w4a8(aq, copies[j % R], M, N, K, wt, out=outs[arm, j])
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                step()
            torch.cuda.synchronize()
            m0 = qg.capture_fusion_stats()[0]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            merged.append(qg.capture_fusion_stats()[0] - m0)
            graphs.append(g)
        qg.set_capture_fusion(1)
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        same = torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        times = [[], []]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.rounds):
            for arm, g in enumerate(graphs):
                g.replay()
                e0.record()
                for _ in range(a.reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[arm].append(e0.elapsed_time(e1) * 1e3 / (a.reps * a.G))
        med = [statistics.median(t) for t in times]
        spread = (max(times[0]) - min(times[0])) / med[0]
        line = (f"M={M} N={N} K={K} wtype={wt}: unfused {med[0]:7.3f} ({min(times[0]):.3f} .. {max(times[0]):.3f})  "
                f"fused {med[1]:7.3f} ({min(times[1]):.3f} .. {max(times[1]):.3f})  gain {med[0] / med[1]:.3f}x  "
                f"unfused spread {100 * spread:.1f}%  merged {merged[1]}/{a.G}  bits {'equal' if same else 'DIFFER'}")
        print(line, flush=True)
        lines.append(line)
        assert same and merged[0] == 0, (spec, same, merged)
        del copies, outs, graphs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
