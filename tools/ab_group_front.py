#!/usr/bin/env python3
"""A/B of the affine route of grouped GEMV launches (qg_set_group_affine), tools/ab_capture_fuse.py's protocol
in ONE process: per class, 64 products per step on distinct resident weight copies (> 600 MB, so every launch
streams from HBM), issued as qg_gemm_w4a8_grouped launches of `group` items each (consecutive copies, shared
activations, consecutive outputs: affine), captured twice into a hipGraph — mode 0 (gemvg_kernel) and mode 2
(the strided batch's kernel for every class) — and replayed in interleaved rounds, HIP events on the launch
stream. Outputs must agree bit for bit between the arms, and the route query must name the two families. The
gate in csrc/qg_gemv_kernel.hpp (group_affine_class_enabled) enables the classes where "affine" beats
"grouped" by more than the grouped arm's own spread.

  python tools/ab_group_front.py [--shapes 1x4096x4096:2:64,...] [--rounds 7] [--reps 20] [--out table.txt]
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

# MxNxK:wtype:group — the shape list of tools/ab_capture_fuse.py in groups of 64, then gate/up-like pairs
# (N = 14336, K = 4096) and Q/K/V-like triples (N = K = 4096)
DEFAULT = ("1x4096x4096:2:64,2x4096x4096:2:64,4x4096x4096:2:64,1x4096x4096:3:64,1x4096x4096:6:64,1x4096x4096:7:64,"
           "1x4096x4096:8:64,1x32000x4096:2:64,1x4096x14336:2:64,2x4096x14336:2:64,3x4096x14336:2:64,"
           "4x4096x14336:2:64,2x8192x14336:2:64,"
           "1x14336x4096:2:2,2x14336x4096:2:2,1x4096x4096:2:3,2x4096x4096:2:3,1x4096x4096:8:3")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--G", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=1, help="untimed rounds of both arms before the counted ones")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; {a.G} products per step in grouped launches of `group` items, {a.rounds} interleaved "
             f"rounds x {a.reps} replays after {a.warm} uncounted; us per GEMV, median (min .. max); gain = grouped / affine; spread = (max - min) "
             "/ median of the grouped arm"]
    print(lines[0], flush=True)
    for spec in a.shapes.split(","):
        dims, wt, grp = spec.split(":")
        M, N, K = (int(x) for x in dims.split("x"))
        wt, grp = int(wt), int(grp)
        nl = a.G // grp          # launches per step
        prods = nl * grp
        gen = torch.Generator(device=dev)
        gen.manual_seed(M * 7 + N)
        aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
        wq = qg.quantize(torch.rand((N, K), generator=gen, device=dev) * 2 - 1, wt)
        R = max(prods, math.ceil(600e6 / wq.numel()))
        copies = torch.empty((R,) + tuple(wq.shape), dtype=torch.uint8, device=dev)
        copies.copy_(wq.unsqueeze(0).expand_as(copies))
        outs = torch.zeros((2, prods, M, N), dtype=torch.float32, device=dev)
        graphs, routes = [], []
        for arm, mode in enumerate((0, 2)):
            qg.set_group_affine(mode)
            routes.append(qg.group_config([(aq.data_ptr(), copies[j].data_ptr(), outs[arm, j].data_ptr(), N, N)
                                           for j in range(grp)], M, K, wt))

            def step(arm=arm):
                for l in range(nl):
                    js = range(l * grp, (l + 1) * grp)
                    qg.gemm_w4a8_grouped([aq] * grp, [copies[j] for j in js], [N] * grp, M, K, wt,
                                         outs=[outs[arm, j] for j in js])
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                step()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            graphs.append(g)
        qg.set_group_affine(1)
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        same = torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        times = [[], []]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rnd in range(a.warm + a.rounds):
            for arm, g in enumerate(graphs):
                g.replay()
                e0.record()
                for _ in range(a.reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= a.warm:  # (the first round after the copies are made runs slow in whichever arm goes first)
                    times[arm].append(e0.elapsed_time(e1) * 1e3 / (a.reps * prods))
        med = [statistics.median(t) for t in times]
        spread = (max(times[0]) - min(times[0])) / med[0]
        line = (f"M={M} N={N} K={K} wtype={wt} group={grp}: grouped {med[0]:7.3f} ({min(times[0]):.3f} .. {max(times[0]):.3f})  "
                f"affine {med[1]:7.3f} ({min(times[1]):.3f} .. {max(times[1]):.3f})  gain {med[0] / med[1]:.3f}x  "
                f"grouped spread {100 * spread:.1f}%  bits {'equal' if same else 'DIFFER'}\n"
                f"    grouped: {routes[0]}\n    affine:  {routes[1]}")
        print(line, flush=True)
        lines.append(line)
        assert same and routes[0].startswith("gemvg") and routes[1].startswith("gemvb"), (spec, same, routes)
        del copies, outs, graphs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
