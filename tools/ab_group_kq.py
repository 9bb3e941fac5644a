#!/usr/bin/env python3
"""qg_gemm_w4a8_grouped_kq against what a caller had for a dense K-quant layer's decode projections, in one process
(measurement tool, not product): captured graphs, HIP events on the launch stream, interleaved rounds, median with the
spread.
  python tools/ab_group_kq.py [--rounds 7] [--classes 0,1,2] [--m 1,2,4,8] [--out FILE]
Arms, us per layer (one layer = the class's group of products at one M):
  grouped   one qg_gemm_w4a8_grouped_kq call per layer: one kernel node;
  single    the same items as consecutive qg_gemm_w4a8 calls, one kernel node each (a K-quant call never merges in capture).
Classes, the shapes of a Q4_K_M Llama-3-8B layer at K = 4096: QKV with N = 4096 Q4_K, 1024 Q4_K, 1024 Q6_K (the layers
whose V is Q6_K: the mix form); QKV with all three Q4_K (the other layers: the q4k form); gate / up, N = 14336 twice,
Q4_K. A graph holds `layers` layers (32 for QKV, 8 for gate / up), each on its own copy of the weights (more than 480 MB
per graph), every layer followed by a one-element kernel node. Before anything is timed the two arms are compared bit
for bit. early-exit: the share of the grouped launch's workgroups that lie past their item's rows and leave at once."""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from bench import graph_time_us  # noqa: E402
from tools.ab_moe import one_expert  # noqa: E402

K = 4096
# (name, [(N, type)], layers per graph)
CLASSES = [("qkv Q4_K/Q4_K/Q6_K", [(4096, qg.Q4_K), (1024, qg.Q4_K), (1024, qg.Q6_K)], 32),
           ("qkv Q4_K/Q4_K/Q4_K", [(4096, qg.Q4_K), (1024, qg.Q4_K), (1024, qg.Q4_K)], 32),
           ("gate/up Q4_K/Q4_K", [(14336, qg.Q4_K), (14336, qg.Q4_K)], 8)]


def early_exit_share(cfg: str, ns) -> float:
    """From the config line: 1 - (row tiles the items have) / (workgroups of the grid)."""
    f = dict(x.split("=") for x in cfg.split()[1:])
    rpb = int(f["WGS"]) // 64 * (64 // int(f["LPR"]))
    gx, gy = map(int, re.fullmatch(r"(\d+)x(\d+)", f["grid"]).groups())
    return 1.0 - sum((n + rpb - 1) // rpb for n in ns) / (gx * gy)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--classes", default="0,1,2", help="comma-separated indices into CLASSES")
    ap.add_argument("--m", default="1,2,4,8", help="comma-separated M")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every line: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# {qg.version()}; K={K}; us per layer, median of {a.rounds} interleaved rounds (min..max), captured graphs of "
         "`layers` layers, each on its own copy of the weights, a one-element kernel node after every layer. NOT AHEAD: "
         "the slowest grouped round is not under the fastest single round")
    sep = torch.zeros(1, device=dev)
    for name, shape, layers in [CLASSES[int(i)] for i in a.classes.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(len(shape) * 1000 + shape[-1][1])
        ns, ts = [n for n, _ in shape], [t for _, t in shape]
        ws = [[one_expert(t, n, K, gen, dev) for n, t in shape] for _ in range(layers)]
        mb = sum(w.numel() for w in ws[0]) * layers / 1e6
        for M in [int(m) for m in a.m.split(",")]:
            aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
            out_g, out_s = ([[torch.zeros((M, n), dtype=torch.float32, device=dev) for n in ns] for _ in range(layers)]
                            for _ in range(2))

            def grouped():
                for w, o in zip(ws, out_g):
                    qg.gemm_w4a8_grouped_kq([aq] * len(ns), w, ns, ts, M, K, outs=o)
                    sep.add_(1.0)

            def single():
                for w, o in zip(ws, out_s):
                    for wi, oi, n, t in zip(w, o, ns, ts):
                        qg.gemm_w4a8(aq, wi, M, n, K, t, out=oi)
                    sep.add_(1.0)

            grouped(), single()
            torch.cuda.synchronize()
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for g, s in zip(out_g, out_s) for x, y in zip(g, s))
            times = {"grouped": [], "single": []}
            for _ in range(a.rounds):
                for arm, fn in (("grouped", grouped), ("single", single)):
                    times[arm].append(graph_time_us(fn, 10, layers))
            cell = lambda v: f"{statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})"
            g, s = times["grouped"], times["single"]
            cfg = qg.group_kq_config([(aq.data_ptr(), w.data_ptr(), o.data_ptr(), n, 0, t)
                                      for w, o, n, t in zip(ws[0], out_g[0], ns, ts)], M, K)
            emit(f"{name} N={'/'.join(map(str, ns))} M={M} layers={layers} ({mb:.0f} MB): grouped {cell(g)}  single {cell(s)}  "
                 f"grouped/single {statistics.median(g) / statistics.median(s):.3f}{'' if max(g) < min(s) else ' NOT AHEAD'}  "
                 f"bits {'equal' if same else 'DIFFER'}  early-exit {100 * early_exit_share(cfg, ns):.0f}%  [{cfg}]")
            del out_g, out_s
        del ws


if __name__ == "__main__":
    main()
