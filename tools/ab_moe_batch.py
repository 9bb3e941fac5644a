#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_batch against the two entries the library had for these shapes, in one process, timed as bench.py
does (measurement tool, not product): G steps per hipGraph, HIP events on the launch stream, interleaved rounds, median
with the spread.
  python tools/ab_moe_batch.py [--rounds 7] [--G 4] [--layers 0,1] [--tokens 4,8,16,32,64,128,256] [--out FILE]
Arms, us per call (one call = the T * n_used expert products of one projection):
  (a) batch    qg_gemm_w4a8_moe_batch, the plan kernel included;
  (b) decode   qg_gemm_w4a8_moe on the same operands;
  (c) prefill  qg_gemm_w4a8_moe_prefill on the same operands, its plan kernel included.
Every step's ids come from a seeded router: n_used distinct experts per token drawn uniformly, or ("skew") every slot
on expert 0 with probability 1/2 and uniform otherwise. Each step works on another copy of the layer's expert tensor;
the copies rotate over a resident pool of more than 600 MB, so no step finds its weights in a cache. The down
projection (K > N) takes one activation row per slot, gate / up one per token. Every step of every arm is followed
by a one-element kernel node, as in tools/ab_moe.py. Before anything is timed (a) is compared with (b) bit for bit.
The last column says whether (a) is below min((b), (c)) by more than the run's own spread: `yes` where the batch arm's
maximum is below the minimum of the better of the two, `no` otherwise."""
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
from tools.ab_moe import LAYERS, one_expert  # noqa: E402
from tools.ab_moe_prefill import router  # noqa: E402

TYPES = (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=4, help="steps per graph")
    ap.add_argument("--layers", default=None, help="comma-separated indices into tools/ab_moe.py LAYERS")
    ap.add_argument("--types", default="Q4_K,Q6_K")
    ap.add_argument("--tokens", default="4,8,16,32,64,128,256")
    ap.add_argument("--skew-tokens", default="64", help="T of the skewed cases")
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

    emit(f"# {qg.version()}; us per call (T * n_used expert products), median of {a.rounds} interleaved rounds "
         f"(min..max), G={a.G} steps per graph, each on another copy of the expert tensor in a pool > 600 MB, a "
         "one-element kernel node after every step; per = slots / n_expert")
    sep = torch.zeros(1, device=dev)
    layers = LAYERS if a.layers is None else [LAYERS[int(i)] for i in a.layers.split(",")]
    cases = [(int(x), False) for x in a.tokens.split(",") if x] + [(int(x), True) for x in a.skew_tokens.split(",") if x]
    cpu_gen = torch.Generator()
    for lname, N, K, n_expert, n_used in layers:
        a_rows = n_used if K > N else 1
        for tname, t in TYPES:
            if tname not in a.types.split(","):
                continue
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + K + t)
            w = one_expert(t, N, K, gen, dev)
            copies = max(a.G, math.ceil(600e6 / (w.numel() * n_expert)))
            pool = torch.empty((copies, n_expert) + tuple(w.shape), dtype=torch.uint8, device=dev)
            pool.copy_(w.expand_as(pool))
            for T, skew in cases:
                slots = T * n_used
                cpu_gen.manual_seed(1000 * T + n_expert + skew)
                aq = qg.quantize_q8_1(torch.rand((T, a_rows, K), generator=gen, device=dev) * 2 - 1)
                ids_d = [router(T, n_used, n_expert, skew, cpu_gen).to(dev) for _ in range(a.G)]
                out = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                ws = torch.empty(qg.moe_batch_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def arm(fn, **kw):
                    def run():
                        for j in range(a.G):
                            fn(aq, pool[copy_of(j)], ids_d[j], T, n_used, N, K, t, a_rows=a_rows, out=out[j], **kw)
                            sep.add_(1.0)
                    return run

                arms = [("batch", arm(qg.gemm_w4a8_moe_batch, workspace=ws)), ("decode", arm(qg.gemm_w4a8_moe)),
                        ("prefill", arm(qg.gemm_w4a8_moe_prefill, workspace=ws))]
                # (a) against (b), bit for bit, before anything is timed
                arms[0][1]()
                got = out.clone()
                arms[1][1]()
                torch.cuda.synchronize()
                same = bool(torch.equal(got.view(torch.int32), out.view(torch.int32)))
                reps = 10 if slots <= 512 else 4
                times = {name: [] for name, _ in arms}
                for _ in range(a.rounds):
                    for name, fn in arms:
                        times[name].append(graph_time_us(fn, reps, a.G))
                        first[0] = (first[0] + a.G) % copies
                med = {n: statistics.median(v) for n, v in times.items()}
                best = min(("decode", "prefill"), key=lambda n: med[n])
                emit(f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T}{' skew' if skew else ''} slots={slots} "
                     f"per={slots / n_expert:g}: " +
                     "  ".join(f"{n} {med[n]:.1f} ({min(v):.1f}..{max(v):.1f})" for n, v in times.items()) +
                     f"  batch/min(decode,prefill) {med['batch'] / med[best]:.3f} ({best})"
                     f"  below beyond spread: {'yes' if max(times['batch']) < min(times[best]) else 'no'}"
                     f"  bits==decode {same}  [{qg.moe_batch_config(T, n_used, n_expert, N, K, t)}]")
                del out, ws
            del pool


if __name__ == "__main__":
    main()
