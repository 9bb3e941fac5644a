#!/usr/bin/env python3
"""qg_gemm_w4a8_moe against what a caller with host-known ids can do today, in one process, timed as bench.py does
(measurement tool, not product): G steps per hipGraph, HIP events on the launch stream, interleaved rounds, median.
  python tools/ab_moe.py [--rounds 7] [--G 8] [--out profiles/moe/ab_moe.txt]
Arms, us per slot (one slot = one (token, expert) product of M = 1):
  (a) moe     one qg_gemm_w4a8_moe launch per step, the ids read on the device;
  (b) nodes   the same products as single qg_gemm_w4a8 M = 1 calls with the capture-time merge off: one kernel node
              per slot, what every type can do today with ids copied to the host before capture;
  (c) merged  the same with the merge on (Q4_0 .. Q8_0 only: the grouped node of up to 64 GEMVs).
Every step's ids pick, per token, n_used distinct experts of one copy of the layer's expert tensor; the copies rotate
over a resident pool of more than 600 MB, so no step finds its weights in a cache. The down projection (K > N)
takes one activation row per slot (a_rows = n_used), gate / up one per token.
A decode step's expert products are followed by other kernels (the activation, the next router), so by default every
step of every arm is followed by a one-element kernel node: without it (--no-separator) the capture-time merge joins
the GEMVs of up to 64 slots ACROSS steps in arm (c), one launch boundary per 64 slots whatever T is, which no model
graph offers. The separator's time is part of every arm's figure alike."""
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

# (name, N, K, n_expert, n_used)
LAYERS = [("mixtral gate/up", 14336, 4096, 8, 2), ("mixtral down", 4096, 14336, 8, 2),
          ("qwen3-moe gate/up", 768, 2048, 128, 8), ("qwen3-moe down", 2048, 768, 128, 8)]
TYPES = (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K), ("Q4_0", qg.Q4_0), ("Q8_0", qg.Q8_0))
TOKENS = (1, 4, 8)


def one_expert(t: int, n: int, k: int, gen: torch.Generator, dev: torch.device) -> torch.Tensor:
    """[n, k/bs, block bytes]: quantized uniform values for the row types, uniform bytes with small finite f16 scales
    for the K-quants (the timing does not depend on the values; the products are checked by tests/test_gpu_moe.py)."""
    if t in (qg.Q4_0, qg.Q8_0):
        return qg.quantize(torch.rand((n, k), generator=gen, device=dev) * 2 - 1, t)
    w = torch.randint(0, 256, (n, k // 256, qg.BLOCK_BYTES[t]), generator=gen, device=dev, dtype=torch.uint8)
    d = ((torch.rand((n, k // 256, 2), generator=gen, device=dev) * 2 - 1) * 0.01).to(torch.float16).view(torch.uint8)
    if t == qg.Q4_K:
        w[..., 0:4] = d.reshape(n, k // 256, 4)
    else:
        w[..., 208:210] = d.reshape(n, k // 256, 4)[..., 0:2]
    return w


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=8, help="steps per graph")
    ap.add_argument("--no-separator", action="store_true", help="no kernel node between the steps of a graph")
    ap.add_argument("--layers", default=None, help="comma-separated indices into LAYERS")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per slot (M = 1 product), median of {a.rounds} interleaved rounds (min..max), "
             f"G={a.G} steps per graph, each on another copy of the expert tensor in a pool > 600 MB; " +
             ("no separator between steps" if a.no_separator else "a one-element kernel node after every step")]
    sep = torch.zeros(1, device=dev)

    def end_step() -> None:
        if not a.no_separator:
            sep.add_(1.0)
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    layers = LAYERS if a.layers is None else [LAYERS[int(i)] for i in a.layers.split(",")]
    for lname, N, K, n_expert, n_used in layers:
        a_rows_of = n_used if K > N else 1
        for tname, t in TYPES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + K + t)
            w = one_expert(t, N, K, gen, dev)
            copies = max(a.G, math.ceil(600e6 / (w.numel() * n_expert)))
            pool = torch.empty((copies, n_expert) + tuple(w.shape), dtype=torch.uint8, device=dev)
            pool.copy_(w.expand_as(pool))
            for T in TOKENS:
                slots = T * n_used
                aq = qg.quantize_q8_1(torch.rand((T, a_rows_of, K), generator=gen, device=dev) * 2 - 1)
                ids_h = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32) for _ in range(a.G)]
                ids_d = [i.to(dev) for i in ids_h]
                out = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def moe():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe(aq, pool[copy_of(j)], ids_d[j], T, n_used, N, K, t, a_rows=a_rows_of, out=out[j])
                        end_step()

                def singles():
                    for j in range(a.G):
                        p = pool[copy_of(j)]
                        for tt in range(T):
                            for u in range(n_used):
                                qg.gemm_w4a8(aq[tt, u % a_rows_of:u % a_rows_of + 1], p[int(ids_h[j][tt, u])], 1, N, K, t,
                                             out=out[j, tt, u:u + 1])
                        end_step()

                def nodes():
                    qg.set_capture_fusion(0)
                    try:
                        singles()
                    finally:
                        qg.set_capture_fusion(1)

                arms = [("moe", moe), ("nodes", nodes)] + ([("merged", singles)] if t in (qg.Q4_0, qg.Q8_0) else [])
                # the arms agree bit for bit before anything is timed
                res = {}
                for name, fn in arms:
                    out.zero_()
                    fn()
                    torch.cuda.synchronize()
                    res[name] = out.clone()
                same = all(torch.equal(res["moe"].view(torch.int32), r.view(torch.int32)) for r in res.values())
                times = {name: [] for name, _ in arms}
                for _ in range(a.rounds):
                    for name, fn in arms:
                        times[name].append(graph_time_us(fn, 10, a.G * slots))
                        first[0] = (first[0] + a.G) % copies
                med = {n: statistics.median(v) for n, v in times.items()}
                emit(f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T} slots={slots}: " + "  ".join(
                    f"{n} {med[n]:.3f} ({min(v):.3f}..{max(v):.3f})" for n, v in times.items()) +
                    f"  moe/nodes {med['moe'] / med['nodes']:.3f}" +
                    (f"  moe/merged {med['moe'] / med['merged']:.3f}" if "merged" in med else "") +
                    f"  bits {'==' if same else 'DIFFER'}  [{qg.moe_config(T, n_used, N, K, t)}]")
                del out, res
            del pool
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
