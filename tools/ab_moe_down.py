#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_down against the sequence it replaces, on the same operands, in one process (measurement tool, not
product): interleaved rounds, median, HIP events on the launch stream. The protocol of tools/ab_moe_glu.py.
  python tools/ab_moe_down.py [--rounds 7] [--G 8] [--out profiles/moe_down/ab_moe_down.txt]
Arms, us per token (one token = its n_used down products, their multiplication by the router weights and their sum):
  seq, seq'  the sequence a caller runs without the entry: qg_gemm_w4a8_moe at a_rows = n_used, then torch's
             (d * w[..., None]).sum(1) (torch.mul into a buffer, torch.sum into the output: two kernels). The same arm
             twice: the difference of the two medians is the run-to-run spread every comparison is held against;
  fused      one qg_gemm_w4a8_moe_down launch;
  prod       the product launch of seq alone, neither multiply nor sum: what the fused launch has to beat to gain on
             the product itself and not only on the elementwise kernels.
Each class is measured twice: "graph", G steps captured into one hipGraph and replayed (bench.py's graph_time_us), and
"eager", the same G steps enqueued from Python between two events (the host's launch path is part of the figure).
Every step's ids pick, per token, n_used distinct experts (a uniform router) of one copy of the layer's down tensor;
the copies rotate over a resident pool of more than 600 MB, so no step finds its weights in a cache. Every step of every
arm is followed by a one-element kernel node, as in tools/ab_moe.py.
Before anything is timed the fused result is compared bit for bit with the fold acc = acc + w[:, u] * d[:, u] in
ascending u done with torch's elementwise kernels on the sequence's d, and its largest relative difference to torch's
sum (whose order is torch's own) is printed."""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from ab_moe import one_expert  # noqa: E402
from ab_moe_glu import eager_time_us  # noqa: E402
from bench import graph_time_us  # noqa: E402

# (name, N, K, n_expert, n_used): the down shapes
LAYERS = [("mixtral", 4096, 14336, 8, 2), ("qwen3-moe", 2048, 768, 128, 8)]
TYPES = (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K))
TOKENS = (1, 8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=8, help="steps per graph / per eager call")
    ap.add_argument("--layers", default=None, help="comma-separated indices into LAYERS")
    ap.add_argument("--pool-mb", type=float, default=600.0, help="resident bytes of the weight tensor the copies rotate over")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; us per token (n_used down products + weights + sum), median of {a.rounds} interleaved rounds "
             f"(min..max), G={a.G} steps per graph / eager call, each on another copy of the down tensor in a pool "
             f"> {a.pool_mb:.0f} MB; a one-element kernel node after every step. spread = |seq - seq'|; ahead: fused "
             "below the lower seq median by more than the spread"]
    sep = torch.zeros(1, device=dev)
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    layers = LAYERS if a.layers is None else [LAYERS[int(i)] for i in a.layers.split(",")]
    for lname, N, K, n_expert, n_used in layers:
        for tname, t in TYPES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + K + t)
            w1 = one_expert(t, N, K, gen, dev)
            copies = max(a.G, math.ceil(a.pool_mb * 1e6 / (w1.numel() * n_expert)))
            pool = torch.empty((copies, n_expert) + tuple(w1.shape), dtype=torch.uint8, device=dev)
            pool.copy_(w1.expand_as(pool))
            for T in TOKENS:
                aq = qg.quantize_q8_1((torch.rand((T * n_used, K), generator=gen, device=dev) * 2 - 1) * 0.02)
                aq = aq.reshape(T, n_used, K // 32, 36)
                ids_d = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32).to(dev)
                         for _ in range(a.G)]
                rw = torch.softmax(torch.rand((a.G, T, n_used), generator=gen, device=dev) * 4, dim=-1).contiguous()
                out = torch.zeros((a.G, T, N), dtype=torch.float32, device=dev)
                d = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                tmp = torch.zeros((T, n_used, N), dtype=torch.float32, device=dev)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def product(j):
                    qg.gemm_w4a8_moe(aq, pool[copy_of(j)], ids_d[j], T, n_used, N, K, t, a_rows=n_used, out=d[j])

                def seq():
                    for j in range(a.G):
                        product(j)
                        torch.mul(d[j], rw[j].unsqueeze(-1), out=tmp)
                        torch.sum(tmp, 1, out=out[j])
                        sep.add_(1.0)

                def prod():
                    for j in range(a.G):
                        product(j)
                        sep.add_(1.0)

                def fused():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe_down(aq, pool[copy_of(j)], ids_d[j], rw[j], T, n_used, N, K, t, out=out[j])
                        sep.add_(1.0)

                # the results agree before anything is timed
                seq()
                ref = out.clone()
                fold = torch.zeros_like(out)
                for u in range(n_used):
                    fold = fold + rw[:, :, u].unsqueeze(-1) * d[:, :, u]
                out.zero_()
                fused()
                torch.cuda.synchronize()
                same = torch.equal(out.view(torch.int32), fold.view(torch.int32))
                rel = ((out - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
                del ref, fold

                arms = [("seq", seq), ("seq'", seq), ("fused", fused), ("prod", prod)]
                for mode, timer in (("graph", graph_time_us), ("eager", eager_time_us)):
                    times = {name: [] for name, _ in arms}
                    for _ in range(a.rounds):
                        for name, fn in arms:
                            times[name].append(timer(fn, 10, a.G * T))
                            first[0] = (first[0] + a.G) % copies
                    med = {n: statistics.median(v) for n, v in times.items()}
                    spread = abs(med["seq"] - med["seq'"])
                    low = min(med["seq"], med["seq'"])
                    ahead = med["fused"] < low - spread
                    emit(f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T} {mode}: " + "  ".join(
                        f"{n} {med[n]:.3f} ({min(v):.3f}..{max(v):.3f})" for n, v in times.items()) +
                        f"  spread {spread:.3f}  fused/seq {med['fused'] / low:.3f}  fused/prod {med['fused'] / med['prod']:.3f}"
                        f"  {'ahead' if ahead else 'NOT AHEAD'}  fold bits {'==' if same else 'DIFFER'}  max rel diff to "
                        f"torch's sum {rel:.2e}  [{qg.moe_down_config(T, n_used, N, K, t)}]")
                del out, d, tmp
            del pool
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
