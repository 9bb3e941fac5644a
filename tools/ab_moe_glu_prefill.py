#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_glu_prefill against the sequence it replaces, in one process (measurement tool, not product): G steps
per timing, HIP events on the launch stream, interleaved rounds, median with the spread, captured (one hipGraph of the G
steps, as bench.py times) and eager (the same G steps launched from Python between two events).
  python tools/ab_moe_glu_prefill.py [--rounds 7] [--G 4] [--layers 0,2] [--tokens 16,64,256,1024] [--out FILE]
Arms, us per call (one call = act(gate(x)) * up(x) for the T * n_used slots):
  fused     qg_gemm_w4a8_moe_glu_prefill: the plan kernel and the fused MFMA kernel;
  sequence  qg_gemm_w4a8_moe_prefill on the gate experts, then on the up experts, then torch's GLU on the two results
            (silu(g) * u, two elementwise kernels): the same operands, ids and workspace.
The ids of a step come from the uniform router of tools/ab_moe_prefill.py; each step works on another copy of the gate
and up tensors, which rotate over resident pools of more than 600 MB each, and is followed by a one-element kernel node.
Before anything is timed the two arms are compared (relative to the largest output; the bits are the tests' business)."""
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
from tools.ab_moe_prefill import TYPES, router  # noqa: E402


def eager_time_us(fn, reps: int, per: int) -> float:
    """fn() launched `reps` times from the host between two events, us per call."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * per)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=4, help="steps per timing")
    ap.add_argument("--layers", default="0,2", help="comma-separated indices into tools/ab_moe.py LAYERS (the gate/up ones)")
    ap.add_argument("--tokens", default="16,64,256,1024")
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

    emit(f"# {qg.version()}; us per call (SwiGLU of the T * n_used gate and up products), median of {a.rounds} interleaved "
         f"rounds (min..max), G={a.G} steps per timing, each on another copy of the gate and up tensors in pools > 600 MB, a "
         "one-element kernel node after every step; uniform router")
    sep = torch.zeros(1, device=dev)
    cpu_gen = torch.Generator()
    for lname, N, K, n_expert, n_used in [LAYERS[int(i)] for i in a.layers.split(",")]:
        for tname, t in TYPES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + K + t)
            pools = []
            for _ in range(2):
                w = one_expert(t, N, K, gen, dev)
                copies = max(a.G, math.ceil(600e6 / (w.numel() * n_expert)))
                pool = torch.empty((copies, n_expert) + tuple(w.shape), dtype=torch.uint8, device=dev)
                pool.copy_(w.expand_as(pool))
                pools.append(pool)
            gates, ups = pools
            for T in [int(x) for x in a.tokens.split(",") if x]:
                cpu_gen.manual_seed(1000 * T + n_expert)
                aq = qg.quantize_q8_1(torch.rand((T, K), generator=gen, device=dev) * 2 - 1)
                ids = [router(T, n_used, n_expert, False, cpu_gen).to(dev) for _ in range(a.G)]
                shape = (a.G, T, n_used, N)
                out, g, u = (torch.zeros(shape, dtype=torch.float32, device=dev) for _ in range(3))
                ref = torch.zeros(shape, dtype=torch.float32, device=dev)
                ws = torch.empty(qg.moe_prefill_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def fused():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe_glu_prefill(aq, gates[copy_of(j)], ups[copy_of(j)], ids[j], T, n_used, N, K, t,
                                                     qg.GLU_SWIGLU, workspace=ws, out=out[j])
                        sep.add_(1.0)

                def sequence():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe_prefill(aq, gates[copy_of(j)], ids[j], T, n_used, N, K, t, workspace=ws, out=g[j])
                        qg.gemm_w4a8_moe_prefill(aq, ups[copy_of(j)], ids[j], T, n_used, N, K, t, workspace=ws, out=u[j])
                        torch.mul(torch.nn.functional.silu(g[j]), u[j], out=ref[j])
                        sep.add_(1.0)

                fused()
                sequence()
                torch.cuda.synchronize()
                worst = float((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
                arms = (("fused", fused), ("sequence", sequence))
                reps = 10 if T * n_used <= 512 else 4
                times = {(m, n): [] for m in ("captured", "eager") for n, _ in arms}
                for _ in range(a.rounds):
                    for mode, timer in (("captured", graph_time_us), ("eager", eager_time_us)):
                        for name, fn in arms:
                            times[(mode, name)].append(timer(fn, reps, a.G))
                            first[0] = (first[0] + a.G) % copies
                cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f}..{max(v):.1f})"
                row = f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T}:"
                for mode in ("captured", "eager"):
                    f, s = times[(mode, "fused")], times[(mode, "sequence")]
                    ahead = max(f) < min(s)  # beyond the spread: the slowest fused round under the fastest of the sequence
                    row += (f"  {mode}: fused {cell(f)}  sequence {cell(s)}  fused/sequence "
                            f"{statistics.median(f) / statistics.median(s):.3f}{'' if ahead else ' NOT AHEAD'}")
                emit(row + f"  |fused-seq|/max {worst:.1e}  [{qg.moe_glu_prefill_config(T, n_used, n_expert, N, K, t)}] "
                     f"[{qg.moe_prefill_config(T, n_used, n_expert, N, K, t)}]")
                del out, g, u, ref, ws
            del pools, gates, ups, pool


if __name__ == "__main__":
    main()
