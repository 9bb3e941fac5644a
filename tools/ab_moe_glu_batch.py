#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_glu_batch against what a caller had at batched-decode sizes, in one process (measurement tool, not
product): G steps per timing, HIP events on the launch stream, interleaved rounds, median with the spread, captured (one
hipGraph of the G steps, as bench.py times) and eager (the same G steps launched from Python between two events).
  python tools/ab_moe_glu_batch.py [--rounds 7] [--G 4] [--classes 0,1,2,3,4,5] [--out FILE]
Arms, us per call (one call = act(gate(x) + bg) * (up(x) + bu) for the T * n_used slots):
  fused     qg_gemm_w4a8_moe_glu_batch: the plan kernel and the fused decode-GEMV kernel;
  sequence  qg_gemm_w4a8_moe_batch_bias on the gate experts, then on the up experts, then torch's op on the two results
            (silu(g) * u, or gpt-oss's clamped SwiGLU in five elementwise kernels): the same operands, ids, workspace;
  decode    qg_gemm_w4a8_moe_glu_bias, the per-slot decode entry, one launch.
Classes: Qwen3-MoE gate/up (768 x 2048, 8 of 128) Q4_K and Q6_K without bias, SwiGLU, T = 8 .. 256; Mixtral gate/up
(14336 x 4096, 2 of 8) Q4_K, T = 8 .. 64; gpt-oss (2880 x 2880, 4 of 32 and 4 of 128) MXFP4 with both biases and the
clamped SwiGLU, T = 8 .. 64. The ids of a step come from the uniform router of tools/ab_moe_prefill.py; each step works
on another copy of the gate and up tensors, which rotate over resident pools of more than 600 MB each, and is followed
by a one-element kernel node. Before anything is timed the arms are compared: fused and decode bit for bit, fused and
sequence relative to the largest output."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from bench import graph_time_us  # noqa: E402
from tools.ab_moe import one_expert  # noqa: E402
from tools.ab_moe_glu_prefill import eager_time_us  # noqa: E402
from tools.ab_moe_prefill import router  # noqa: E402
from tools.ab_mxfp4_ffn import ALPHA, LIMIT, mxfp4_expert, pool_of  # noqa: E402

SMALL_T, ALL_T = (8, 16, 32, 64), (8, 16, 32, 64, 256)
# (name, N, K, n_expert, n_used, type name, type, biased with the OAI op, T)
CLASSES = [("qwen3-moe gate/up", 768, 2048, 128, 8, "Q4_K", qg.Q4_K, False, ALL_T),
           ("qwen3-moe gate/up", 768, 2048, 128, 8, "Q6_K", qg.Q6_K, False, ALL_T),
           ("mixtral gate/up", 14336, 4096, 8, 2, "Q4_K", qg.Q4_K, False, SMALL_T),
           ("mixtral gate/up", 14336, 4096, 8, 2, "Q6_K", qg.Q6_K, False, SMALL_T),
           ("gpt-oss-20b", 2880, 2880, 32, 4, "MXFP4", qg.MXFP4, True, SMALL_T),
           ("gpt-oss-120b", 2880, 2880, 128, 4, "MXFP4", qg.MXFP4, True, SMALL_T)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=4, help="steps per timing")
    ap.add_argument("--classes", default="0,1,2,3,4,5", help="comma-separated indices into CLASSES")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G, lines = a.G, []

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every line: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# {qg.version()}; us per call (the GLU of the T * n_used gate and up products), median of {a.rounds} interleaved "
         f"rounds (min..max), G={G} steps per timing, each on another copy of the gate and up tensors in pools > 600 MB, a "
         "one-element kernel node after every step; uniform router. NOT AHEAD: the slowest fused round is not under the "
         "fastest round of that arm")
    sep = torch.zeros(1, device=dev)
    cpu_gen = torch.Generator()
    for lname, N, K, n_expert, n_used, tname, t, oai, tokens in [CLASSES[int(i)] for i in a.classes.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(N + K + t)
        (gates, copies), (ups, _) = (pool_of(mxfp4_expert(N, K, gen, dev) if t == qg.MXFP4 else one_expert(t, N, K, gen, dev),
                                             n_expert, G, 600.0, dev) for _ in range(2))
        op = qg.GLU_SWIGLU_OAI if oai else qg.GLU_SWIGLU
        bg, bu = ((torch.rand((n_expert, N), generator=gen, device=dev) * 2 - 1 for _ in range(2)) if oai else (None, None))
        for T in tokens:
            cpu_gen.manual_seed(1000 * T + n_expert)
            aq = qg.quantize_q8_1(torch.rand((T, K), generator=gen, device=dev) * 2 - 1)
            ids = [router(T, n_used, n_expert, False, cpu_gen).to(dev) for _ in range(G)]
            out, dec, g, u, ref = (torch.zeros((G, T, n_used, N), dtype=torch.float32, device=dev) for _ in range(5))
            tmp = torch.zeros((T, n_used, N), dtype=torch.float32, device=dev)
            ws = torch.empty(qg.moe_batch_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
            first = [0]
            cp = lambda j: (first[0] + j) % copies  # the copies rotate from timing to timing as well
            dims = (T, n_used, N, K, t)

            def fused():
                for j in range(G):
                    qg.gemm_w4a8_moe_glu_batch(aq, gates[cp(j)], ups[cp(j)], ids[j], *dims, op, bg, bu, ALPHA, LIMIT, workspace=ws,
                                               out=out[j])
                    sep.add_(1.0)

            def sequence():
                for j in range(G):
                    qg.gemm_w4a8_moe_batch_bias(aq, gates[cp(j)], bg, ids[j], *dims, workspace=ws, out=g[j])
                    qg.gemm_w4a8_moe_batch_bias(aq, ups[cp(j)], bu, ids[j], *dims, workspace=ws, out=u[j])
                    if oai:
                        x = g[j].clamp_(max=LIMIT)
                        y = u[j].clamp_(-LIMIT, LIMIT).add_(1.0)
                        torch.mul(x, ALPHA, out=tmp)
                        tmp.sigmoid_().mul_(x)
                        torch.mul(tmp, y, out=ref[j])
                    else:
                        torch.mul(torch.nn.functional.silu(g[j]), u[j], out=ref[j])
                    sep.add_(1.0)

            def decode():
                for j in range(G):
                    qg.gemm_w4a8_moe_glu_bias(aq, gates[cp(j)], ups[cp(j)], bg, bu, ids[j], *dims, op, ALPHA, LIMIT, out=dec[j])
                    sep.add_(1.0)

            fused(), sequence(), decode()
            torch.cuda.synchronize()
            bits = "equal" if torch.equal(out.view(torch.int32), dec.view(torch.int32)) else "DIFFER"
            worst = float((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            arms = (("fused", fused), ("sequence", sequence), ("decode", decode))
            times = {(m, n): [] for m in ("captured", "eager") for n, _ in arms}
            for _ in range(a.rounds):
                for mode, timer in (("captured", graph_time_us), ("eager", eager_time_us)):
                    for name, fn in arms:
                        times[(mode, name)].append(timer(fn, 10, G))
                        first[0] = (first[0] + G) % copies
            cell = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f}..{max(v):.1f})"
            row = f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T}:"
            for mode in ("captured", "eager"):
                f = times[(mode, "fused")]
                row += f"  {mode}: fused {cell(f)}"
                for other in ("sequence", "decode"):
                    s = times[(mode, other)]
                    row += (f"  {other} {cell(s)}  fused/{other} {statistics.median(f) / statistics.median(s):.3f}"
                            f"{'' if max(f) < min(s) else ' NOT AHEAD'}")
            emit(row + f"  fused-decode bits {bits}  |fused-seq|/max {worst:.1e}  [{qg.moe_glu_batch_config(T, n_used, n_expert, N, K, t)}]")
            del out, dec, g, u, ref, tmp, ws
        del gates, ups


if __name__ == "__main__":
    main()
