#!/usr/bin/env python3
"""qg_gemm_w4a8_f32_kq against what a caller had for a Q4_K / Q6_K decode projection on FP32 rows, in one process
(measurement tool, not product): HIP events on the launch stream, interleaved rounds, median with the spread.
  python tools/ab_kq_f32.py [--rounds 7] [--types 12,14] [--shapes 0,1,2] [--m 1,2,4,8] [--out FILE]
Arms, us per layer (one layer = one product at one M), both through the C ABI on buffers allocated once:
  fused   one qg_gemm_w4a8_f32_kq call: one kernel node;
  two     qg_quantize_q8_1 into a workspace, then qg_gemm_w4a8 on it: two kernel nodes.
Shapes N x K: 4096 x 4096, 4096 x 14336, 14336 x 4096. Modes: `captured`, a graph of `layers` layers replayed 10 times,
and `eager`, the same launches enqueued from Python 10 times (the host's cost per call is part of that figure). Each layer
has its own copy of the weights (more than 480 MB per pass) and is followed by a one-element kernel node. Before anything
is timed the two arms are compared bit for bit."""
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

SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # N x K
NAMES = {qg.Q4_K: "Q4_K", qg.Q6_K: "Q6_K"}


def eager_time_us(fn, reps: int, per: int) -> float:
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
    ap.add_argument("--types", default="12,14")
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices into SHAPES")
    ap.add_argument("--m", default="1,2,4,8", help="comma-separated M")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib, P = qg._lib.load(), lambda t: t.data_ptr()
    lines = []

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)
        if a.out:  # (rewritten after every line: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# {qg.version()}; us per layer, median of {a.rounds} interleaved rounds (min..max); `layers` layers per pass, each on "
         "its own copy of the weights, a one-element kernel node after every layer. NOT AHEAD: the slowest fused round is "
         "not under the fastest two-call round")
    sep = torch.zeros(1, device=dev)
    for t in [int(x) for x in a.types.split(",")]:
        for n, k in [SHAPES[int(i)] for i in a.shapes.split(",")]:
            gen = torch.Generator(device=dev)
            gen.manual_seed(t * 100003 + n + k)
            w0 = one_expert(t, n, k, gen, dev)
            layers = max(2, -(-480_000_000 // w0.numel()))
            ws = [w0] + [w0.roll(i, 0) for i in range(1, layers)]
            for M in [int(m) for m in a.m.split(",")]:
                x = torch.rand((M, k), generator=gen, device=dev) * 2 - 1
                q8 = torch.empty((M, k // 32, 36), dtype=torch.uint8, device=dev)
                out_f, out_t = (torch.zeros((layers, M, n), dtype=torch.float32, device=dev) for _ in range(2))
                st = torch.cuda.current_stream

                def fused():
                    for w, o in zip(ws, out_f):
                        qg._lib.check(lib.qg_gemm_w4a8_f32_kq(P(x), P(w), P(o), M, n, k, t, st().cuda_stream), "fused")
                        sep.add_(1.0)

                def two():
                    for w, o in zip(ws, out_t):
                        qg._lib.check(lib.qg_quantize_q8_1(P(x), P(q8), M * k, st().cuda_stream), "quantize")
                        qg._lib.check(lib.qg_gemm_w4a8(P(q8), P(w), P(o), M, n, k, t, st().cuda_stream), "product")
                        sep.add_(1.0)

                fused(), two()
                torch.cuda.synchronize()
                same = torch.equal(out_f.view(torch.int32), out_t.view(torch.int32))
                for mode, timer in (("captured", graph_time_us), ("eager", eager_time_us)):
                    times = {"fused": [], "two": []}
                    for _ in range(a.rounds):
                        for arm, fn in (("fused", fused), ("two", two)):
                            times[arm].append(timer(fn, 10, layers))
                    cell = lambda v: f"{statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f})"
                    f, s = times["fused"], times["two"]
                    emit(f"{NAMES[t]} N={n} K={k} M={M} {mode} layers={layers}: fused {cell(f)}  two {cell(s)}  fused/two "
                         f"{statistics.median(f) / statistics.median(s):.3f}{'' if max(f) < min(s) else ' NOT AHEAD'}  "
                         f"bits {'equal' if same else 'DIFFER'}  [{qg.f32_kq_config(M, n, k, t)}]")
                del out_f, out_t
            del ws, w0


if __name__ == "__main__":
    main()
