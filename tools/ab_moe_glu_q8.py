#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_glu_q8_1 against the two calls it replaces, on the same operands, in one process (measurement tool,
not product): interleaved rounds, median, HIP events on the launch stream.
  python tools/ab_moe_glu_q8.py [--rounds 7] [--G 8] [--out profiles/moe_glu_q8/ab_moe_glu_q8.txt]
Arms, us per slot (one slot = one (token, expert) pair: a gate product, an up product, the SwiGLU and the Q8_1 blocks of
their N outputs):
  seq, seq'  qg_gemm_w4a8_moe_glu into T * n_used * N floats, then qg_quantize_q8_1 on them, on one stream (the C entry
             into a preallocated buffer: no allocation in the figure). The same arm twice: the difference of the two
             medians is the run-to-run spread every comparison is held against;
  fused      one qg_gemm_w4a8_moe_glu_q8_1 launch;
  glu        seq's first launch alone: what the fused launch adds to the product it contains.
Classes, pools, the rotation of the weight copies, the one-element kernel node after every step, "graph" and "eager":
those of tools/ab_moe_glu.py. Before anything is timed the fused bytes are compared with seq's, for both ops."""
from __future__ import annotations

import argparse
import ctypes
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
from ab_moe_glu import LAYERS, TOKENS, TYPES, eager_time_us  # noqa: E402
from bench import graph_time_us  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=8, help="steps per graph / per eager call")
    ap.add_argument("--layers", default=None, help="comma-separated indices into LAYERS")
    ap.add_argument("--pool-mb", type=float, default=600.0, help="resident bytes per weight tensor the copies rotate over")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = qg._lib.load()
    lines = [f"# {qg.version()}; us per slot (gate product + up product + SwiGLU + Q8_1 blocks), median of {a.rounds} "
             f"interleaved rounds (min..max), G={a.G} steps per graph / eager call, each on another copy of the gate and up "
             f"tensors in pools > {a.pool_mb:.0f} MB each; a one-element kernel node after every step. spread = |seq - seq'|; "
             "ahead: fused below the lower seq median by more than the spread"]
    sep = torch.zeros(1, device=dev)
    print(lines[0], flush=True)
    layers = LAYERS if a.layers is None else [LAYERS[int(i)] for i in a.layers.split(",")]
    for lname, N, K, n_expert, n_used in layers:
        for tname, t in TYPES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + K + t)
            pools = []
            for _ in range(2):  # gate, up: different bytes
                w = one_expert(t, N, K, gen, dev)
                copies = max(a.G, math.ceil(a.pool_mb * 1e6 / (w.numel() * n_expert)))
                pool = torch.empty((copies, n_expert) + tuple(w.shape), dtype=torch.uint8, device=dev)
                pool.copy_(w.expand_as(pool))
                pools.append(pool)
            gate, up = pools
            for T in TOKENS:
                slots = T * n_used
                aq = qg.quantize_q8_1((torch.rand((T, K), generator=gen, device=dev) * 2 - 1) * 0.02)
                ids_d = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32).to(dev)
                         for _ in range(a.G)]
                h = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                hq = torch.zeros((a.G, T, n_used, N // 32, 36), dtype=torch.uint8, device=dev)
                first = [0]

                def glu(op=qg.GLU_SWIGLU, quantize=False):
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    for j in range(a.G):
                        c = (first[0] + j) % copies  # the copies rotate from timing to timing as well
                        qg.gemm_w4a8_moe_glu(aq, gate[c], up[c], ids_d[j], T, n_used, N, K, t, op, out=h[j])
                        if quantize:
                            rc = lib.qg_quantize_q8_1(h[j].data_ptr(), hq[j].data_ptr(), h[j].numel(), st)
                            assert rc == 0, rc
                        sep.add_(1.0)

                def seq(op=qg.GLU_SWIGLU):
                    glu(op, True)

                def fused(op=qg.GLU_SWIGLU):
                    for j in range(a.G):
                        c = (first[0] + j) % copies
                        qg.gemm_w4a8_moe_glu_q8_1(aq, gate[c], up[c], ids_d[j], T, n_used, N, K, t, op, out=hq[j])
                        sep.add_(1.0)

                same = True
                for op in (qg.GLU_REGLU, qg.GLU_SWIGLU):  # the bytes agree before anything is timed
                    seq(op)
                    ref = hq.clone()
                    hq.zero_()
                    fused(op)
                    torch.cuda.synchronize()
                    same = same and torch.equal(hq, ref) and bool(ref.any())
                    del ref

                arms = [("seq", seq), ("seq'", seq), ("fused", fused), ("glu", glu)]
                for mode, timer in (("graph", graph_time_us), ("eager", eager_time_us)):
                    times = {name: [] for name, _ in arms}
                    for _ in range(a.rounds):
                        for name, fn in arms:
                            times[name].append(timer(fn, 10, a.G * slots))
                            first[0] = (first[0] + a.G) % copies
                    med = {n: statistics.median(v) for n, v in times.items()}
                    spread = abs(med["seq"] - med["seq'"])
                    low = min(med["seq"], med["seq'"])
                    line = (f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T} slots={slots} {mode}: " + "  ".join(
                        f"{n} {med[n]:.3f} ({min(v):.3f}..{max(v):.3f})" for n, v in times.items()) +
                        f"  spread {spread:.3f}  fused/seq {med['fused'] / low:.3f}  fused/glu {med['fused'] / med['glu']:.3f}"
                        f"  {'ahead' if med['fused'] < low - spread else 'NOT AHEAD'}  bytes {'==' if same else 'DIFFER'}"
                        f"  [{qg.moe_glu_q8_1_config(T, n_used, N, K, t)}]")
                    print(line, flush=True)
                    lines.append(line)
                del h, hq
            del pools, gate, up, pool
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
