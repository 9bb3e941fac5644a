#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_glu against the three-kernel sequence it replaces, on the same operands, in one process
(measurement tool, not product): interleaved rounds, median, HIP events on the launch stream.
  python tools/ab_moe_glu.py [--rounds 7] [--G 8] [--out profiles/moe_glu/ab_moe_glu.txt]
Arms, us per slot (one slot = one (token, expert) pair: a gate product, an up product and the GLU of their N outputs):
  seq, seq'  the sequence a caller runs without the entry: qg_gemm_w4a8_moe on the gate experts, qg_gemm_w4a8_moe on
             the up experts, then torch's silu(g) * u (torch.nn.functional.silu in place, then torch.mul into the
             output: two elementwise kernels, torch has no fused one). The same arm twice: the difference of the two
             medians is the run-to-run spread every comparison is held against;
  fused      one qg_gemm_w4a8_moe_glu launch (SwiGLU);
  two        the two product launches of seq alone, no activation: what the fused launch has to beat to gain on the
             products themselves and not only on the activation kernels.
Each class is measured twice: "graph", G steps captured into one hipGraph and replayed (bench.py's graph_time_us), and
"eager", the same G steps enqueued from Python between two events (the host's launch path is part of the figure).
Every step's ids pick, per token, n_used distinct experts (a uniform router) of one copy of the layer's gate and up
tensors; the copies rotate over a resident pool of more than 600 MB per tensor, so no step finds its weights in a cache.
Every step of every arm is followed by a one-element kernel node, as in tools/ab_moe.py.
Before anything is timed the fused ReGLU result is compared bit for bit with relu(g) * u from the sequence's g and u,
and the fused SwiGLU result with torch's silu(g) * u (largest relative difference printed; torch's silu is another
rounding of the same function).
--variant-lib PATH adds the arm "variant": the same fused call through another build of the library (an A/B build of
csrc/Makefile, e.g. EXTRA=-DQG_MOE_GLU_STAGE_ONCE=0), loaded on its own; its bits must equal the fused arm's."""
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
import torch.nn.functional as F  # noqa: E402

import quant_gemm as qg  # noqa: E402
from ab_moe import one_expert  # noqa: E402
from bench import graph_time_us  # noqa: E402

# (name, N, K, n_expert, n_used): the gate / up shapes
LAYERS = [("mixtral", 14336, 4096, 8, 2), ("qwen3-moe", 768, 2048, 128, 8)]
TYPES = (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K))
TOKENS = (1, 8)


def eager_time_us(fn, reps: int = 10, per: int = 1) -> float:
    """fn() enqueued `reps` times from Python between two events on the current stream, after two warm-up calls."""
    fn()
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
    ap.add_argument("--G", type=int, default=8, help="steps per graph / per eager call")
    ap.add_argument("--layers", default=None, help="comma-separated indices into LAYERS")
    ap.add_argument("--pool-mb", type=float, default=600.0, help="resident bytes per weight tensor the copies rotate over")
    ap.add_argument("--variant-lib", default=None, help="another build of libqg_hip.so: the arm 'variant'")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    vlib = None
    if a.variant_lib:
        vlib = ctypes.CDLL(os.path.abspath(a.variant_lib), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        vlib.qg_gemm_w4a8_moe_glu.argtypes = [P, P, P, I, P, I64, P, I64, I, I, I, I, I, I, P]
        vlib.qg_gemm_w4a8_moe_glu.restype = I
    lines = [f"# {qg.version()}; us per slot (gate product + up product + SwiGLU), median of {a.rounds} interleaved rounds "
             f"(min..max), G={a.G} steps per graph / eager call, each on another copy of the gate and up tensors in pools "
             f"> {a.pool_mb:.0f} MB each; a one-element kernel node after every step. spread = |seq - seq'|; ahead: fused "
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
                # small activations keep g where silu bends (|g| of a few units) instead of saturating it
                aq = qg.quantize_q8_1((torch.rand((T, K), generator=gen, device=dev) * 2 - 1) * 0.02)
                ids_d = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32).to(dev)
                         for _ in range(a.G)]
                out = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                g = torch.zeros_like(out)
                u = torch.zeros_like(out)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def products(j):
                    c = copy_of(j)
                    qg.gemm_w4a8_moe(aq.unsqueeze(1), gate[c], ids_d[j], T, n_used, N, K, t, a_rows=1, out=g[j])
                    qg.gemm_w4a8_moe(aq.unsqueeze(1), up[c], ids_d[j], T, n_used, N, K, t, a_rows=1, out=u[j])

                def seq():
                    for j in range(a.G):
                        products(j)
                        torch.mul(F.silu(g[j], inplace=True), u[j], out=out[j])
                        sep.add_(1.0)

                def two():
                    for j in range(a.G):
                        products(j)
                        sep.add_(1.0)

                def fused(op=qg.GLU_SWIGLU):
                    for j in range(a.G):
                        c = copy_of(j)
                        qg.gemm_w4a8_moe_glu(aq, gate[c], up[c], ids_d[j], T, n_used, N, K, t, op, out=out[j])
                        sep.add_(1.0)

                def variant(op=qg.GLU_SWIGLU):
                    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    for j in range(a.G):
                        c = copy_of(j)
                        rc = vlib.qg_gemm_w4a8_moe_glu(aq.data_ptr(), gate[c].data_ptr(), up[c].data_ptr(), n_expert,
                                                       ids_d[j].data_ptr(), n_used, out[j].data_ptr(), N, T, n_used, N, K, t,
                                                       op, st)
                        assert rc == 0, rc
                        sep.add_(1.0)

                # the results agree before anything is timed
                seq()
                ref = out.clone()
                two()  # g again (seq's silu ran in place)
                relu_ref = torch.relu(g) * u
                out.zero_()
                fused()
                torch.cuda.synchronize()
                rel = ((out - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
                glo, ghi = g.min().item(), g.max().item()
                out.zero_()
                fused(qg.GLU_REGLU)
                torch.cuda.synchronize()
                same = torch.equal(out.view(torch.int32), relu_ref.view(torch.int32))
                vsame = ""
                if vlib is not None:
                    fused()
                    fres = out.clone()
                    out.zero_()
                    variant()
                    torch.cuda.synchronize()
                    vsame = f"  variant bits {'==' if torch.equal(out.view(torch.int32), fres.view(torch.int32)) else 'DIFFER'}"
                    del fres
                del ref, relu_ref

                arms = [("seq", seq), ("seq'", seq), ("fused", fused), ("two", two)] + ([("variant", variant)] if vlib else [])
                for mode, timer in (("graph", graph_time_us), ("eager", eager_time_us)):
                    times = {name: [] for name, _ in arms}
                    for _ in range(a.rounds):
                        for name, fn in arms:
                            times[name].append(timer(fn, 10, a.G * slots))
                            first[0] = (first[0] + a.G) % copies
                    med = {n: statistics.median(v) for n, v in times.items()}
                    spread = abs(med["seq"] - med["seq'"])
                    low = min(med["seq"], med["seq'"])
                    ahead = med["fused"] < low - spread
                    emit(f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T} slots={slots} {mode}: " + "  ".join(
                        f"{n} {med[n]:.3f} ({min(v):.3f}..{max(v):.3f})" for n, v in times.items()) +
                        f"  spread {spread:.3f}  fused/seq {med['fused'] / low:.3f}  fused/two {med['fused'] / med['two']:.3f}"
                        + (f"  fused/variant {med['fused'] / med['variant']:.3f}" if vlib else "") + vsame +
                        f"  {'ahead' if ahead else 'NOT AHEAD'}  reglu bits {'==' if same else 'DIFFER'}  swiglu max rel diff "
                        f"to torch {rel:.2e} (g in {glo:.3g}..{ghi:.3g})  [{qg.moe_glu_config(T, n_used, N, K, t)}]")
                del out, g, u
            del pools, gate, up, pool
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
