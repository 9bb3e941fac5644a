#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_prefill against the decode entry and against per-expert eager products, in one process, timed as
bench.py does (measurement tool, not product): G steps per hipGraph, HIP events on the launch stream, interleaved
rounds, median with the spread.
  python tools/ab_moe_prefill.py [--rounds 7] [--G 4] [--layers 0,1] [--tokens 16,64,256,1024] [--out FILE]
Arms, us per call (one call = the T * n_used expert products of one projection):
  (a) prefill  qg_gemm_w4a8_moe_prefill, the plan kernel included;
  (b) decode   qg_gemm_w4a8_moe on the same operands: what the library did for these shapes before;
  (c) eager    one qg_gemm_w4a8 node per expert that has rows, on rows gathered beforehand with host-known counts:
               the ceiling a synchronising caller reaches, the gather and the scatter not charged;
  plan         qg_debug_moe_prefill_plan: the plan kernel plus two small device copies (counts, sorted list).
Every step's ids come from a seeded router: n_used distinct experts per token drawn uniformly, or ("skew") every slot
on expert 0 with probability 1/2 and uniform otherwise. Each step works on another copy of the layer's expert tensor;
the copies rotate over a resident pool of more than 600 MB, so no step finds its weights in a cache. The down
projection (K > N) takes one activation row per slot, gate / up one per token. Every step of every arm is followed
by a one-element kernel node, as in tools/ab_moe.py. Before anything is timed (a) is compared with (c) (relative to
the largest output; the bits are the tests' business)."""
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

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from quant_gemm import _lib  # noqa: E402
from bench import graph_time_us  # noqa: E402
from tools.ab_moe import LAYERS, one_expert  # noqa: E402

TYPES = (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K))


def router(T: int, n_used: int, n_expert: int, skew: bool, gen: torch.Generator) -> torch.Tensor:
    if skew:
        ids = torch.randint(0, n_expert, (T, n_used), generator=gen)
        return torch.where(torch.rand((T, n_used), generator=gen) < 0.5, torch.zeros_like(ids), ids).to(torch.int32)
    return torch.stack([torch.randperm(n_expert, generator=gen)[:n_used] for _ in range(T)]).to(torch.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=4, help="steps per graph")
    ap.add_argument("--layers", default=None, help="comma-separated indices into tools/ab_moe.py LAYERS")
    ap.add_argument("--tokens", default="16,64,256,1024")
    ap.add_argument("--skew-tokens", default="256", help="T of the skewed cases")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--libs", nargs="*", default=[], help="A/B builds of the library (e.g. make EXTRA=-DQG_MOE_PREFILL_FORM=k "
                    "BUILD=build_mpfk OUT=...): their prefill entry is timed as further arms, named by file")
    ap.add_argument("--forms-only", action="store_true", help="time the prefill arms only")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    variants = []
    for path in a.libs:
        lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        lib.qg_gemm_w4a8_moe_prefill.argtypes = _lib.SIGNATURES["qg_gemm_w4a8_moe_prefill"][0]
        lib.qg_gemm_w4a8_moe_prefill.restype = ctypes.c_int
        variants.append((os.path.basename(path), lib))
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
         "one-element kernel node after every step")
    sep = torch.zeros(1, device=dev)
    layers = LAYERS if a.layers is None else [LAYERS[int(i)] for i in a.layers.split(",")]
    cases = [(int(x), False) for x in a.tokens.split(",") if x] + [(int(x), True) for x in a.skew_tokens.split(",") if x]
    cpu_gen = torch.Generator()
    for lname, N, K, n_expert, n_used in layers:
        a_rows = n_used if K > N else 1
        for tname, t in TYPES:
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
                ids_h = [router(T, n_used, n_expert, skew, cpu_gen) for _ in range(a.G)]
                ids_d = [i.to(dev) for i in ids_h]
                out = torch.zeros((a.G, T, n_used, N), dtype=torch.float32, device=dev)
                ws = torch.empty(qg.moe_prefill_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
                # arm (c): per step and expert, the slots, their gathered activation rows and an output of their own
                aflat = aq.reshape(T * a_rows, K // 32, 36)
                groups = []
                for j in range(a.G):
                    flat = ids_h[j].reshape(-1)
                    g = []
                    for e in range(n_expert):
                        sl = torch.nonzero(flat == e).reshape(-1)
                        if len(sl):
                            rows = (sl // n_used) * a_rows + (sl % n_used) % a_rows
                            g.append((e, sl.to(dev), aflat[rows.to(dev)].contiguous(),
                                      torch.zeros((len(sl), N), dtype=torch.float32, device=dev)))
                    groups.append(g)
                first = [0]

                def copy_of(j):  # the copies rotate from timing to timing as well
                    return (first[0] + j) % copies

                def prefill():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe_prefill(aq, pool[copy_of(j)], ids_d[j], T, n_used, N, K, t, a_rows=a_rows, workspace=ws,
                                                 out=out[j])
                        sep.add_(1.0)

                def decode():
                    for j in range(a.G):
                        qg.gemm_w4a8_moe(aq, pool[copy_of(j)], ids_d[j], T, n_used, N, K, t, a_rows=a_rows, out=out[j])
                        sep.add_(1.0)

                def eager():
                    for j in range(a.G):
                        p = pool[copy_of(j)]
                        for e, _, rows, o in groups[j]:
                            qg.gemm_w4a8(rows, p[e], rows.shape[0], N, K, t, out=o)
                        sep.add_(1.0)

                def plan():
                    for j in range(a.G):
                        qg.debug_moe_prefill_plan(ids_d[j], n_expert, N, K, t, a_rows=a_rows, workspace=ws)
                        sep.add_(1.0)

                # (a) against (c) before anything is timed
                prefill()
                eager()
                torch.cuda.synchronize()
                worst = 0.0
                for j in range(a.G):
                    flat = out[j].reshape(slots, N)
                    for e, sl, _, o in groups[j]:
                        worst = max(worst, float((flat[sl] - o).abs().max() / o.abs().max().clamp_min(1e-30)))
                def variant(lib):
                    def fn():
                        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                        for j in range(a.G):
                            rc = lib.qg_gemm_w4a8_moe_prefill(aq.data_ptr(), a_rows, pool[copy_of(j)].data_ptr(), n_expert,
                                                              ids_d[j].data_ptr(), n_used, out[j].data_ptr(), N, T, n_used, N, K,
                                                              t, ws.data_ptr(), ws.numel(), st)
                            assert rc == 0, rc
                            sep.add_(1.0)
                    return fn

                arms = [("prefill", prefill), ("decode", decode), ("eager", eager), ("plan", plan)]
                if a.forms_only:
                    arms = arms[:2]
                arms += [(name, variant(lib)) for name, lib in variants]
                reps = 10 if slots <= 512 else 4
                times = {name: [] for name, _ in arms}
                for _ in range(a.rounds):
                    for name, fn in arms:
                        times[name].append(graph_time_us(fn, reps, a.G))
                        first[0] = (first[0] + a.G) % copies
                med = {n: statistics.median(v) for n, v in times.items()}
                emit(f"{lname} N={N} K={K} E={n_expert} used={n_used} {tname} T={T}{' skew' if skew else ''} slots={slots}: " +
                     "  ".join(f"{n} {med[n]:.1f} ({min(v):.1f}..{max(v):.1f})" for n, v in times.items()) +
                     f"  prefill/decode {med['prefill'] / med['decode']:.3f}" +
                     (f"  prefill/eager {med['prefill'] / med['eager']:.3f}" if "eager" in med else "") +
                     f"  |a-c|/max {worst:.1e}  [{qg.moe_prefill_config(T, n_used, n_expert, N, K, t)}]")
                del out, groups, ws
            del pool


if __name__ == "__main__":
    main()
