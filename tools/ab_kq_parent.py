#!/usr/bin/env python3
"""Another build of the library (the parent commit's) against the in-tree one, Q4_K and Q6_K products at the shapes
of tools/ab_q6k.py, timed as it does (same graphs, rotating weight copies, interleaved rounds; measurement tool, not
product). Both arms go through ctypes qg_gemm_w4a8; per shape the medians, each arm's min and max, and whether the
in-tree median exceeds the other's by more than that arm's own min-to-max spread.
  python tools/ab_kq_parent.py [--lib tools/variants/libqg_parent.so] [--out profiles/kq_shared/ab_parent_vs_result.txt]
(tools/kq_bits.py says how the other library is built.)"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "llama.cpp-quant-gemm_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import quant_gemm as qg  # noqa: E402
from ab_q6k import DEFAULT, random_kquant, rotating  # noqa: E402
from bench import graph_time_us  # noqa: E402

P = ctypes.c_void_p
ROUNDS, G = 7, 64


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    lib.qg_gemm_w4a8.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    return lib.qg_gemm_w4a8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "tools", "variants", "libqg_parent.so"))
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    arms = (("parent", load(a.lib)),
            ("result", load(os.path.join(REPO, "llama.cpp-quant-gemm_amd", "quant_gemm", "libqg_hip.so"))))
    dev = torch.device("cuda", 0)
    lines = [f"# {qg.version()}; parent library against the result, qg_gemm_w4a8, us per launch over {ROUNDS} interleaved "
             f"rounds (parent, result, parent, ...), G={G} launches per graph over rotating weight copies > 600 MB",
             "# ok: result median - parent median <= parent max - parent min"]
    print("\n".join(lines), flush=True)
    worst = 0
    for spec in DEFAULT.split(","):
        M, N, K = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(M + N + K)
        aq = qg.quantize_q8_1(torch.rand((M, K), generator=gen, device=dev) * 2 - 1)
        out = torch.empty((G, M, N), dtype=torch.float32, device=dev)
        for tname, t in (("Q4_K", qg.Q4_K), ("Q6_K", qg.Q6_K)):
            cp = rotating(random_kquant(t, N, K, gen, dev), G)

            def step_of(f):
                def run():
                    cs = P(torch.cuda.current_stream().cuda_stream)
                    for j in range(G):
                        rc = f(P(aq.data_ptr()), P(cp[j].data_ptr()), P(out[j].data_ptr()), M, N, K, t, cs)
                        if rc != 0:
                            raise RuntimeError(f"status {rc}")
                return run

            times = {n: [] for n, _ in arms}
            for _ in range(ROUNDS):
                for n, f in arms:
                    times[n].append(graph_time_us(step_of(f), 10, G))
            bits = []
            for n, f in arms:
                step_of(f)()
                torch.cuda.synchronize()
                bits.append(out[0].clone().view(torch.int32))
            med = {n: statistics.median(v) for n, v in times.items()}
            spread = max(times["parent"]) - min(times["parent"])
            ok = med["result"] - med["parent"] <= spread
            worst += not ok
            line = (f"{tname} M={M} N={N} K={K}: " + "  ".join(
                f"{n} {med[n]:.3f} (min {min(times[n]):.3f} max {max(times[n]):.3f})" for n, _ in arms) +
                f"  diff {med['result'] - med['parent']:+.3f}  parent spread {spread:.3f}  {'ok' if ok else 'SLOWER'}"
                f"  bits {'==' if torch.equal(bits[0], bits[1]) else 'DIFFER'}  cfg {qg.debug_config(M, N, K, t)}")
            print(line, flush=True)
            lines.append(line)
            del cp
        del out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if worst else 0


if __name__ == "__main__":
    sys.exit(main())
