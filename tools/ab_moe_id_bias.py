#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_prefill_bias and qg_gemm_w4a8_moe_batch_bias against what a caller can do without them, on the same
operands, in one process (measurement tool, not product): interleaved rounds, median, HIP events on the launch stream.
The protocol of tools/ab_mxfp4_ffn.py.
  python tools/ab_moe_id_bias.py [--rounds 7] [--G 4] [--out profiles/moe_id_bias/ab_moe_id_bias.txt]
                                 [--forms 1=PATH,2=PATH,3=PATH,4=PATH]
gpt-oss's FFN shape, N = K = 2880, MXFP4 experts, 4 of 32 and 4 of 128, us per call (one mul_mat_id of T tokens):
  prefill T = 16, 64, 256, 1024
    seq, seq'  qg_gemm_w4a8_moe (one pass over the expert per slot) and torch's gathered bias add (index_select + add_):
               what the caller of the previous release does; the same arm twice: the difference of the two medians is
               the run-to-run spread every comparison is held against;
    new        one qg_gemm_w4a8_moe_prefill_bias call (plan + product);
    eager      one qg_gemm_w4a8 per expert with slots, on rows gathered beforehand (outside the timed region) and with
               the counts known to the host -- no gather, no scatter, no bias: a lower bound on a host-driven loop;
  batch T = 8, 16, 32, 64
    seq, seq'  as above;   new  one qg_gemm_w4a8_moe_batch_bias call;   prefill  one qg_gemm_w4a8_moe_prefill_bias call.
  --forms: the prefill entry of other builds of the library (make EXTRA=-DQG_MOE_PREFILL_FORM=1..4, which force
    (TT, RG) = (1,1) (2,1) (4,1) (4,4)) at T = 64 and 256 beside this build's choice.
Each class is measured "graph" (G steps captured into one hipGraph and replayed, bench.py's graph_time_us) and "eager"
(the same G steps enqueued from Python between two events). Every step's ids pick, per token, n_used distinct experts
(a uniform router) of one copy of the expert tensor; the copies rotate over a resident pool of more than 600 MB, so no
step finds its weights in a cache. Every step of every arm is followed by a one-element kernel node.
Before anything is timed the new entries' results are compared bit for bit: batch with seq (the same product bits, the
same float32 add), prefill with the batch entry within the MFMA family's bound (its K-slice order differs)."""
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
import quant_gemm._lib as L  # noqa: E402
from ab_moe_glu import eager_time_us  # noqa: E402
from ab_mxfp4_ffn import mxfp4_expert, pool_of  # noqa: E402
from bench import graph_time_us  # noqa: E402

# (name, N, K, n_expert, n_used)
GPT_OSS = [("gpt-oss-20b", 2880, 2880, 32, 4), ("gpt-oss-120b", 2880, 2880, 128, 4)]
PREFILL_T = (16, 64, 256, 1024)
BATCH_T = (8, 16, 32, 64)
FORMS_T = (64, 256)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=4, help="steps per graph / per eager call")
    ap.add_argument("--pool-mb", type=float, default=600.0, help="resident bytes of the expert tensor the copies rotate over")
    ap.add_argument("--forms", default=None, help="name=path,... of other builds of libqg_hip.so (forced prefill forms)")
    ap.add_argument("--only", default=None, help="prefill, batch or forms: that part alone")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G = a.G
    lines = [f"# {qg.version()}; us per call of T tokens, median of {a.rounds} interleaved rounds (min..max), G={G} steps per "
             f"graph / eager call, each on another copy of the expert tensor in a pool > {a.pool_mb:.0f} MB; a one-element "
             "kernel node after every step. spread = |seq - seq'|; ahead: new below the lower seq median by more than the spread"]
    sep = torch.zeros(1, device=dev)
    print(lines[0], flush=True)
    variants = []
    for item in (a.forms.split(",") if a.forms else []):
        name, path = item.split("=")
        lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        for sym in ("qg_gemm_w4a8_moe_prefill_bias", "qg_moe_prefill_bias_config"):
            getattr(lib, sym).argtypes, getattr(lib, sym).restype = L.SIGNATURES[sym]
        variants.append((name, lib))

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    def measure(label, arms, copies, first, tail, base="seq", cands=("new",)):
        for mode, timer in (("graph", graph_time_us), ("eager", eager_time_us)):
            times = {name: [] for name, _ in arms}
            for _ in range(a.rounds):
                for name, fn in arms:
                    times[name].append(timer(fn, 10, G))
                    first[0] = (first[0] + G) % copies
            med = {n: statistics.median(v) for n, v in times.items()}
            spread = abs(med[base] - med[base + "'"])
            low = min(med[base], med[base + "'"])
            verdicts = "  ".join(f"{c}/{base} {med[c] / low:.3f} {'ahead' if med[c] < low - spread else 'NOT AHEAD'}" for c in cands)
            emit(f"{label} {mode}: " + "  ".join(f"{n} {med[n]:.2f} ({min(v):.2f}..{max(v):.2f})" for n, v in times.items()) +
                 f"  spread {spread:.2f}  {verdicts}  {tail}")

    P = ctypes.c_void_p
    for lname, N, K, n_expert, n_used in GPT_OSS:
        gen = torch.Generator(device=dev)
        gen.manual_seed(N + K + n_expert)
        pool, copies = pool_of(mxfp4_expert(N, K, gen, dev), n_expert, G, a.pool_mb, dev)
        bias = (torch.rand((n_expert, N), generator=gen, device=dev) * 2 - 1) * 4
        for T in sorted(set(PREFILL_T + BATCH_T)):
            parts = [p for p in ("prefill", "batch", "forms") if (a.only in (None, p)) and
                     T in {"prefill": PREFILL_T, "batch": BATCH_T, "forms": FORMS_T if variants else ()}[p]]
            if not parts:
                continue
            S = T * n_used
            a1 = qg.quantize_q8_1((torch.rand((T, K), generator=gen, device=dev) * 2 - 1) * 0.5).reshape(T, 1, K // 32, 36)
            ids_h = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32) for _ in range(G)]
            ids_d = [i.to(dev) for i in ids_h]
            ids_l = [i.long().reshape(-1) for i in ids_d]
            out = torch.zeros((G, T, n_used, N), dtype=torch.float32, device=dev)
            gath = torch.zeros((S, N), dtype=torch.float32, device=dev)
            ws_p = torch.empty(qg.moe_prefill_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
            ws_b = torch.empty(qg.moe_batch_workspace_size(T, n_used, n_expert), dtype=torch.uint8, device=dev)
            # the eager arm's operands: per step the slots' rows gathered in expert order, and the counts on the host
            order = [torch.sort(i.reshape(-1), stable=True)[1] for i in ids_h]
            counts = [torch.bincount(i.reshape(-1), minlength=n_expert).tolist() for i in ids_h]
            a_sorted = [a1.reshape(T, K // 32, 36)[(o // n_used).to(dev)].contiguous() for o in order]
            out_sorted = torch.zeros((S, N), dtype=torch.float32, device=dev)
            first = [0]
            cp = lambda j: (first[0] + j) % copies

            def seq():
                for j in range(G):
                    qg.gemm_w4a8_moe(a1, pool[cp(j)], ids_d[j], T, n_used, N, K, qg.MXFP4, out=out[j])
                    torch.index_select(bias, 0, ids_l[j], out=gath)
                    out[j].add_(gath.view(T, n_used, N))
                    sep.add_(1.0)

            def new_prefill():
                for j in range(G):
                    qg.gemm_w4a8_moe_prefill_bias(a1, pool[cp(j)], bias, ids_d[j], T, n_used, N, K, qg.MXFP4, workspace=ws_p, out=out[j])
                    sep.add_(1.0)

            def new_batch():
                for j in range(G):
                    qg.gemm_w4a8_moe_batch_bias(a1, pool[cp(j)], bias, ids_d[j], T, n_used, N, K, qg.MXFP4, workspace=ws_b, out=out[j])
                    sep.add_(1.0)

            def per_expert():
                for j in range(G):
                    w, r0 = pool[cp(j)], 0
                    for e, m in enumerate(counts[j]):
                        if m:
                            qg.gemm_w4a8(a_sorted[j][r0:r0 + m], w[e], m, N, K, qg.MXFP4, out=out_sorted[r0:r0 + m])
                            r0 += m
                    sep.add_(1.0)

            def variant(lib):
                def run():
                    st = P(torch.cuda.current_stream().cuda_stream)  # (per call: a capture runs on a stream of its own)
                    for j in range(G):
                        rc = lib.qg_gemm_w4a8_moe_prefill_bias(P(a1.data_ptr()), 1, P(pool[cp(j)].data_ptr()), P(bias.data_ptr()), N,
                                                               n_expert, P(ids_d[j].data_ptr()), n_used, P(out[j].data_ptr()), N, T,
                                                               n_used, N, K, qg.MXFP4, P(ws_p.data_ptr()), ws_p.numel(), st)
                        assert rc == 0, rc
                        sep.add_(1.0)
                return run

            # the results agree before anything is timed
            seq()
            ref = out.clone()
            out.zero_()
            verdict = []
            if S <= 65535 and qg.moe_batch_bias_config(T, n_used, n_expert, N, K, qg.MXFP4):
                new_batch()
                torch.cuda.synchronize()
                verdict.append("batch bits " + ("==" if torch.equal(out.view(torch.int32), ref.view(torch.int32)) else "DIFFER"))
                out.zero_()
            new_prefill()
            torch.cuda.synchronize()
            verdict.append(f"prefill max |diff| / max |ref| {((out - ref).abs().max() / ref.abs().max()).item():.1e}")
            del ref
            label = f"{lname} N={N} K={K} E={n_expert} used={n_used} MXFP4 T={T}"
            if "prefill" in parts:
                measure(label + " prefill", [("seq", seq), ("seq'", seq), ("new", new_prefill), ("eager", per_expert)], copies, first,
                        f"{'; '.join(verdict)}  [{qg.moe_prefill_bias_config(T, n_used, n_expert, N, K, qg.MXFP4)}]", cands=("new", "eager"))
            if "batch" in parts:
                measure(label + " batch", [("seq", seq), ("seq'", seq), ("new", new_batch), ("prefill", new_prefill)], copies, first,
                        f"{'; '.join(verdict)}  [{qg.moe_batch_bias_config(T, n_used, n_expert, N, K, qg.MXFP4)}]", cands=("new", "prefill"))
            if "forms" in parts:
                arms = [("seq", new_prefill), ("seq'", new_prefill)] + [(name, variant(lib)) for name, lib in variants]
                measure(label + " forms (seq = this build's choice)", arms, copies, first,
                        f"[{qg.moe_prefill_bias_config(T, n_used, n_expert, N, K, qg.MXFP4)}]", cands=tuple(n for n, _ in variants))
            del out, gath, a_sorted, out_sorted
        del pool
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
