#!/usr/bin/env python3
"""qg_gemm_w4a8_moe_glu_bias and qg_gemm_w4a8_moe_down_bias against the sequences they replace, on the same operands, in
one process (measurement tool, not product): interleaved rounds, median, HIP events on the launch stream. The protocol
of tools/ab_moe_glu.py / tools/ab_moe_down.py.
  python tools/ab_mxfp4_ffn.py [--rounds 7] [--G 8] [--out profiles/mxfp4_ffn/ab_mxfp4_ffn.txt]
gpt-oss's FFN shape, N = K = 2880, MXFP4 experts, 4 of 32 and 4 of 128, T = 1 and 8, us per token:
  glu   seq, seq'  two qg_gemm_w4a8_moe (gate, up), torch's two gathered bias adds (index_select + add_, each) and
                   gpt-oss's clamped SwiGLU in torch ops; the same arm twice: the difference of the two medians is the
                   run-to-run spread every comparison is held against;
        fused      one qg_gemm_w4a8_moe_glu_bias launch;   prod: the two product launches of seq alone;
  down  seq, seq'  qg_gemm_w4a8_moe at a_rows = n_used, torch's gathered bias add, the multiply by the router weights
                   and the sum over the token's slots;
        fused      one qg_gemm_w4a8_moe_down_bias launch;  prod: the product launch of seq alone.
One more pair of rows at Qwen3-MoE's shape with Q4_K experts, where the new entries with null biases stand against the
old ones (old, old', new): the same kernels' work with another argument block, expected within the spread.
Each class is measured "graph" (G steps captured into one hipGraph and replayed, bench.py's graph_time_us) and "eager"
(the same G steps enqueued from Python between two events). Every step's ids pick, per token, n_used distinct experts
(a uniform router) of one copy of the layer's tensors; the copies rotate over resident pools of more than 600 MB each,
so no step finds its weights in a cache. Every step of every arm is followed by a one-element kernel node.
Before anything is timed the fused results are compared with the sequences': down bit for bit with the ascending fold
done in torch, glu by its largest relative difference (torch's sigmoid is not the entry's expf chain)."""
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

ALPHA, LIMIT = 1.702, 7.0
# (name, N, K, n_expert, n_used)
GPT_OSS = [("gpt-oss-20b", 2880, 2880, 32, 4), ("gpt-oss-120b", 2880, 2880, 128, 4)]
QWEN3 = (("qwen3-moe gate/up", 768, 2048, 128, 8), ("qwen3-moe down", 2048, 768, 128, 8))
TOKENS = (1, 8)


def mxfp4_expert(n, k, gen, dev):
    """[n, k/32, 17]: uniform code bytes, scales 2^-10 .. 2^-3 (the timing does not depend on the values)."""
    w = torch.randint(0, 256, (n, k // 32, 17), generator=gen, device=dev, dtype=torch.uint8)
    w[..., 0] = torch.randint(118, 126, (n, k // 32), generator=gen, device=dev, dtype=torch.uint8)
    return w


def pool_of(w1, n_expert, G, pool_mb, dev):
    copies = max(G, math.ceil(pool_mb * 1e6 / (w1.numel() * n_expert)))
    pool = torch.empty((copies, n_expert) + tuple(w1.shape), dtype=torch.uint8, device=dev)
    pool.copy_(w1.expand_as(pool))
    return pool, copies


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--G", type=int, default=8, help="steps per graph / per eager call")
    ap.add_argument("--pool-mb", type=float, default=600.0, help="resident bytes per weight tensor the copies rotate over")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    G = a.G
    lines = [f"# {qg.version()}; us per token, median of {a.rounds} interleaved rounds (min..max), G={G} steps per graph / "
             f"eager call, each on another copy of the expert tensors in pools > {a.pool_mb:.0f} MB; a one-element kernel "
             "node after every step. spread = |seq - seq'| (|old - old'|); ahead: fused below the lower seq median by more "
             "than the spread; same: new within the spread of the lower old median"]
    sep = torch.zeros(1, device=dev)
    print(lines[0], flush=True)

    def emit(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    def measure(label, arms, T, copies, first, base, cand, verdict, tail):
        for mode, timer in (("graph", graph_time_us), ("eager", eager_time_us)):
            times = {name: [] for name, _ in arms}
            for _ in range(a.rounds):
                for name, fn in arms:
                    times[name].append(timer(fn, 10, G * T))
                    first[0] = (first[0] + G) % copies
            med = {n: statistics.median(v) for n, v in times.items()}
            spread = abs(med[base] - med[base + "'"])
            low = min(med[base], med[base + "'"])
            emit(f"{label} T={T} {mode}: " + "  ".join(f"{n} {med[n]:.3f} ({min(v):.3f}..{max(v):.3f})" for n, v in times.items()) +
                 f"  spread {spread:.3f}  {cand}/{base} {med[cand] / low:.3f}  {verdict(med[cand], low, spread)}  {tail}")

    ahead = lambda c, low, spread: "ahead" if c < low - spread else "NOT AHEAD"
    same = lambda c, low, spread: "same" if abs(c - low) <= spread else ("faster" if c < low else "SLOWER")

    for lname, N, K, n_expert, n_used in GPT_OSS:
        gen = torch.Generator(device=dev)
        gen.manual_seed(N + K + n_expert)
        pools = [pool_of(mxfp4_expert(N, K, gen, dev), n_expert, G, a.pool_mb, dev) for _ in range(3)]
        (pg, copies), (pu, _), (pd, _) = pools
        bias = [(torch.rand((n_expert, N), generator=gen, device=dev) * 2 - 1) * 4 for _ in range(3)]
        for T in TOKENS:
            a1 = qg.quantize_q8_1((torch.rand((T, K), generator=gen, device=dev) * 2 - 1) * 0.5).reshape(T, K // 32, 36)
            an = qg.quantize_q8_1((torch.rand((T * n_used, K), generator=gen, device=dev) * 2 - 1) * 0.5)
            an = an.reshape(T, n_used, K // 32, 36)
            ids_d = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32).to(dev) for _ in range(G)]
            ids_l = [i.long().reshape(-1) for i in ids_d]
            rw = torch.softmax(torch.rand((G, T, n_used), generator=gen, device=dev) * 4, dim=-1).contiguous()
            gbuf = torch.zeros((G, T, n_used, N), dtype=torch.float32, device=dev)
            ubuf, hbuf = torch.zeros_like(gbuf), torch.zeros_like(gbuf)
            gath = torch.zeros((T * n_used, N), dtype=torch.float32, device=dev)
            tmp = torch.zeros((T, n_used, N), dtype=torch.float32, device=dev)
            ybuf = torch.zeros((G, T, N), dtype=torch.float32, device=dev)
            first = [0]
            cp = lambda j: (first[0] + j) % copies

            def add_bias(x, b, j):  # torch's gathered bias add: two kernels
                torch.index_select(b, 0, ids_l[j], out=gath)
                x.add_(gath.view(T, n_used, N))

            def glu_prod(j):
                qg.gemm_w4a8_moe(a1, pg[cp(j)], ids_d[j], T, n_used, N, K, qg.MXFP4, out=gbuf[j])
                qg.gemm_w4a8_moe(a1, pu[cp(j)], ids_d[j], T, n_used, N, K, qg.MXFP4, out=ubuf[j])

            def glu_seq():
                for j in range(G):
                    glu_prod(j)
                    add_bias(gbuf[j], bias[0], j)
                    add_bias(ubuf[j], bias[1], j)
                    x = gbuf[j].clamp_(max=LIMIT)
                    y = ubuf[j].clamp_(-LIMIT, LIMIT).add_(1.0)
                    torch.mul(x, ALPHA, out=tmp)
                    tmp.sigmoid_().mul_(x)
                    torch.mul(tmp, y, out=hbuf[j])
                    sep.add_(1.0)

            def glu_prod_only():
                for j in range(G):
                    glu_prod(j)
                    sep.add_(1.0)

            def glu_fused():
                for j in range(G):
                    qg.gemm_w4a8_moe_glu_bias(a1, pg[cp(j)], pu[cp(j)], bias[0], bias[1], ids_d[j], T, n_used, N, K, qg.MXFP4,
                                              qg.GLU_SWIGLU_OAI, ALPHA, LIMIT, out=hbuf[j])
                    sep.add_(1.0)

            def down_prod(j):
                qg.gemm_w4a8_moe(an, pd[cp(j)], ids_d[j], T, n_used, N, K, qg.MXFP4, a_rows=n_used, out=gbuf[j])

            def down_seq():
                for j in range(G):
                    down_prod(j)
                    add_bias(gbuf[j], bias[2], j)
                    torch.mul(gbuf[j], rw[j].unsqueeze(-1), out=tmp)
                    torch.sum(tmp, 1, out=ybuf[j])
                    sep.add_(1.0)

            def down_prod_only():
                for j in range(G):
                    down_prod(j)
                    sep.add_(1.0)

            def down_fused():
                for j in range(G):
                    qg.gemm_w4a8_moe_down_bias(an, pd[cp(j)], bias[2], ids_d[j], rw[j], T, n_used, N, K, qg.MXFP4, out=ybuf[j])
                    sep.add_(1.0)

            # the results agree before anything is timed
            glu_seq()
            ref = hbuf.clone()
            glu_fused()
            torch.cuda.synchronize()
            glu_rel = ((hbuf - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
            down_seq()
            fold = torch.zeros_like(ybuf)
            for u in range(n_used):
                fold = fold + rw[:, :, u].unsqueeze(-1) * gbuf[:, :, u]
            ybuf.zero_()
            down_fused()
            torch.cuda.synchronize()
            bits = "==" if torch.equal(ybuf.view(torch.int32), fold.view(torch.int32)) else "DIFFER"
            del ref, fold

            label = f"{lname} N={N} K={K} E={n_expert} used={n_used} MXFP4"
            measure(label + " glu", [("seq", glu_seq), ("seq'", glu_seq), ("fused", glu_fused), ("prod", glu_prod_only)], T, copies,
                    first, "seq", "fused", ahead,
                    f"max rel diff to torch's op {glu_rel:.2e}  [{qg.moe_glu_bias_config(T, n_used, N, K, qg.MXFP4)}]")
            measure(label + " down", [("seq", down_seq), ("seq'", down_seq), ("fused", down_fused), ("prod", down_prod_only)], T,
                    copies, first, "seq", "fused", ahead,
                    f"fold bits {bits}  [{qg.moe_down_bias_config(T, n_used, N, K, qg.MXFP4)}]")
            del gbuf, ubuf, hbuf, ybuf
        del pools, pg, pu, pd

    # Q4_K at Qwen3-MoE's shape: the new entries with null biases against the old ones
    for (lname, N, K, n_expert, n_used), down in zip(QWEN3, (False, True)):
        gen = torch.Generator(device=dev)
        gen.manual_seed(N + K)
        (pw, copies), (pv, _) = (pool_of(one_expert(qg.Q4_K, N, K, gen, dev), n_expert, G, a.pool_mb, dev) for _ in range(2))
        for T in TOKENS:
            rows = T * n_used if down else T
            aq = qg.quantize_q8_1((torch.rand((rows, K), generator=gen, device=dev) * 2 - 1) * 0.02)
            aq = aq.reshape((T, n_used, K // 32, 36) if down else (T, K // 32, 36))
            ids_d = [torch.stack([torch.randperm(n_expert)[:n_used] for _ in range(T)]).to(torch.int32).to(dev) for _ in range(G)]
            rw = torch.softmax(torch.rand((G, T, n_used), generator=gen, device=dev) * 4, dim=-1).contiguous()
            out = torch.zeros((G, T, N) if down else (G, T, n_used, N), dtype=torch.float32, device=dev)
            first = [0]
            cp = lambda j: (first[0] + j) % copies

            def old():
                for j in range(G):
                    if down:
                        qg.gemm_w4a8_moe_down(aq, pw[cp(j)], ids_d[j], rw[j], T, n_used, N, K, qg.Q4_K, out=out[j])
                    else:
                        qg.gemm_w4a8_moe_glu(aq, pw[cp(j)], pv[cp(j)], ids_d[j], T, n_used, N, K, qg.Q4_K, qg.GLU_SWIGLU, out=out[j])
                    sep.add_(1.0)

            def new():
                for j in range(G):
                    if down:
                        qg.gemm_w4a8_moe_down_bias(aq, pw[cp(j)], None, ids_d[j], rw[j], T, n_used, N, K, qg.Q4_K, out=out[j])
                    else:
                        qg.gemm_w4a8_moe_glu_bias(aq, pw[cp(j)], pv[cp(j)], None, None, ids_d[j], T, n_used, N, K, qg.Q4_K,
                                                  qg.GLU_SWIGLU, out=out[j])
                    sep.add_(1.0)

            old()
            ref = out.clone()
            out.zero_()
            new()
            torch.cuda.synchronize()
            bits = "==" if torch.equal(out.view(torch.int32), ref.view(torch.int32)) else "DIFFER"
            del ref
            measure(f"{lname} N={N} K={K} E={n_expert} used={n_used} Q4_K null bias", [("old", old), ("old'", old), ("new", new)], T,
                    copies, first, "old", "new", same, f"bits {bits}")
            del out
        del pw, pv
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
