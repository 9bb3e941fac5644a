#!/usr/bin/env python3
"""Compare the GEMV / K-quant / expert kernels of two `make asm` outputs (csrc/Makefile), instantiation by instantiation.

    python tools/kq_asm_compare.py PARENT_ASM_DIR RESULT_ASM_DIR [--drop KERNEL:POS ...]

--drop w16s_kernel:2 leaves the parent's third integer / bool template argument of w16s_kernel out of the pairing key: for
a result that removed that template parameter.

Pairs the kernels of qg_q{4,6}k_{gemv,mmq}, qg_moe, qg_moe_prefill, qg_moe_batch, qg_moe_glu, qg_moe_down, qg_moe_plan, qg_gemv,
qg_gemv_q4_0 .. qg_gemv_q8_0, qg_capture_fuse and qg_w4a16 by their name and integer / bool template arguments across the whole file set (a kernel may have moved between files; a file one side
does not have is skipped there; one only the result has is a new file: NEW <file>, its kernels not paired), and compares the instruction text from each kernel's label to its end (symbol names, labels' function
numbers and comments normalised away) and the kernel-resource-usage remarks. Prints one line per file of the result and every pair
that differs: REGS where the instruction sequence and the remarks are the parent's and only register numbers moved,
DIFF otherwise; GONE <symbol> for a kernel of the parent the result no longer builds (an instantiation no shape
reached). Exit status 1 if any pair differs; a kernel only the result has is an error."""
import re
import sys
from pathlib import Path

FILES = ["qg_q4k_gemv", "qg_q4k_mmq", "qg_q6k_gemv", "qg_q6k_mmq", "qg_moe", "qg_moe_prefill", "qg_moe_batch", "qg_moe_glu",
         "qg_moe_down", "qg_moe_plan", "qg_gemv", "qg_gemv_q4_0", "qg_gemv_q4_1", "qg_gemv_q5_0", "qg_gemv_q5_1", "qg_gemv_q8_0", "qg_capture_fuse",
         "qg_w4a16"]
RES = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def key(sym):
    """The kernel's own name (the last <length><name> of the mangled nested name) and its Li<n>E / Lb<n>E template
    arguments, in order."""
    i, name = (3 if sym.startswith("_ZN") else 2), ""
    while m := re.match(r"\d+", sym[i:]):
        i += len(m.group())
        name = sym[i : i + int(m.group())]
        i += len(name)
    return (name,) + tuple(re.findall(r"L[ib](\d+)E", sym))


def masked(lines):
    """register numbers away: v12, s[4:5], a3 -> v, s[:], a"""
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", l) for l in lines]


def kernels(asm):
    """mangled name -> normalised instruction lines of every *_kernel in a .s file"""
    out, cur = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"(_Z\w*_kernel\w*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = re.sub(r";.*", "", line).strip()
        if not line or line.startswith((".loc", ".file", ".cfi")):
            continue
        line = re.sub(r"_Z\w+", "SYM", line)
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def resources(txt):
    out, cur = {}, None
    for line in txt.read_text().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r":\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in RES:
            cur[m.group(1)] = m.group(2)
    return out


def main(parent, result, drop=()):
    """drop: (kernel name, position) pairs — that integer / bool template argument is left out of the PARENT's key (the
    result removed the parameter, so its mangled names no longer carry it)."""
    side = []
    for d in (Path(parent), Path(result)):
        side.append({})
        for f in FILES:
            asm = d / f"{f}-hip-amdgcn-amd-amdhsa-gfx950.s"
            if not asm.exists():
                continue
            if len(side) == 2 and not (Path(parent) / asm.name).exists():
                print(f"NEW {f}: {len(kernels(asm))} kernels, none paired")
                continue
            k, r = kernels(asm), resources(d / f"{f}.hip.resource.txt")
            for s in k:
                kk = key(s)
                for name, pos in drop if len(side) == 1 else ():
                    if kk[0] == name:
                        kk = kk[: 1 + pos] + kk[2 + pos :]
                assert kk not in side[-1], (f, s, "two kernels with one key")
                side[-1][kk] = (f, s, k[s], r[s])
    assert side[1].keys() <= side[0].keys(), ("only in the result", sorted(side[1].keys() - side[0].keys()))
    bad = 0
    for f in FILES:
        for kk in sorted(side[0].keys() - side[1].keys()):
            if side[0][kk][0] == f:
                print(f"  GONE {side[0][kk][1]}")
        keys = sorted(kk for kk in side[1] if side[1][kk][0] == f)
        same = 0
        for kk in keys:
            (fa, sa, ia, ra), (fb, sb, ib, rb) = side[0][kk], side[1][kk]
            if fa != fb:
                print(f"  MOVED {sb}: {fa} -> {fb}")
            if ia == ib and ra == rb:
                same += 1
                continue
            bad += 1
            tag = "REGS" if ra == rb and masked(ia) == masked(ib) else "DIFF"
            print(f"  {tag} {sb}\n    parent {len(ia)} instr {ra}\n    result {len(ib)} instr {rb}")
        print(f"{f}: {len(keys)} pairs, {same} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    drops = [(a.split(":")[0], int(a.split(":")[1])) for i, a in enumerate(sys.argv[1:]) if sys.argv[i] == "--drop"]
    dirs = [a for i, a in enumerate(sys.argv[1:]) if a != "--drop" and sys.argv[i] != "--drop"]
    sys.exit(main(*dirs[:2], drop=drops))
