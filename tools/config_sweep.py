#!/usr/bin/env python3
"""Every kernel choice the host side makes, over a fixed grid of shapes: one line `entry args -> rc "config"` per query
(qg_select_algo's answer rides on the qg_debug_config line of its shape).

    python tools/config_sweep.py [--lib PATH/libqg_hip.so] > sweep.txt

Nothing is launched and no GPU is needed (without one device_cus() is 256, so the output is deterministic). Run it on two
builds and diff the outputs: a refactor of the dispatch (the instantiation ladders of qg_kq_launch.hpp and
qg_gemv_impl.hpp, the unit form and workgroup rules of qg_gemv_kernel.hpp) must leave the diff empty, a retune shows
exactly the shapes it moves. --lib names the library to query (default: the one built next to the package); the
signatures are the package's."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd"))

ROW_TYPES, KQ_TYPES = (2, 3, 6, 7, 8), (12, 14)
ROW_K = (64, 96, 256, 512, 1024, 2048, 2304, 4096, 4128, 4352, 8192, 11008, 14336, 16384)
KQ_K = tuple(sorted({k for k in ROW_K if k % 256 == 0} | {768}))
NS = (1, 300, 4096, 8192, 20000)
MOE = ((1, 2, 4), (3, 2, 8), (64, 8, 128))  # (T, n_used, n_expert)
W16_TYPES = (2, 8)
W16_M = tuple(range(1, 9)) + (9, 16, 17, 24, 32, 33, 40, 64, 65, 100, 128, 512)
W16_OFFS = ((0, 0), (0, 4), (0, 2), (4, 0))  # (a_off, b_off) bytes off 256-B alignment


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import quant_gemm
    import quant_gemm._lib as L
    lib = ctypes.CDLL(args.lib) if args.lib else L.load()
    for name in ("qg_debug_config", "qg_moe_config", "qg_moe_batch_config", "qg_moe_glu_config", "qg_moe_down_config",
                 "qg_moe_prefill_config", "qg_group_config", "qg_w16_config", "qg_select_algo", "qg_set_group_affine", "qg_block_bytes"):
        if name == "qg_moe_down_config" and not hasattr(lib, name):
            continue  # --lib: a build from before the entry
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name]

    def line(entry, *a):
        buf = ctypes.create_string_buffer(256)
        rc = getattr(lib, entry)(*a, buf, 256)
        return f'{entry} {" ".join(map(str, a))} -> {rc} "{buf.value.decode()}"'

    for t in ROW_TYPES + KQ_TYPES:
        for k in (ROW_K if t in ROW_TYPES else KQ_K):
            for n in NS:
                for m in range(1, 9):
                    print(line("qg_debug_config", m, n, k, t, 0, 0), f"qg_select_algo={lib.qg_select_algo(m, n, k, t)}")
                for T, n_used, n_expert in MOE:
                    print(line("qg_moe_config", T, n_used, n, k, t))
                    print(line("qg_moe_glu_config", T, n_used, n, k, t))
                    if hasattr(lib, "qg_moe_down_config"):
                        print(line("qg_moe_down_config", T, n_used, n, k, t))
                    print(line("qg_moe_batch_config", T, n_used, n_expert, n, k, t))
                    print(line("qg_moe_prefill_config", T, n_used, n_expert, n, k, t))
    # grouped launches on addresses nothing dereferences: 2 and 8 equal items (an affine progression), one mixed-N group
    a, w, c = 1 << 40, 2 << 40, 3 << 40
    for mode in (0, 1, 2):
        lib.qg_set_group_affine(mode)
        for t in ROW_TYPES + KQ_TYPES:
            bb = lib.qg_block_bytes(t)
            for k in (ROW_K if t in ROW_TYPES else KQ_K):
                wbytes = lambda n: n * (k // 32) * bb
                groups = {f"{cnt}x4096": [(a, w + i * wbytes(4096), c + i * 4096 * 4, 4096, 0) for i in range(cnt)] for cnt in (2, 8)}
                groups["4096+11008"] = [(a, w, c, 4096, 0), (a, w + wbytes(4096), c + 4096 * 4, 11008, 0)]
                for tag, items in groups.items():
                    arr = (quant_gemm._GemvItem * len(items))(*[quant_gemm._GemvItem(*it) for it in items])
                    for m in (1, 2, 4):
                        buf = ctypes.create_string_buffer(256)
                        rc = lib.qg_group_config(arr, len(items), m, k, t, buf, 256)
                        print(f'qg_group_config affine={mode} {tag} {m} {k} {t} -> {rc} "{buf.value.decode()}"')
    lib.qg_set_group_affine(1)
    # W4A16 / W8A16: the operand offsets reach the alignment rules of the dispatch, ws_bytes a caller workspace (none, any)
    for t in W16_TYPES:
        for k in ROW_K:
            for n in NS:
                for m in W16_M:
                    for a_off, b_off in W16_OFFS:
                        for ws in (0, 1 << 40):
                            print(line("qg_w16_config", m, n, k, t, a_off, b_off, ws))


if __name__ == "__main__":
    main()
