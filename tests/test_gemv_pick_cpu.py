"""A pinned sample of the row GEMV's configuration strings (csrc/qg_gemv_kernel.hpp gemv_pick, described by
csrc/qg_gemv.hip), without a GPU: every line of tests/golden/gemv_pick_configs.txt is asked again and must come back
byte for byte. The lines are a subset of what tools/config_sweep.py prints (plus the forced-GEMV queries at M = 5, 8,
the M tile of 8); a retune of the dispatch therefore shows up as a reviewed diff of the fixture.

    python tests/test_gemv_pick_cpu.py [--lib PATH/libqg_hip.so] > tests/golden/gemv_pick_configs.txt

writes the fixture from a library (default: the one built next to the package)."""
import ctypes
import os
import sys

import pytest

ROW_TYPES = (2, 3, 6, 7, 8)  # Q4_0, Q4_1, Q5_0, Q5_1, Q8_0
MS = (1, 2, 3, 4, 5, 8)
KS = (64, 96, 1024, 2048, 4096, 8192, 9472, 14336)
NS = (40, 4096, 20000)
GROUP_MS, GROUP_KS = (1, 2, 4), (2048, 4096, 8192)
ALGO_AUTO, ALGO_GEMV = 0, 1
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_pick_configs.txt")
MAX_LINES = 400


def queries():
    """('debug', M, N, K, type, algo) and ('group', mode, tag, M, K, type): every (type, M, K) once under AUTO with N
    cycling through NS, the M tile of 8 forced to the GEMV at four K, and every (affine mode, group, M, K) with the type
    cycling through ROW_TYPES independently of the mode (so the three modes of one group are comparable)."""
    q = []
    for ti, t in enumerate(ROW_TYPES):
        for mi, m in enumerate(MS):
            for ki, k in enumerate(KS):
                q.append(("debug", m, NS[(ti + mi + ki) % 3], k, t, ALGO_AUTO))
    for t in ROW_TYPES:
        for m in (5, 8):
            for k in (96, 1024, 4096, 8192):
                q.append(("debug", m, 40, k, t, ALGO_GEMV))
    for mode in (0, 1, 2):
        for gi, tag in enumerate(("2x4096", "8x4096", "4096+11008")):
            for mi, m in enumerate(GROUP_MS):
                for ki, k in enumerate(GROUP_KS):
                    q.append(("group", mode, tag, m, k, ROW_TYPES[(gi + mi + ki) % 5]))
    q.append(("group", 1, "2x0", 1, 4096, 2))  # the empty-tile edge: every item has N = 0 (accepted, nothing to launch)
    return q


def group_items(lib, tag, k, t):
    """The sweep tool's groups, on addresses nothing dereferences: 2 / 8 equal items (an affine progression), one
    mixed-N group; '2x0': two items without rows."""
    a, w, c = 1 << 40, 2 << 40, 3 << 40
    wbytes = lambda n: n * (k // 32) * lib.qg_block_bytes(t)
    if tag == "4096+11008":
        return [(a, w, c, 4096, 0), (a, w + wbytes(4096), c + 4096 * 4, 11008, 0)]
    cnt, n = (int(x) for x in tag.split("x"))
    return [(a, w + i * wbytes(n), c + i * n * 4, n, 0) for i in range(cnt)]


def bind(lib):
    import quant_gemm._lib as L
    for name in ("qg_debug_config", "qg_group_config", "qg_select_algo", "qg_set_group_affine", "qg_block_bytes"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name]
    return lib


def answer(lib, q, sumi=0):
    import quant_gemm
    buf = ctypes.create_string_buffer(256)
    if q[0] == "debug":
        _, m, n, k, t, algo = q
        rc = lib.qg_debug_config(m, n, k, t, algo, sumi, buf, 256)
        return f'qg_debug_config {m} {n} {k} {t} {algo} -> {rc} "{buf.value.decode()}" qg_select_algo={lib.qg_select_algo(m, n, k, t)}'
    _, mode, tag, m, k, t = q
    items = group_items(lib, tag, k, t)
    arr = (quant_gemm._GemvItem * len(items))(*[quant_gemm._GemvItem(*it) for it in items])
    lib.qg_set_group_affine(mode)
    try:
        rc = lib.qg_group_config(arr, len(items), m, k, t, buf, 256)
    finally:
        lib.qg_set_group_affine(1)
    return f'qg_group_config affine={mode} {tag} {m} {k} {t} -> {rc} "{buf.value.decode()}"'


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return bind(L.load())


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as f:
        return f.read().splitlines()


def test_the_sample_covers_what_it_says(pinned):
    q = queries()
    assert len(q) == len(pinned) <= MAX_LINES
    dbg = [x for x in q if x[0] == "debug"]
    assert {x[4] for x in dbg} == set(ROW_TYPES) and {x[1] for x in dbg} == set(MS)
    assert {x[3] for x in dbg} == set(KS) and {x[2] for x in dbg} == set(NS)
    for t in ROW_TYPES:  # every type meets every M, every K and every N
        mine = [x for x in dbg if x[4] == t]
        assert {x[1] for x in mine} == set(MS) and {x[3] for x in mine} == set(KS) and {x[2] for x in mine} == set(NS)
    grp = [x for x in q if x[0] == "group"]
    assert {x[1] for x in grp} == {0, 1, 2} and {x[3] for x in grp} == set(GROUP_MS) and {x[4] for x in grp} >= set(GROUP_KS)
    assert {x[5] for x in grp} == set(ROW_TYPES)


def test_config_strings_are_the_pinned_ones(so, pinned):
    """Line by line; the parity hook (sumi = 1) must name the product's kernel, so it gives the same line."""
    for q, want in zip(queries(), pinned):
        assert answer(so, q) == want
        if q[0] == "debug":
            assert answer(so, q, sumi=1) == want


def test_the_sample_reaches_every_family_word(pinned):
    """The three formats of the describe consumer and the three argument signatures of the single call are all in the
    sample (or the comparison above would pin less than it claims)."""
    text = "\n".join(pinned)
    for word in ('"gemv F=', '"gemvb F=', '"gemvg F=', "SIG=m1 ", "SIG=short ", "full=0", "full=1", '"none"'):
        assert word in text, word


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd"))
    import quant_gemm._lib as L
    path = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
    lib = bind(ctypes.CDLL(path) if path else L.load())
    for q in queries():
        line = answer(lib, q)
        assert q[0] != "debug" or answer(lib, q, sumi=1) == line, line
        print(line)
