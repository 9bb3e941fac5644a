"""A pinned sample of the W4A16 / W8A16 dispatch's configuration strings (csrc/qg_w4a16.hip: the candidates, W16Pick,
w16_run), without a GPU: every line of tests/golden/w16_pick_configs.txt is asked again and must come back byte for
byte. The lines are a subset of what tools/config_sweep.py prints for qg_w16_config; a retune of the dispatch therefore
shows up as a reviewed diff of the fixture. The fixture was written from the library BEFORE the dispatch became one
pick and one consumer (profiles/w16_pick/README.md), so it also holds that refactor to the choices it found.

    python tests/test_w16_pick_cpu.py [--lib PATH/libqg_hip.so] > tests/golden/w16_pick_configs.txt

writes the fixture from a library (default: the one built next to the package)."""
import ctypes
import os
import re
import sys

import pytest

TYPES = (2, 8)  # Q4_0 (W4A16), Q8_0 (W8A16)
MS = (1, 2, 4, 8, 9, 17, 32, 40, 64, 100)
KS = (96, 256, 512, 1024, 2048, 4096, 8192, 14336)
NS = (40, 4096, 8200)
WS = (0, 1 << 40)  # no workspace can be had; a caller's workspace of any size
# off 256-B alignment: weights 4-B / 2-B aligned only, activations 4-B aligned only
OFFS = ((0, 4), (0, 2), (4, 0))
OFF_SHAPES = ((1, 40, 4096), (4, 4096, 1024), (17, 64, 256), (32, 4096, 4096), (40, 40, 2048), (100, 4096, 512))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w16_pick_configs.txt")
MAX_LINES = 400
FAMILIES = ("w16d", "w16s", "w16sk", "w16mfma", "w16gemv", "w16gemv1r", "w16generic")
# the fields of each family that take two values, and the values the sample must show
TWO_VALUED = {
    "w16d": {"F": {2, 8}, "RT": {1, 2}, "W": {12, 16}, "NP": {2, 3}, "SB": {2, 4}},
    "w16s": {"F": {2, 8}, "TT": {1, 2}, "NP": {2, 3}},
    "w16sk": {"F": {2, 8}, "RT": {4, 8}, "TT": {2, 4}, "NP": {2, 3}},
    "w16mfma": {"F": {2, 8}, "RT": {1, 2}},
    "w16gemv": {"F": {2, 8}, "BPL": {2, 4}, "ONEU": {0, 1}, "SIG": {"m1", "full"}},
    "w16generic": {"F": {2, 8}},
}


def queries():
    """(M, N, K, type, a_off, b_off, ws_bytes): every (type, M, K) on aligned operands with N cycling through NS, then
    the offsets on a few shapes; each with and without a workspace."""
    q = []
    for ti, t in enumerate(TYPES):
        for mi, m in enumerate(MS):
            for ki, k in enumerate(KS):
                q += [(m, NS[(ti + mi + ki) % 3], k, t, 0, 0, ws) for ws in WS]
    for t in TYPES:
        for a_off, b_off in OFFS:
            for m, n, k in OFF_SHAPES:
                q += [(m, n, k, t, a_off, b_off, ws) for ws in WS]
    return q


def bind(lib):
    import quant_gemm._lib as L
    for name in ("qg_w16_config", "qg_gemm_w16_workspace_size"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = L.SIGNATURES[name]
    return lib


def config(lib, m, n, k, t=2, a_off=0, b_off=0, ws=0):
    buf = ctypes.create_string_buffer(256)
    rc = lib.qg_w16_config(m, n, k, t, a_off, b_off, ws, buf, 256)
    return rc, buf.value.decode()


def fields(text):
    """'w16s F=2 ... grid=16x3x4 ...' -> {'family': 'w16s', 'F': 2, ..., 'grid': '16x3x4', 'SIG': 'm1'}"""
    words = text.split()
    out = {"family": words[0] if words else ""}
    for w in words[1:]:
        name, v = w.split("=")
        out[name] = int(v) if re.fullmatch(r"-?\d+", v) else v
    return out


def answer(lib, q):
    rc, text = config(lib, *q)
    return f'qg_w16_config {" ".join(map(str, q))} -> {rc} "{text}"'


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return bind(L.load())


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as f:
        return f.read().splitlines()


def test_config_strings_are_the_pinned_ones(so, pinned):
    q = queries()
    assert len(q) == len(pinned) <= MAX_LINES
    for one, want in zip(q, pinned):
        assert answer(so, one) == want


def test_the_sample_reaches_every_family_and_both_values_of_every_field(pinned):
    seen = {}
    for line in pinned:
        f = fields(line.split('"')[1])
        for name, v in f.items():
            seen.setdefault(f["family"], {}).setdefault(name, set()).add(v)
    assert set(seen) == set(FAMILIES)
    for family, want in TWO_VALUED.items():
        for name, values in want.items():
            assert seen[family][name] == values, (family, name)
    assert seen["w16gemv"]["MT"] == {1, 2, 4, 8}
    for family in ("w16s", "w16sk"):  # one slice (no workspace needed) and several
        assert 1 in seen[family]["ks"] and max(seen[family]["ks"]) > 1 and 0 in seen[family]["ws"]


def test_workspace_size_covers_every_reachable_need(so):
    """qg_gemm_w16_workspace_size(M, N, K) is one figure for both types and any alignment: at least the ws= of whatever
    the shape runs, with and without a workspace."""
    needs = 0
    for m, n, k, t, a_off, b_off, ws in queries():
        f = fields(config(so, m, n, k, t, a_off, b_off, ws)[1])
        if "ws" in f:
            needs += f["ws"] > 0
            assert so.qg_gemm_w16_workspace_size(m, n, k) >= f["ws"], (m, n, k, t, a_off, b_off, ws)
            assert ws or f["ws"] == 0  # nothing that needs a workspace is picked without one
    assert needs > 20


def test_query_conventions(so):
    """qg_debug_config's: no buffer is an argument error, an empty call is QG_OK and names nothing, the entry's own
    refusals come back with an empty line."""
    assert so.qg_w16_config(1, 8, 256, 2, 0, 0, 0, None, 0) == -1
    assert config(so, 0, 8, 256) == (0, "") and config(so, 4, 0, 256) == (0, "")
    assert config(so, -1, 8, 256) == (-1, "")
    rc, text = config(so, 4, 8, 48)
    assert rc != 0 and text == ""  # K % 32
    rc, text = config(so, 4, 8, 256, a_off=2)
    assert rc != 0 and text == ""  # activations below 4-B alignment


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd"))
    import quant_gemm._lib as L
    path = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
    lib = bind(ctypes.CDLL(path) if path else L.load())
    for one in queries():
        print(answer(lib, one))
