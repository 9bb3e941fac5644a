"""qg_gemm_w4a8_grouped_kq on the GPU: one launch of Q4_K / Q6_K items against the float64 contract (tests/kquant_ref.py,
tests/q6k_ref.py) and against the single call's bits.

Per item: |C - C64| <= 2 (K/32 + 2) 2^-24 mag (W = 0: the decode GEMV's lane-serial sum), the bits of qg.gemm_w4a8 on the
item, nothing written outside its columns, a relaunch identical. The grid M x K x pattern reaches every (T, MT, LPR, ONE)
of kq_group_kernel; rows (67, 16, 1) leave partial tiles and workgroups that exit early.
"""
import ctypes
import functools

import numpy as np
import pytest

import kquant_ref as KR
import q6k_ref as QR

pytestmark = pytest.mark.gpu

Q4_K, Q6_K = 12, 14
REF = {Q4_K: (KR, KR.random_q4k, 16), Q6_K: (QR, QR.random_q6k, 2)}  # reference module, weights, offset past 256 B
PATTERNS = {"q4k": [Q4_K] * 3, "q6k": [Q6_K] * 3, "mix3": [Q4_K, Q6_K, Q4_K], "mix2": [Q6_K, Q4_K]}
MS, KS, ROWS = (1, 2, 3, 8), (256, 512, 1024, 2304, 4096, 4352), (67, 16, 1)
SENT = -7.25


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@functools.lru_cache(maxsize=None)
def act(m, k, which):
    return KR.random_q8_1(np.random.default_rng([m, k, which]), m, k)


@functools.lru_cache(maxsize=None)
def weights(t, n, k):
    return REF[t][1](np.random.default_rng([t, n, k]), n, k)


@functools.lru_cache(maxsize=None)
def ref64(t, m, n, k, which):
    """(C64, mag) of weights(t, n, k) with activation tensor `which`: computed once, shared, never modified."""
    c64, _, mag = REF[t][0].gemm(act(m, k, which), weights(t, n, k))
    return c64, mag


def group(qg, types, m, k, rows=ROWS):
    """The device operands of a group: (A, B, out slice, wide buffer, column offset, N, type, activation index) per item.
    Items 0 and 1 share activation tensor 0, the others tensor 1; item i's weights are weights(t, n, k) rolled by i rows, so
    no two items of a type and N are alike."""
    import torch
    a_dev = [KR.dev_at(act(m, k, w), 4 * w) for w in (0, 1)]
    g = []
    for i, (t, n) in enumerate(zip(types, rows)):
        which = int(i >= 2)
        wide = torch.full((m, n + 9), SENT, dtype=torch.float32, device="cuda")
        b = KR.dev_at(np.roll(weights(t, n, k), i, axis=0), REF[t][2])
        assert b.data_ptr() % 256 == REF[t][2]
        g.append((a_dev[which], b, wide[:, 4:4 + n], wide, 4, n, t, which))
    return g


def launch(qg, g, m, k):
    qg.gemm_w4a8_grouped_kq([x[0] for x in g], [x[1] for x in g], [x[5] for x in g], [x[6] for x in g], m, k,
                            outs=[x[2] for x in g])


def line(qg, g, m, k):
    return qg.group_kq_config([(x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[5], x[3].stride(0), x[6]) for x in g], m, k)


def form(types, m, k):
    """What the config line must name: the type form, MT from M, (LPR, WGS, ONE) from K / 64 units."""
    ty = "mix" if len(set(types)) > 1 else {Q4_K: "q4k", Q6_K: "q6k"}[types[0]]
    u = k // 64
    lpr, wgs = (64, 1024) if u >= 64 else (16, 512) if u >= 16 else (4, 256)
    return f"gemvg:kq T={ty} MT={1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8} LPR={lpr} WGS={wgs} ONE={int(u <= lpr)} "


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_group_against_contract_and_single_call(qg, pattern, m, k):
    types = PATTERNS[pattern]
    g = group(qg, types, m, k)
    cfg = line(qg, g, m, k)
    assert cfg.startswith(form(types, m, k)) and f"x{len(types)} " in cfg, cfg
    launch(qg, g, m, k)
    first = [host(x[3]).copy() for x in g]
    for x in g:
        x[3].fill_(SENT)
    launch(qg, g, m, k)
    for i, ((a, b, _, wide, off, n, t, which), c1) in enumerate(zip(g, first)):
        w = host(wide)
        assert np.array_equal(bits(w), bits(c1))  # relaunch
        c = w[:, off:off + n]
        c64, mag = (np.roll(x, i, axis=1) for x in ref64(t, m, n, k, which))
        err, tol = np.abs(c.astype(np.float64) - c64), KR.tol(mag, k, 0)
        print(f"{cfg} item N={n} t={t}: max err/tol = {(err / tol).max():.3f}")
        assert (err <= tol).all()
        assert np.array_equal(bits(c), bits(host(qg.gemm_w4a8(a, b, m, n, k, t))))
        assert (w[:, :off] == SENT).all() and (w[:, off + n:] == SENT).all()


def test_grid_reaches_every_form(qg):
    """The config lines over the grid of the test above (no launch: stand-in addresses) name all 3 x 4 x 6 instantiations."""
    fake = lambda p: [(4096, 4096, 4096, n, 0, t) for n, t in zip(ROWS, PATTERNS[p])]
    seen = {" ".join(qg.group_kq_config(fake(p), m, k).split()[1:6]) for p in PATTERNS for m in MS for k in KS}
    want = {f"T={ty} MT={mt} LPR={lpr} WGS={wgs} ONE={one}" for ty in ("q4k", "q6k", "mix") for mt in (1, 2, 4, 8)
            for lpr, wgs in ((4, 256), (16, 512), (64, 1024)) for one in (1, 0)}
    assert len(want) == 72 and seen == want, sorted(seen ^ want)
    assert qg.group_kq_config(fake("mix3"), 3, 2304).split()[6] == "grid=3x3"  # 67 rows in tiles of 32, three items


def test_more_items_than_one_launch_holds(qg):
    """65 items, so two launches (64 + 1), types alternating with a run of three alike: each the bits of its single call."""
    m, k, n = 1, 256, 16
    types = [Q6_K if i % 3 == 0 else Q4_K for i in range(65)]
    g = group(qg, types, m, k, rows=[n] * 65)
    launch(qg, g, m, k)
    for a, b, c, wide, off, _, t, _ in g:
        assert np.array_equal(bits(host(c)), bits(host(qg.gemm_w4a8(a, b, m, n, k, t))))
        assert (host(wide)[:, :off] == SENT).all() and (host(wide)[:, off + n:] == SENT).all()


def test_captured_call_is_one_kernel_node(qg):
    """One captured call is one kernel node; replays after the activations were rewritten in place give the eager
    single calls' bits on the new activations. One stream, no parallel branch."""
    import torch
    m, k = 2, 1024
    g = group(qg, PATTERNS["mix3"], m, k)
    launch(qg, g, m, k)  # (warm: module load outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        launch(qg, g, m, k)
    hip, count = qg._lib.load(), ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(graph.raw_cuda_graph(), None, ctypes.byref(count)) == 0 and count.value == 1
    node, kind = ctypes.c_void_p(), ctypes.c_int(-1)
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    assert hip.hipGraphGetNodes(graph.raw_cuda_graph(), ctypes.byref(node), ctypes.byref(count)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0  # hipGraphNodeTypeKernel
    graph.instantiate()
    for seed in (5, 6, 7):
        for which in (0, 1):
            new = torch.from_numpy(KR.random_q8_1(np.random.default_rng([seed, which]), m, k)).cuda()
            next(x for x in g if x[7] == which)[0].copy_(new)
        for x in g:
            x[3].fill_(SENT)
        graph.replay()
        for a, b, c, _, _, n, t, _ in g:
            assert np.array_equal(bits(host(c)), bits(host(qg.gemm_w4a8(a, b, m, n, k, t))))
