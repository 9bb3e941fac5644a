"""Grouped GEMV front end and the affine route (csrc/qg_gemv_kernel.hpp gemvg_kernel / gemv_launch,
csrc/qg_group_affine.hpp; qg.h at qg_set_group_affine).

Bar: every item's output equals its eager single qg_gemm_w4a8 launch bit for bit (torch.equal on the int32
view), through the explicit qg_gemm_w4a8_grouped and through a captured graph, in every mode of
qg_set_group_affine (0 off, 1 the measured classes, 2 every class), and qg_group_config names the kernel
family the case must take: "gemvb" (the strided batch's kernel) for an affine group of two or more items where
the mode's gate admits its class, "gemvg" (the grouped kernel) otherwise.

Shapes, the smallest that reach each path: K = 256 (4-lane rows), 4096 (one wave per row), 8192 (the unit
loop); N = 40 and 48 (ragged tile, half-filled two-tile workgroup) and 4096 (the grid's full width, XCD tile
order); M = 1, 2, 4; Q4_0, Q5_1, Q8_0; groups of 1, 2, 3, 8, 64 and 65 items. Layouts: ascending and descending
progressions, one weight matrix with per-item activations (zero weight stride), outputs as column slices of
one buffer (ldc > N), a progression with one item displaced (the general path), mixed N (early exit).
"""
import pytest

from test_gpu_capture_fuse import acts, bits_equal, captured, eager, gen_, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(autouse=True)
def _defaults(qg):
    qg.set_capture_fusion(1)
    qg.set_group_affine(1)
    yield
    qg.set_capture_fusion(1)
    qg.set_group_affine(1)


def gate(m, k, cnt):
    """group_affine_class_enabled (csrc/qg_gemv_kernel.hpp) in mode 1: the loop-free one-unit form (K <= 4096
    among this file's shapes) at M = 1, N <= 4096 (every shape here), 8 items or more."""
    return k <= 4096 and m == 1 and cnt >= 8


def build(torch, gen, t, m, k, ns, layout):
    """(activations, weights, outputs, affine) of one group; outputs NaN-filled views; `keep` owns the buffers."""
    cnt = len(ns)
    n = ns[0]
    same_n = all(x == n for x in ns)
    if not same_n:
        a = acts(torch, gen, m, k)
        ws = [weights(torch, gen, 1, x, k, t)[0] for x in ns]
        outs = [torch.full((m, x), float("nan"), dtype=torch.float32, device="cuda") for x in ns]
        return [a] * cnt, ws, outs, False
    pool = weights(torch, gen, cnt + 2, n, k, t)
    a1 = acts(torch, gen, m, k)
    out = torch.full((cnt, m, n), float("nan"), dtype=torch.float32, device="cuda")
    A, W, O, affine = [a1] * cnt, [pool[i] for i in range(cnt)], [out[i] for i in range(cnt)], True
    if layout == "desc":
        W, O = W[::-1], O[::-1]
    elif layout == "zero_b":
        am = torch.stack([acts(torch, gen, m, k) for _ in range(cnt)])
        A, W = [am[i] for i in range(cnt)], [pool[0]] * cnt
    elif layout == "cols":
        wide = torch.full((m, cnt * n + 5), float("nan"), dtype=torch.float32, device="cuda")
        O = [wide[:, i * n:(i + 1) * n] for i in range(cnt)]
    elif layout == "near":
        W[cnt // 2] = pool[cnt + 1]
        affine = cnt <= 2  # two items are always a progression
    else:
        assert layout == "asc"
    return A, W, O, affine


def check_case(torch, qg, t, m, k, ns, layout, seed):
    gen = gen_(torch, seed)
    A, W, O, affine = build(torch, gen, t, m, k, ns, layout)
    cnt = len(ns)
    ref = eager(torch, qg, lambda: [qg.gemm_w4a8(A[i], W[i], m, ns[i], k, t) for i in range(cnt)])
    items = [(A[i].data_ptr(), W[i].data_ptr(), O[i].data_ptr(), ns[i], O[i].stride(0) if m > 1 else ns[i])
             for i in range(cnt)]

    def clear():
        for o in O:
            o.fill_(float("nan"))

    def same():
        return all(bits_equal(torch, O[i], ref[i]) for i in range(cnt))

    def step():
        for i in range(cnt):
            qg.gemm_w4a8(A[i], W[i], m, ns[i], k, t, out=O[i])
    routes = {}
    for mode in (0, 1, 2):
        qg.set_group_affine(mode)
        # the first launch's route: items 0..63
        head = items[:64]
        want = "gemvb" if (mode and affine and len(head) >= 2 and (mode == 2 or gate(m, k, len(head)))) else "gemvg"
        routes[mode] = qg.group_config(items, m, k, t)
        assert routes[mode].split()[0] == want, (mode, routes[mode])
        clear()
        qg.gemm_w4a8_grouped(A, W, ns, m, k, t, outs=O)
        torch.cuda.synchronize()
        assert same(), ("grouped", mode, routes[mode])
        captured(torch, qg, step, replays=1, before_replay=clear)
        assert same(), ("captured", mode, routes[mode])
    return routes


COUNTS = [2, 3, 8, 64, 65]
LAYOUTS = ["asc", "desc", "zero_b", "cols", "near"]
SMALL = [(t, m, k, n) for t in (2, 7, 8) for m in (1, 2, 4) for k in (256, 4096) for n in (40, 48)]
CASES = [(t, m, k, n, COUNTS[i % 5], LAYOUTS[(i // 5 + i) % 5]) for i, (t, m, k, n) in enumerate(SMALL)]
# every layout at every count once more at the headline's class (Q4_0, M = 1, one wave per row), small N
CASES += [(2, 1, 4096, 48, c, lay) for c in COUNTS for lay in LAYOUTS if (2, 1, 4096, 48, c, lay) not in CASES]
# a single item; the unit loop (M = 1, and M = 2 through the explicit entry); the grid's full width
CASES += [(2, 1, 4096, 48, 1, "asc"), (8, 2, 256, 40, 1, "asc"),
          (2, 1, 8192, 48, 3, "asc"), (8, 1, 8192, 40, 2, "desc"), (7, 1, 8192, 48, 3, "near"), (2, 2, 8192, 48, 2, "asc"),
          (2, 1, 4096, 4096, 64, "asc"), (2, 1, 4096, 4096, 65, "desc"), (7, 2, 4096, 4096, 3, "desc"),
          (8, 4, 4096, 4096, 3, "near"), (2, 1, 8192, 4096, 2, "asc"), (2, 1, 256, 4096, 8, "zero_b"),
          (2, 4, 4096, 4096, 2, "cols")]


@pytest.mark.parametrize("t,m,k,n,cnt,layout", CASES)
def test_group_bits_and_route(torch_, qg, t, m, k, n, cnt, layout):
    check_case(torch_, qg, t, m, k, [n] * cnt, layout, 31 * t + 7 * m + k + n + cnt)


@pytest.mark.parametrize("t,m,k,ns", [(2, 1, 4096, [40, 48, 4096, 48]), (7, 2, 256, [200, 40]),
                                      (8, 4, 4096, [4096, 40, 48]), (2, 1, 8192, [48, 4096])])
def test_mixed_n_takes_the_grouped_kernel(torch_, qg, t, m, k, ns):
    """Items of different N: never affine; workgroups past a short item's rows exit (full = 0)."""
    routes = check_case(torch_, qg, t, m, k, ns, "asc", 5 + t + m + k)
    assert all(r.startswith("gemvg") and " full=0 " in r for r in routes.values()), routes


def test_route_names_the_batch_kernel_and_grid(torch_, qg):
    """The headline group: 64 products N = K = 4096 on consecutive weight copies, shared activations."""
    torch = torch_
    m, n, k, t, cnt = 1, 4096, 4096, 2, 64
    a, w, c = 1 << 40, 2 << 40, 3 << 40  # nothing is dereferenced by the query
    items = [(a, w + i * n * (k // 32) * 18, c + i * n * 4, n, 0) for i in range(cnt)]
    qg.set_group_affine(0)
    assert qg.group_config(items, m, k, t) == "gemvg F=2 MT=1 BPL=2 LPR=64 WGS=512 PRE=1 ONEU=1 TPW=2 full=1 grid=256x64"
    qg.set_group_affine(2)
    assert qg.group_config(items, m, k, t) == "gemvb F=2 MT=1 BPL=2 LPR=64 WGS=512 PRE=1 ONEU=1 TPW=1 grid=512x64"
    # the batch entry's own alignment rule: a weight stride that is no multiple of 16 bytes stays grouped
    odd = [(a, w + i * (n * (k // 32) * 18 + 4), c + i * n * 4, n, 0) for i in range(cnt)]
    assert qg.group_config(odd, m, k, t).startswith("gemvg")
    assert qg.group_config([], m, k, t) == "none"
    del torch


@pytest.mark.parametrize("calls,brk", [(8, 4), (12, 10)])
def test_capture_progression_breaks(torch_, qg, calls, brk):
    """Captured calls on consecutive weights, one of which (the fifth of 8; the eleventh of 12) uses a displaced
    matrix: the node is the strided form while the calls keep the progression (mode 2: from the second call;
    mode 1: from the eighth) and the grouped kernel from the break on; all calls still merge into ONE node (the
    counters' rule of tests/test_gpu_capture_fuse.py: calls - ceil(calls / 64) merged) and every output is exact."""
    torch = torch_
    m, n, k, t = 1, 48, 4096, 2
    gen = gen_(torch, 4242 + calls)
    a = acts(torch, gen, m, k)
    pool = weights(torch, gen, calls + 3, n, k, t)
    W = [pool[i] for i in range(calls)]
    W[brk] = pool[calls + 2]
    ref = eager(torch, qg, lambda: torch.stack([qg.gemm_w4a8(a, W[i], m, n, k, t) for i in range(calls)]))
    out = torch.full((calls, m, n), float("nan"), dtype=torch.float32, device="cuda")

    def step():
        for i in range(calls):
            qg.gemm_w4a8(a, W[i], m, n, k, t, out=out[i])
    for mode in (0, 1, 2):
        qg.set_group_affine(mode)
        merged, nodes = captured(torch, qg, step, replays=2, before_replay=lambda: out.fill_(float("nan")))
        assert (merged, nodes) == (calls - 1, 1), mode
        assert bits_equal(torch, out, ref), mode
    # and the prefix that keeps the progression is the strided form, the whole list is not
    qg.set_group_affine(2)
    it = [(a.data_ptr(), W[i].data_ptr(), out[i].data_ptr(), n, n) for i in range(calls)]
    assert qg.group_config(it[:brk], m, k, t).startswith("gemvb")
    assert qg.group_config(it[:brk + 1], m, k, t).startswith("gemvg")
    qg.set_group_affine(1)
    assert qg.group_config(it[:brk], m, k, t).startswith("gemvb" if brk >= 8 else "gemvg")
