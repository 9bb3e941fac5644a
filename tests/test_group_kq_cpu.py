"""qg_gemm_w4a8_grouped_kq without a GPU: validation codes and their order on fake pointers, the routes of the config line."""
import ctypes

import pytest

Q4_K, Q6_K = 12, 14
FAKE = 4096  # never dereferenced: every call here is refused, empty or a config query


class Item(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("N", ctypes.c_int),
                ("ldc", ctypes.c_int), ("wtype", ctypes.c_int), ("reserved", ctypes.c_int)]


def item(A=FAKE, B=FAKE, C=FAKE, N=8, ldc=0, t=Q4_K, reserved=0):
    return Item(A, B, C, N, ldc, t, reserved)


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def run(so, items, M=1, K=256, count=None):
    arr = (Item * max(len(items), 1))(*items)
    return so.qg_gemm_w4a8_grouped_kq(arr, len(items) if count is None else count, M, K, None)


def config(so, items, M, K):
    arr, buf = (Item * max(len(items), 1))(*items), ctypes.create_string_buffer(256)
    rc = so.qg_group_kq_config(arr, len(items), M, K, buf, 256)
    return rc, buf.value.decode()


def test_validation_codes_and_their_order(so):
    ok = item()
    # sizes first: before K, the type and the pointers
    for bad in (dict(count=-1), dict(M=-1)):
        assert run(so, [item(t=2, A=None)], **{"K": 33, **bad}) == -1
    for kw in (dict(N=-1), dict(ldc=-1), dict(N=8, ldc=7), dict(reserved=1)):
        assert run(so, [ok, item(t=2, A=None, **kw)], K=33) == -1, kw
    assert so.qg_gemm_w4a8_grouped_kq(None, 1, 1, 256, None) == -1
    # K: a positive multiple of 256, before the type
    for k in (0, -256, 32, 288, 4128):
        assert run(so, [item(t=2, A=None)], K=k) == -2, k
    # the type of any one item, wherever it sits and even where it is empty; before the empty call and the pointers
    for t in (11, 23, 39, 2, 99):
        for pos in range(3):
            items = [item(A=None), item(t=Q6_K, B=FAKE + 1), item(N=0)]
            items[pos].wtype = t
            assert run(so, items) == -3 and run(so, items, M=0) == -3, (t, pos)
    # empty: nothing touched, whatever the pointers are
    assert run(so, []) == 0 and so.qg_gemm_w4a8_grouped_kq(None, 0, 1, 256, None) == 0
    assert run(so, [item(A=None, B=1, C=2)], M=0) == 0 and run(so, [item(A=None, B=1, N=0), item(C=None, N=0, t=Q6_K)]) == 0
    # null before alignment, over all items
    for kw in (dict(A=None), dict(B=None), dict(C=None)):
        assert run(so, [item(B=FAKE + 8), item(t=Q6_K, **kw)]) == -1, kw
    # alignment: A and C 4 B, B by the item's own type (Q4_K 16 B, Q6_K 2 B)
    for kw in (dict(A=FAKE + 2), dict(C=FAKE + 2), dict(B=FAKE + 8), dict(B=FAKE + 4), dict(B=FAKE + 1, t=Q6_K)):
        assert run(so, [ok, item(**kw)]) == -4, kw
    rc, s = config(so, [item(B=FAKE + 16), item(B=FAKE + 2, t=Q6_K), item(B=FAKE + 1, t=Q6_K, N=0)], 1, 256)
    assert rc == 0 and s.startswith("gemvg:kq T=mix "), s


def test_routes_of_the_config_line(so):
    q4, q6 = item(N=67), item(N=16, t=Q6_K)
    assert config(so, [q4, q6], 8, 4096) == (0, "gemvg:kq T=mix MT=8 LPR=64 WGS=1024 ONE=1 grid=5x2 lds=43008")
    assert config(so, [q6, q6], 3, 768) == (0, "gemvg:kq T=q6k MT=4 LPR=4 WGS=256 ONE=0 grid=1x2 lds=2736")
    assert config(so, [q4], 1, 1024)[1].startswith("gemvg:kq T=q4k MT=1 LPR=16 WGS=512 ONE=1 grid=3x1 ")
    # one by one: M beyond the decode GEMV, and records of the largest type present beyond 160 KiB
    assert config(so, [q4, q6], 9, 256)[1].startswith("items: ")
    k4, k6 = 160 * 1024 // 336 * 256, 160 * 1024 // 304 * 256  # the last K whose records of one row fit: Q4_K's, Q6_K's
    assert k4 < k6 and config(so, [q4, q6], 1, k4)[1].startswith("gemvg:kq T=mix ")
    assert config(so, [q4, q6], 1, k4 + 256)[1].startswith("items: ") and config(so, [q4, q6], 2, k4)[1].startswith("items: ")
    assert config(so, [q6, q6], 1, k6)[1].startswith("gemvg:kq T=q6k ") and config(so, [q6], 1, k6 + 256)[1].startswith("items: ")
    # an empty Q4_K item does not size the records
    assert config(so, [item(N=0), q6], 1, k6)[1].startswith("gemvg:kq T=q6k ")
    # nothing to launch
    for items, m in (([], 1), ([q4], 0), ([item(N=0), item(N=0, t=Q6_K)], 4)):
        assert config(so, items, m, 256) == (0, "none")
    assert config(so, [item(t=2)], 1, 256)[0] == -3 and so.qg_group_kq_config(None, 0, 1, 256, None, 0) == -1
