"""quant_gemm._types, the package's one copy of the type ids and block geometry, against the built library's table
(csrc/qg_types.hpp through qg_block_bytes / qg_block_elems). CPU only: neither query touches a device."""


def test_python_table_matches_library():
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm._types as T
    import quant_gemm.ggml
    import quant_gemm.host

    lib = L.load()
    assert set(T.BLOCK_BYTES) == set(T.BLOCK_ELEMS) == {2, 3, 6, 7, 8, 9, 11, 12, 14, 23, 39}
    for t in T.BLOCK_BYTES:
        assert lib.qg_block_bytes(t) == T.BLOCK_BYTES[t], t
        assert lib.qg_block_elems(t) == T.BLOCK_ELEMS[t], t
    # ids the library has no block of: an unknown one, and the named non-block types
    for t in (99, 5, T.F32, T.F16, T.I32):
        assert lib.qg_block_bytes(t) == 0 and lib.qg_block_elems(t) == 0, t
    # the public names are the leaf module's objects
    assert quant_gemm.BLOCK_BYTES is T.BLOCK_BYTES and quant_gemm.host.BLOCK_BYTES is T.BLOCK_BYTES
    assert (quant_gemm.Q3_K, quant_gemm.Q4_K, quant_gemm.Q6_K, quant_gemm.IQ4_XS, quant_gemm.MXFP4) == (11, 12, 14, 23, 39)
    assert quant_gemm.ggml.Q4_K == T.Q4_K and quant_gemm.ggml.I32 == T.I32
