"""The type ids and block geometry (include/qg/qg.h, csrc/qg_types.hpp), once for the package and free of imports;
tests/test_types_cpu.py holds every entry to qg_block_bytes / qg_block_elems of the built library."""
# ggml_type ids (compat/ggml_types.h:199-215)
F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q8_1 = 0, 1, 2, 3, 6, 7, 8, 9
Q3_K = 11  # 256-element super-blocks of 110 bytes, 3-bit codes (qg.h "Q3_K weights")
Q4_K = 12  # 256-element super-blocks of 144 bytes (qg.h "Q4_K weights")
Q6_K = 14  # 256-element super-blocks of 210 bytes (qg.h "Q6_K weights")
IQ4_XS = 23  # 256-element super-blocks of 136 bytes, 4-bit codes into a table (qg.h "IQ4_XS weights")
I32 = 26  # the ids of mul_mat_id_from_ggml
MXFP4 = 39  # 32-element blocks of 17 bytes: an E8M0 scale byte and E2M1 codes (qg.h "MXFP4 weights")

BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34, Q8_1: 36, Q3_K: 110, Q4_K: 144, Q6_K: 210, IQ4_XS: 136, MXFP4: 17}
BLOCK_ELEMS = {t: 256 if t in (Q3_K, Q4_K, Q6_K, IQ4_XS) else 32 for t in BLOCK_BYTES}
