"""Which grouped GEMV launches are strided batches (csrc/qg_group_affine.hpp), on the host.

The header is pure host code (no HIP includes): tests/cpp/group_affine_host_test.cpp includes only it and is
built here with g++ -fsanitize=address,undefined. Covered: groups of 1, 2, 3 and 64 items with ascending,
descending and zero strides and shared activations; one item displaced by 4 bytes in A, in B or in C; unequal
N or ldc; strides below the batch form's alignment; pointer differences that do not fit intptr_t (between
neighbours and from the first to the last item); empty input.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llama.cpp-quant-gemm_amd", "csrc")


def test_header_has_no_hip_includes():
    src = open(os.path.join(CSRC, "qg_group_affine.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs and all("hip" not in i and "qg_" not in i for i in incs), incs


def test_affine_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "group_affine_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "group_affine_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_affine_host_test: ok" in r.stdout
