"""Hazard logic of the capture-time GEMV merge (csrc/qg_capture_fuse.hpp), on the host.

The header is pure host code (no HIP includes): tests/cpp/capture_fuse_host_test.cpp includes only it and is
built here with g++ -fsanitize=address,undefined. Covered: disjoint spans, each of the five overlap kinds
(new C over earlier A / B / C, new A / B over earlier C), touching-but-disjoint spans, span overflow
(= overlap), strided C with ldc > N, and the 64-item limit.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "llama.cpp-quant-gemm_amd", "csrc")


def test_header_has_no_hip_includes():
    src = open(os.path.join(CSRC, "qg_capture_fuse.hpp")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs and all("hip" not in i and "qg_" not in i for i in incs), incs


def test_hazard_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "capture_fuse_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "capture_fuse_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "capture_fuse_host_test: ok" in r.stdout
