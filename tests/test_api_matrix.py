"""The C ABI's status codes and kernel choices, replayed against the recorded matrix (tools/api_matrix.py).

tests/golden/api_matrix.json holds what the library answered, case by case, when the matrix was recorded
(`tools/api_matrix.py --record`): the launch-free configuration queries over type x algo x sumi x M x N x K, and
every pointer-taking entry point with one defect at a time and with the defect pairs whose precedence matters
(negative size, bad K, weight type, empty, null, alignment -- the order include/qg/qg.h documents). The tree's
library must answer every case the same. CPU only: the library runs in a child process with no device
visible, and the child makes no fake-pointer call if it sees one all the same.
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "llama.cpp-quant-gemm_amd", "quant_gemm", "libqg_hip.so")


@pytest.fixture(scope="module")
def replay():
    spec = importlib.util.spec_from_file_location("api_matrix", os.path.join(REPO, "tools", "api_matrix.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    diffs, skipped, fixture = tool.check(LIB)  # one child process for both halves
    return diffs, skipped, fixture


def _report(diffs, half):
    bad = [d for d in diffs if d[0] == half]
    for _, case, want, got in bad[:30]:
        print(f"{case}: recorded {want}, now {got}")
    return len(bad)


def test_fixture_is_well_formed(replay):
    _, _, fixture = replay
    # only calls the library rejects or treats as empty were recorded: none reached a launch
    assert fixture["dropped_launching"] == 0
    assert fixture["dispatch_cases"] > 10000 and fixture["status_cases"] > 5000
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "api_matrix.json")) <= 64 * 1024


def test_dispatch_matrix(replay):
    """qg_debug_config, qg_debug_config_tiled, qg_debug_config_tiled_act, qg_select_algo and
    qg_gemm_w4a8_workspace_size: status and describe string of every recorded query."""
    diffs, _, _ = replay
    assert _report(diffs, "dispatch") == 0


def test_status_matrix(replay):
    """Every rejected or empty call returns the recorded code."""
    diffs, skipped, _ = replay
    if skipped:
        pytest.skip(skipped)
    assert _report(diffs, "status") == 0
