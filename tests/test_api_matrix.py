"""The C ABI's status codes and kernel choices, replayed against the recorded matrix (tools/api_matrix.py).

tests/golden/api_matrix.json holds what the library answered, case by case, when the matrix was recorded
(`tools/api_matrix.py --record`): the launch-free configuration queries over type x algo x sumi x M x N x K, and
every pointer-taking entry point with one defect at a time and with the defect pairs whose precedence matters
(negative size, bad K, weight type, empty, null, alignment -- the order include/qg/qg.h documents). The tree's
library must answer every case the same. tests/golden/api_matrix_types.json is the second fixture of the same tool:
Q3_K, Q6_K, IQ4_XS and MXFP4 through the same queries and entries, the mul_mat_id entries with their defects and
qg_moe*_config, and every weight id against every entry that takes one. CPU only: the library runs in a child process with no device
visible, and the child makes no fake-pointer call if it sees one all the same.
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "llama.cpp-quant-gemm_amd", "quant_gemm", "libqg_hip.so")


def _replay(which):
    spec = importlib.util.spec_from_file_location("api_matrix", os.path.join(REPO, "tools", "api_matrix.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    diffs, skipped, fixture = tool.check(LIB, which)  # one child process for both halves
    fixture["path"] = tool.GOLDENS[which]
    return diffs, skipped, fixture


@pytest.fixture(scope="module")
def replay():
    return _replay("base")


@pytest.fixture(scope="module")
def replay_types():
    return _replay("types")


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
    assert os.path.getsize(fixture["path"]) <= 64 * 1024


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


# ---- the second fixture (tests/golden/api_matrix_types.json): the same three assertions ---------------------------
def test_types_fixture_is_well_formed(replay_types):
    test_fixture_is_well_formed(replay_types)


def test_types_dispatch_matrix(replay_types):
    """qg_debug_config* and qg_select_algo of Q3_K, Q6_K, IQ4_XS and MXFP4 (M = 6 | 7 and 8 | 9 among the shapes), and every
    qg_moe*_config over every named weight id."""
    test_dispatch_matrix(replay_types)


def test_types_status_matrix(replay_types):
    """The same entries around a call of each of those types, the ten mul_mat_id entries (one defect at a time and in
    pairs), and every named weight id against every entry with a type argument: taken or refused, and at which granule."""
    test_status_matrix(replay_types)
