"""bench.py's compact summary (the bench line's LAST key): built from every kind of row the
line carries, short enough to survive the driver's tail of stdout; and the --dump-outputs writer. CPU only (no GPU, no measurement)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_compact_summary_rows_and_size():
    import bench
    side = []
    for (w, m, n, k, forms) in [("q4_0", 32, 4096, 4096, ("single", "tiled", "tiled_act")), ("q4_1", 1, 4096, 4096, ("single",)),
                                ("q5_0", 1, 4096, 4096, ("single",)), ("q5_1", 1, 4096, 4096, ("single",)),
                                ("q4_0", 1, 32000, 4096, ("single", "batched")), ("q4_0", 1, 4096, 14336, ("single", "tiled")),
                                ("q4_0", 2, 4096, 14336, ("single", "tiled")), ("q4_0", 3, 4096, 14336, ("single", "tiled")),
                                ("q4_0", 4, 4096, 14336, ("single", "tiled")), ("q4_0", 512, 4096, 4096, ("single", "tiled", "tiled_act")),
                                ("q4_0", 32, 4096, 4128, ("prepacked", "padded", "tiled", "tiled_act"))]:
        for f in forms:
            side.append({"wtype": w, "M": m, "N": n, "K": k, "form": f,
                         ("us_per_gemv" if f == "batched" else "us_per_launch"): 12.345, "frac_hbm": 0.1234})
    out = {"roofline": {"us_per_launch": 3.25, "frac": 0.3639, "floor_us": 2.78, "floor": {"units_read_store_us": 3.13}},
           "batched": {"us_per_gemv": 1.385, "frac": 0.854}, "grouped": {"us_per_gemv": 1.505, "frac": 0.786},
           "cpu_baseline": {"ms_per_gemv": 8.95}, "cpu_baseline_mt": [{"cores": 16, "ms_per_gemv": 0.5}],
           "side_configs": side}
    sm = bench.compact_summary(out)
    assert len(sm["side"]) == len(side)
    assert "1x32000x4096:b=12.345" in sm["side"] and "q5_1:1x4096x4096:s=12.345" in sm["side"]
    assert sm["batched_us"] == 1.385 and sm["grouped_us"] == 1.505 and sm["cpu_16t_ms"] == 0.5
    # the driver keeps about 2 KB of the tail: the summary with its key must fit in well under that
    assert len(json.dumps({"summary": sm})) < 1400


def test_dump_outputs_full_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per array; an array over its share of the byte budget becomes the same
    sorted seeded sample of its flat elements on every call."""
    import numpy as np
    import torch

    import bench
    x = torch.arange(6000, dtype=torch.float32).reshape(6, 10, 100)
    y = torch.arange(50, dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path / "a"), {"x": x, "y": y}) == {"x": [6, 10, 100], "y": [50]}
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), x.numpy())
    assert np.load(tmp_path / "a" / "y.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 4 * 1000)  # 1000 elements per array
    for d in ("b", "c"):
        assert bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y}) == {"x": [1000], "y": [50]}
    xs = np.load(tmp_path / "b" / "x.npy")
    assert np.array_equal(xs, np.load(tmp_path / "c" / "x.npy"))
    assert xs.dtype == np.float32 and (np.diff(xs) > 0).all() and xs.max() < 6000
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 2 * 4 * 1000 + 2 * 128  # the .npy headers beside the budgeted data
