"""bench.py's command line and its --dump-outputs writer (CPU only: nothing is timed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _parse(bench, monkeypatch, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(args))
    return bench.parse()


def test_plain_run_has_no_extra_legs(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(bench, monkeypatch, "--full", "--no-files", "--dump-outputs", "x")
    assert a.full and a.files is False and a.dump_outputs == "x"


@pytest.mark.parametrize("args", [("--files",), ("--c4",), ("--steps", "0"), ("--warmup", "-1")])
def test_rejected_arguments(bench, monkeypatch, args):
    with pytest.raises(SystemExit):
        _parse(bench, monkeypatch, *args)


def test_dump_outputs_dtypes(bench, tmp_path):
    pairs = np.zeros(5, dtype=[("i", "<u4"), ("j", "<u4")])
    pairs["i"], pairs["j"] = np.arange(5), np.arange(5) + 1
    ani = np.linspace(0.95, 1, 5).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"pairs_i": pairs["i"], "pairs_j": pairs["j"], "ani": ani})
    i, j, a = (np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("pairs_i", "pairs_j", "ani"))
    assert i.dtype == np.float64 and j.dtype == np.float64 and a.dtype == np.float32
    assert (i == pairs["i"]).all() and (j == pairs["j"]).all() and (a == ani).all()


def test_dump_outputs_samples_the_same_rows_past_the_cap(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4096 + 120)  # room for 10 rows of 8 + 4 bytes
    rows = np.arange(1000, dtype=np.uint32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"r": rows, "f": rows.astype(np.float32)})
    r, f = np.load(str(tmp_path / "a" / "r.npy")), np.load(str(tmp_path / "a" / "f.npy"))
    assert len(r) == 10 and (np.diff(r) > 0).all() and (r == f).all()
    assert (r == np.load(str(tmp_path / "b" / "r.npy"))).all()
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in ("r.npy", "f.npy")) <= 2 * 4096 + 120
