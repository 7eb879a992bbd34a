"""CPU: bench.py's command line -- a plain run and --full, --dump-outputs -- and the helper that writes the outputs of the timed path
(the whole of C, or a fixed, seeded sample of its rows when C is larger than the limit).  No GPU involved."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_dump_outputs_writes_c_whole_or_a_seeded_sample_of_its_rows(tmp_path, monkeypatch):
    import torch
    import bench
    n_cols, rows = 4, 1000
    C = torch.arange(n_cols * rows, dtype=torch.float32)              # column-major: element (r, k) holds k * rows + r
    got = bench.dump_outputs(str(tmp_path / "whole"), C, n_cols)
    a = np.load(tmp_path / "whole" / "C.npy")
    assert a.dtype == np.float32 and a.shape == (n_cols, rows) and np.array_equal(a.ravel(), C.numpy())
    assert got["C"] == [n_cols, rows] and got["of_rows"] == rows

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * n_cols * 100)
    for sub in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / sub), C, n_cols)
        assert not (tmp_path / sub / "C.npy").exists()
    s1, s2 = np.load(tmp_path / "s1" / "C_sampled_rows.npy"), np.load(tmp_path / "s2" / "C_sampled_rows.npy")
    assert s1.dtype == np.float32 and s1.shape == (n_cols, 100) and s1.nbytes <= 4 * n_cols * 100
    assert np.array_equal(s1, s2)                                      # the same rows from run to run
    picked = s1[0].astype(np.int64)
    assert np.all(np.diff(picked) > 0) and np.array_equal(s1, a[:, picked])
