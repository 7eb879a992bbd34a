"""bench.py on one MI355X (-m gpu): a plain run times exactly --steps steps, prints the headline line without the --full extras, and
--dump-outputs writes the C its last timed step computed -- checked element by element against the oracle's VBR::multiply of the same
seeded workload (cant-like 62 451^2, Keeper tau 0.6, 32 x 32 blocks, N = 128, fp32, B seeded as bench.py seeds it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sparta_amd as sa
from oracle import oracle as O
import _util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_product(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["metric"] == "Block-sparse SpMM GFLOP/s" and out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 7 and out["warmup"] == 2 and out["ms_per_step"] > 0.0 and out["value"] > 0.0
    assert out["roofline"] is None and out["cpu_baseline"] is None and "suite" not in out["config"]

    w, n = 32, 128
    m = sa.gen.cant_like(seed=2)
    g = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1).GetGrouping(m)
    v = sa.VBR().fill_from_CSR_inplace(m, g, w, 32, True)
    C = np.load(tmp_path / "C.npy")
    assert C.dtype == np.float32 and C.shape == (n, v.rows)
    assert out["config"]["dumped_outputs"]["C"] == [n, v.rows]
    Bh = (torch.rand(v.cols * n, generator=torch.Generator(device="cpu").manual_seed(1234), dtype=torch.float32) - 0.5).numpy()
    Co = O.vbr_multiply(v.rows, v.cols, w, v.row_part, v.nzcount, v.jab, v.mab, Bh, n)
    bound = U.abs_bound(v.rows, v.cols, w, v.row_part, v.nzcount, v.jab, v.mab, Bh, n)
    err = np.abs(C.ravel() - Co)
    assert np.all(err <= 1e-5 * bound + 1e-30), float((err / (bound + 1e-30)).max())
