"""bench.py as a process on the GPU: a plain run measures the headline alone
and --dump-outputs writes the y of its last timed MatMult."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, spmv_tolerance
from oracle import seqaij


@pytest.mark.gpu
def test_plain_run_line_and_dumped_output(pkg, tmp_path):
    """One plain run at 24^3: exactly one JSON line with the contract's
    fields, --steps timed steps, no leg beside the headline; y.npy is the
    oracle's MatMult of the same operand and x within SURVEY §8d's
    componentwise bound (conftest.spmv_tolerance)."""
    N, K, W = 24, 3, 1
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--grid", str(N), "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip() == lines[0]
    d = json.loads(lines[0])
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["metric"].startswith("CSR SpMV effective HBM GB/s")
    assert d["steps"] == K and d["warmup"] == W and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["roofline"]["launches_timed"] == K
    assert abs(d["value"] - d["config"]["bytes_per_spmv"] / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * d["value"]
    for leg in ("effective", "cg", "cg_gamg", "host_vec", "read_ceiling", "flan_standin", "cpu_baseline",
                "cpu_baseline_all_cores", "result_stable"):
        assert leg not in d, leg
    assert d["budget"]["legs"] == {}
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == ["y.npy"]
    y = np.load(tmp_path / "o" / "y.npy")
    assert y.dtype == np.float64 and y.shape == (N ** 3,)
    ai, aj, aa, _, _ = seqaij.create_system(N, N, N)
    x = pkg.splitmix_uniform(N ** 3, 42)
    ref = seqaij.matmult(ai, aj, aa, x)
    tol, _ = spmv_tolerance(ai, aj, aa, x)
    assert np.all(np.abs(y - ref) <= tol)
