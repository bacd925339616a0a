"""bin/sddmm_test: sblas_sddmm_csr on ash85 in the four order combinations of X and Y against the host verifier, on 1 GPU
and on 2 logical GPUs folded onto the one device; every combination and both GPU counts must give the same bits."""
import os
import subprocess

import pytest

from conftest import ASH85, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "s-blas_amd", "bin", "sddmm_test")


@pytest.mark.parametrize("k", [64, 5])
@pytest.mark.parametrize("gpus", [1, 2])
def test_sddmm_driver(sblas, cuda, gpus, k):
    cp = subprocess.run([EXE, ASH85, str(gpus), str(k)], capture_output=True, text=True, timeout=600)
    out = cp.stdout + cp.stderr
    assert cp.returncode == 0, out[-3000:]
    assert "sddmm_test: PASS" in cp.stdout and "bit-identical: yes" in cp.stdout, out[-3000:]
    assert cp.stdout.count(": ok (max rel err") == 4, out[-3000:]
