"""bin/coo_test: ash85 read as COO, mirrored, shuffled with a fixed seed and converted on the device through
CsrSparseMatrix(coo, dup) in both duplicate modes; the CSR must equal CsrSparseMatrix(file) bit for bit and
sblas_spmv_csr_v1 must give equal results on all three.  1 GPU and 2 logical GPUs folded onto the one device."""
import os
import subprocess

import pytest

from conftest import ASH85, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "s-blas_amd", "bin", "coo_test")


@pytest.mark.parametrize("gpus", [1, 2])
def test_coo_driver(sblas, cuda, gpus):
    cp = subprocess.run([EXE, ASH85, str(gpus)], capture_output=True, text=True, timeout=600)
    out = cp.stdout + cp.stderr
    assert cp.returncode == 0, out[-3000:]
    assert "coo_test: PASS" in cp.stdout, out[-3000:]
    assert cp.stdout.count("bit-identical") == 2 and "spmv on %d GPU(s): equal" % gpus in cp.stdout, out[-3000:]
