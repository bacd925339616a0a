"""bin/order_test: sblas_spmm_csr_v2 (method 2) on column-major B / C and on their row-major twins, twice each (the second
call planned); the row-major result must be the transposed column-major one bit for bit.  1, 2 and 4 logical GPUs on the
one device, N = 64 and 300 (at 300 the column-major side runs the column-tile pipeline, the row-major side the one-piece
merge), both merges, and once through the RCCL stand-in (the exchange branch of the row-major merge)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASH85, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "s-blas_amd", "bin", "order_test")


def _run(args, **env_extra):
    env = dict(os.environ, **env_extra)
    env.pop("SBLAS_SPMM_VARIANT", None)
    cp = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    out = cp.stdout + cp.stderr
    assert cp.returncode == 0, out[-3000:]
    assert "order_test: PASS" in cp.stdout and "bit-identical: yes" in cp.stdout, out[-3000:]
    return cp.stdout


@pytest.fixture(scope="module")
def synthetic_mtx(tmp_path_factory, sblas):
    """a banded matrix tall enough for several row panels per rank at four ranks"""
    from sblas_amd import synth
    rp, ci, v = synth.banded(6000, 24, 200)
    path = tmp_path_factory.mktemp("order") / "banded6000.mtx"
    rows = np.repeat(np.arange(6000), np.diff(rp)) + 1
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("6000 6000 %d\n" % len(ci))
        f.write("".join("%d %d %.17g\n" % (r, c + 1, x) for r, c, x in zip(rows, ci, v)))
    return str(path)


@pytest.mark.parametrize("merge", ["rowblocks", "allreduce"])
@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("gpus", [1, 2, 4])
def test_order_driver(sblas, cuda, synthetic_mtx, gpus, n, merge):
    extra = {"SBLAS_MERGE": "allreduce"} if merge == "allreduce" else {}
    for mtx in (ASH85, synthetic_mtx):
        _run([mtx, n, gpus], **extra)


def test_order_driver_through_the_rccl_stub(sblas, cuda, synthetic_mtx):
    import __graft_entry__
    stub = __graft_entry__.build_rccl_stub()
    for n in (64, 300):
        _run([synthetic_mtx, n, 4], SBLAS_RCCL_LIB=stub, SBLAS_COMM_FORCE_EXCHANGE="1")
