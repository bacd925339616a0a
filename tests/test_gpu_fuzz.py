"""A bounded run of tools/fuzz_parity.py inside the GPU suite: random matrix families, row blocks, leading dimensions,
alpha / beta, kernel-selection switches and value / index types against the oracle (the tool's docstring has the
details; a failing case prints its parameters and `python tools/fuzz_parity.py --seed 3 --only K` replays it).
Its bar is np.allclose against the oracle's loop, at sizes up to 4000 rows; tests/test_gpu_fuzz_spmm.py
(tools/fuzz_spmm.py) holds the same kernels, on smaller matrices, through every entry point, order and switch, to the
numerics judges (exact grids, the rounding-error bound, IEEE classes) and ends in a census of the kernels it reached.
SpMM and SpMV only: the plans added since (transpose, COO, SpGEMM, SDDMM, softmax, attention, the solves, ILU(0),
colouring) have their randomised test in tests/test_gpu_fuzz_plans.py (tools/fuzz_plans.py), and the solvers on top of
them (PCG, BiCGStab, GMRES, with ILU(0) and AMG inside) in tests/test_gpu_fuzz_solvers.py (tools/fuzz_solvers.py)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_random_cases_match_the_oracle(sblas, oracle, cuda):
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    try:
        for case in range(120):
            assert fuzz.one_case(case, np.random.default_rng([3, case]), cuda, 4000), case
    finally:
        for k in fuzz.SWITCHES:
            os.environ.pop(k, None)
        sblas.reload_env()
