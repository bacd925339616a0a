"""The Krylov solvers' host rule (krylov_rule.cpp; no GPU): the pinned dot product restated in C++ against its
restatement in numpy (tests/krylov_numerics.py), the limits against krylov.h, and the launch count of one iteration."""
import os
import re

import numpy as np
import pytest

import krylov_numerics as KN
from conftest import ROOT


@pytest.mark.parametrize("kind", ["random", "mixed", "special"])
@pytest.mark.parametrize("n", KN.sizes())
def test_dot_ref_is_the_written_order(sblas, n, kind):
    x, y = KN.vectors(kind, n)
    got, want = sblas.krylov_dot_ref(x, y), KN.dot_np(x, y)
    assert KN.same_bits(got, want), (n, kind, got, want)
    if kind == "random":
        assert got == want                                                   # finite: plainly ==


def test_the_order_shows_in_the_mixed_vectors():
    """the mixed magnitudes are worth having: another order of the same products gives other bits"""
    x, y = KN.vectors("mixed", 3 * KN.CELL + 5)
    with np.errstate(all="ignore"):
        assert not KN.same_bits(KN.dot_np(x, y), np.sum(x * y)) or not KN.same_bits(KN.dot_np(x, y), np.cumsum(x * y)[-1])


def test_dot_ref_edges(sblas):
    assert KN.bits(sblas.krylov_dot_ref(np.zeros(0), np.zeros(0)))[0] == 0   # +0
    assert sblas.krylov_dot_ref([3.0], [-2.0]) == -6.0
    assert KN.bits(sblas.krylov_dot_ref([0.0], [-1.0]))[0] == 0              # +0 + -0 = +0
    with pytest.raises(sblas.SblasError):
        sblas.krylov_dot_ref(np.zeros(3), np.zeros(4))
    # Two roundings, not a fused multiply-add: lane 0 takes elements 0 and 256, and the second product cancels the first
    # sum exactly only if it is rounded before it is added (fused, the rounding error 2^-60 of a * a would be left).
    a = 1.0 + 2.0 ** -30
    x, y = np.zeros(KN.WIDTH + 1), np.zeros(KN.WIDTH + 1)
    x[[0, KN.WIDTH]], y[[0, KN.WIDTH]] = (1.0, a), (-(a * a), a)
    assert sblas.krylov_dot_ref(x, y) == 0.0 == KN.dot_np(x, y)
    x, y = np.zeros(KN.CELL + 1), np.zeros(KN.CELL + 1)                      # two cells: the second stage adds them
    x[[0, KN.CELL]], y[[0, KN.CELL]] = (3.0, 1.0), (0.5, -1.5)
    assert sblas.krylov_dot_ref(x, y) == 0.0


def test_limits_agree_with_the_header(sblas):
    text = open(os.path.join(ROOT, "s-blas_amd", "csrc", "krylov.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    lim = sblas.krylov_limits()
    assert lim == dict(cell=const("KRYLOV_CELL"), width=const("KRYLOV_LANES"), pcg_vectors=const("KRYLOV_PCG_VECTORS"),
                       bicgstab_vectors=const("KRYLOV_BICGSTAB_VECTORS"), max_dots=const("KRYLOV_MAX_DOTS"))
    assert (lim["cell"], lim["width"]) == (KN.CELL, KN.WIDTH)
    assert lim["cell"] % lim["width"] == 0


def test_launches_of_one_iteration(sblas):
    """counted by hand from the sequence DESIGN.md 3.22 lists, with the solves' launches as SptrsvPlan.info() gives them"""
    for lower, upper in ((1, 1), (3, 7), (63, 63), (0, 0)):
        apply = lower + upper                                                # one M^-1: the lower solve, then the upper
        pcg = ["spmv", "dot", "fold alpha", "x r update", "fold residual"] + ["solve"] * apply + ["dot", "fold beta", "p update"]
        assert sblas.krylov_launches("pcg", "ilu0", lower, upper) == len(pcg)
        bicg = ["p update"] + ["solve"] * apply + ["spmv", "dot", "fold alpha", "s update"] + ["solve"] * apply + \
               ["spmv", "dots", "fold omega", "x r update", "fold residual and beta"]
        assert sblas.krylov_launches("bicgstab", "ilu0", lower, upper) == len(bicg)
    for precond in (None, "jacobi"):                                         # the residual's fold is beta's; Jacobi rides in the updates
        assert sblas.krylov_launches("pcg", precond) == 6
        assert sblas.krylov_launches("pcg", precond, 5, 5) == 6              # read with ILU(0) only
        assert sblas.krylov_launches("bicgstab", precond) == 10
    L = sblas.lib()
    assert L.sblas_krylov_launches(2, 0, None, None) == -1
    assert L.sblas_krylov_launches(0, 3, None, None) == -1
    assert L.sblas_krylov_launches(0, 2, None, None) == -1                   # ILU(0) without the solves' info
    with pytest.raises(sblas.SblasError):
        sblas.krylov_launches("gmres")
    with pytest.raises(sblas.SblasError):
        sblas.krylov_launches("pcg", "ssor")
    for name in ("sblas_krylov_limits", "sblas_krylov_dot_ref", "sblas_krylov_launches", "sblas_hip_krylov_plan_create",
                 "sblas_hip_krylov_start", "sblas_hip_krylov_iterate", "sblas_hip_krylov_status", "sblas_hip_krylov_dot_f64"):
        assert name in sblas.EXPORTS


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    x = torch.zeros(8, dtype=torch.float64)
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(E, match="GPU tensor"):
        sblas.krylov_dot(x, x)
    with pytest.raises(E, match="GPU tensor"):
        sblas.KrylovPlan(8, rp, ci)
    with pytest.raises(E, match="method"):
        sblas.KrylovPlan(8, rp, ci, method="gmres")
    with pytest.raises(E, match="one to three"):
        sblas.krylov_dots([])
    with pytest.raises(E, match="op must be"):
        sblas.krylov_update("axpy", x, [x])
