"""The two ends of a panel in the LDS-tiled SpMM kernels: the prologue, which turns the panel's verdict, span and row
pointers into per-lane row state, and the write-back, which fetches every old value of C a thread needs in one batch
ahead of the barriers and writes the parked sums back on a fixed thread-to-(row, column) map.  Shapes are chosen for
what those two pieces can get wrong:
partial last panels, waves and groups of four rows that straddle the end of the matrix, empty rows at either end of a
panel, a second 64-column half of one column, beta = 0 on a C full of NaN, C at a row offset with ldc > rows, row-major
C, panels that fall back in the kernel, and the planned call.  Everything goes through the C ABI against the CPU oracle
at test_gpu_parity's tolerance, and every case asserts the panel census, so that a run that slipped to the direct
kernels cannot pass."""
import numpy as np
import pytest

from test_gpu_order import COL, ROW, same_bits
from test_gpu_parity import Dev, _env_switch, close

pytestmark = pytest.mark.gpu

SCALINGS = [(1.0, 0.0), (1.0, 1.0), (1.25, -0.5)]


@pytest.fixture(scope="module")
def env(sblas, oracle, cuda):
    import torch
    return sblas, oracle, torch, cuda


@pytest.fixture
def variant_env():
    yield from _env_switch("SBLAS_SPMM_VARIANT")


@pytest.fixture
def panel_rows_env():
    yield from _env_switch("SBLAS_SPMM_PANEL_ROWS")


@pytest.fixture
def density_env():
    yield from _env_switch("SBLAS_WINDOW_DENSITY")


def band(rows, per_row=40, half=100):
    """synth.banded rows over at least a full band of columns (a matrix of three rows still has rows of `per_row`)"""
    from sblas_amd import synth
    cols = max(rows, 2 * half + 1)
    return synth.banded(rows, per_row, half, cols=cols), cols


class Product:
    """One matrix on the device, one B, one C0; run() calls the library, want() the oracle (once per scaling)."""

    def __init__(self, env, rp, ci, v, cols, n, seed=0):
        self.sblas, self.oracle, self.torch, self.dev = env
        self.A = Dev(self.torch, self.dev, rp, ci, v, cols)
        self.rows, self.cols, self.n = self.A.rows, cols, n
        rng = np.random.default_rng(1000 * n + self.rows + seed)
        self.Bl = rng.standard_normal((cols, n))                       # logical cols x n
        self.Cl = rng.standard_normal((self.rows, n))                  # logical rows x n
        self.B = self.torch.from_numpy(self.Bl.T.reshape(-1).copy()).to(self.dev)   # column-major, ldb = cols
        nb = self.sblas.spmm_workspace_bytes(self.rows, cols, len(self.A.h[1]), n)
        self.ws = self.torch.empty(max(nb, 8) // 8, dtype=self.torch.float64, device=self.dev)
        self._want = {}

    def want(self, alpha, beta):
        key = (alpha, beta)
        if key not in self._want:
            c0 = self.Cl.T.reshape(-1).copy()                   # (a copy: the oracle works in place, and a one-row Cl.T is Cl)
            ref = self.oracle.spmm(self.rows, self.cols, self.n, *self.A.h, self.Bl.T.reshape(-1).copy(), c0, alpha, beta)
            self._want[key] = np.asarray(ref).reshape(self.n, self.rows).T.copy()
        return self._want[key]

    def run(self, alpha, beta, order_c=COL, pad=0, off=0, plan=None, c_fill=None):
        """-> (logical rows x n result, the census of the call, whether the rest of the C buffer kept its bits).
        C sits `off` rows into a buffer of rows + pad rows (ldc = rows + pad column-major, n + pad row-major)."""
        torch, S, rows, n = self.torch, self.sblas, self.rows, self.n
        Cl = self.Cl if c_fill is None else np.full((rows, n), c_fill)
        tall = rows + pad
        assert off <= pad
        if order_c == COL:
            ldc, c_offset = tall, off
            buf = np.full(n * ldc, -7.25e300)
            view = lambda b: b.reshape(n, ldc)[:, off:off + rows].T
            buf.reshape(n, ldc)[:, off:off + rows] = Cl.T
        else:
            ldc, c_offset = n + pad, off * (n + pad)
            buf = np.full(tall * ldc, -7.25e300)
            view = lambda b: b.reshape(tall, ldc)[off:off + rows, :n]
            buf.reshape(tall, ldc)[off:off + rows, :n] = Cl
        C = torch.from_numpy(buf.copy()).to(self.dev)
        A = self.A
        S.panel_census()
        if order_c == COL and plan is None:
            S.spmm(rows, self.cols, A.rowptr, A.colidx, A.val, self.B, self.cols, n, alpha, beta, C, ldc, self.ws, c_offset=c_offset)
        elif order_c == COL:
            plan.spmm(A.val, self.B, self.cols, n, alpha, beta, C, ldc, self.ws, c_offset=c_offset)
        elif plan is None:
            S.spmm_ordered(rows, self.cols, A.rowptr, A.colidx, A.val, self.B, self.cols, COL, n, alpha, beta, C, ldc, ROW,
                           self.ws, c_offset=c_offset)
        else:
            plan.spmm_ordered(A.val, self.B, self.cols, COL, n, alpha, beta, C, ldc, ROW, self.ws, c_offset=c_offset)
        torch.cuda.synchronize()
        census = S.panel_census()
        out = C.cpu().numpy()
        got = view(out).copy()
        mask = np.ones(out.shape, bool)
        view(mask)[...] = False
        return got, census, same_bits(out[mask], buf[mask])


def check(p, alpha, beta, fallback=0, **kw):
    got, census, rest = p.run(alpha, beta, **kw)
    ref = p.want(alpha, beta)
    assert census["windowed"] > 0 and census["fallback"] == fallback, census
    assert close(got, ref), (alpha, beta, kw, np.abs(got - ref).max())
    assert rest, "C was written outside the block"
    return got, census


@pytest.mark.parametrize("panel", ["default", "48,2"])
@pytest.mark.parametrize("rows", [1, 3, 5, 47, 95, 96, 97, 100, 191, 193])
def test_rows_partial_last_panel_idle_waves_straddling_groups(env, variant_env, panel_rows_env, density_env, panel, rows):
    """A last panel that is partial, waves without rows, a group of four rows that straddles the end (rows % 4 != 0).
    The classifier's density bar is set for a full-height panel, which a matrix of one to five rows cannot meet: the
    bar is lowered (the switch the density sweeps use) so that these shapes run the kernel under test."""
    variant_env("nomfma")
    density_env("0.001")
    if panel != "default":
        panel_rows_env(panel)
    (rp, ci, v), cols = band(rows)
    p = Product(env, rp, ci, v, cols, 64)
    check(p, 1.25, -0.5)
    check(p, 1.25, -0.5, order_c=ROW)


def test_empty_rows_at_both_ends_of_a_panel_and_an_empty_last_panel(env, variant_env, panel_rows_env, density_env):
    variant_env("nomfma")
    density_env("0.001")
    panel_rows_env("48,2")
    rows = 200                                                      # panels 0-3 full, panel 4 = rows 192-199
    (rp, ci, v), cols = band(rows)
    lens = np.diff(rp).astype(np.int64)
    keep = np.ones(rows, bool)
    keep[[0, 1, 2, 48, 49, 50, 51, 52, 92, 93, 94, 95, 143]] = False   # heads and tails of panels 0, 1, 2
    keep[192:] = False                                              # the last panel holds no nonzero at all
    sel = np.repeat(keep, lens)
    rp2 = np.zeros(rows + 1, np.int64)
    rp2[1:] = np.cumsum(np.where(keep, lens, 0))
    p = Product(env, rp2.astype(np.int32), ci[sel], v[sel], cols, 64)
    for oc in (COL, ROW):
        got, census = check(p, 1.25, -0.5, order_c=oc)
        assert census["windowed"] == 4, census                      # (the empty panel is the direct kernel's: beta * C)
        assert same_bits(got[192:], -0.5 * p.Cl[192:]) and same_bits(got[[0, 50, 95]], -0.5 * p.Cl[[0, 50, 95]])


@pytest.mark.parametrize("n", [64, 65, 127, 128, 130, 8, 24, 32])
def test_widths_second_half_of_one_column_padding_and_the_narrow_kernel(env, variant_env, n):
    """65: two 64-column halves of which the second holds one column; 127 / 130: padding up to the staged width;
    8 / 24 / 32: the narrow LDS-tiled kernel (which takes panels from 56 / 16 nonzeros per row on)."""
    variant_env("nomfma")
    (rp, ci, v), cols = band(197, per_row=70 if n < 64 else 40)
    p = Product(env, rp, ci, v, cols, n)
    for alpha, beta in SCALINGS:
        check(p, alpha, beta)
    check(p, 1.25, -0.5, order_c=ROW)


@pytest.mark.parametrize("order_c", [COL, ROW])
@pytest.mark.parametrize("n", [64, 130])
def test_scaling_and_beta_zero_never_reads_c(env, variant_env, n, order_c):
    variant_env("nomfma")
    (rp, ci, v), cols = band(300)
    p = Product(env, rp, ci, v, cols, n)
    for alpha, beta in SCALINGS:
        check(p, alpha, beta, order_c=order_c)
    got, census, rest = p.run(1.25, 0.0, order_c=order_c, c_fill=np.nan)       # C = NaN everywhere: none may come through
    assert census["windowed"] > 0 and census["fallback"] == 0, census
    assert np.isfinite(got).all() and close(got, p.want(1.25, 0.0)) and rest


@pytest.mark.parametrize("order_c", [COL, ROW])
@pytest.mark.parametrize("n", [64, 130])
def test_row_block_at_an_offset_into_a_taller_c(env, variant_env, n, order_c):
    """A method-2 row block: ldc > rows and C starts `off` rows into the buffer (off = 100 is not a multiple of 8 rows
    and 108 is: both alignments of a panel's 32-row runs); the rows above and below the block keep their bits."""
    variant_env("nomfma")
    (rp, ci, v), cols = band(250)
    p = Product(env, rp, ci, v, cols, n)
    for off in (100, 108):
        check(p, 1.0, 1.0, order_c=order_c, pad=150, off=off)
    check(p, 1.25, 0.0, order_c=order_c, pad=150, off=100)


@pytest.mark.parametrize("order_c", [COL, ROW])
@pytest.mark.parametrize("n", [64, 130])
def test_fallback_in_the_first_a_middle_and_the_last_panel(env, variant_env, panel_rows_env, n, order_c):
    """One shuffled row each in panels 0, 5 and 9 of ten: those three are recomputed by the in-kernel fallback (which now
    holds the old C values across its direct loop), the others are not."""
    variant_env("nomfma")
    panel_rows_env("48,2")
    rows = 480
    (rp, ci, v), cols = band(rows, per_row=60, half=150)
    ci, v = ci.copy(), v.copy()
    rng = np.random.default_rng(11)
    for r in (5, 263, 479):
        perm = rng.permutation(rp[r + 1] - rp[r])
        ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][perm]
        v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][perm]
    p = Product(env, rp, ci, v, cols, n)
    for alpha, beta in ((1.25, -0.5), (1.0, 0.0)):
        got, census = check(p, alpha, beta, fallback=3, order_c=order_c)
        assert census["windowed"] == 7, census


@pytest.mark.parametrize("order_c", [COL, ROW])
@pytest.mark.parametrize("n", [64, 130, 8])
def test_planned_call_gives_the_same_bits(env, variant_env, n, order_c):
    variant_env("nomfma")
    sblas = env[0]
    (rp, ci, v), cols = band(293, per_row=70 if n < 64 else 40)
    p = Product(env, rp, ci, v, cols, n)
    plan = sblas.SpmmPlan(p.rows, cols, p.A.rowptr, p.A.colidx, n)
    try:
        assert plan.info()["windowed"] > 0, plan.info()
        for alpha, beta in ((1.25, -0.5), (1.0, 0.0)):
            a, _ = check(p, alpha, beta, order_c=order_c)
            b, _ = check(p, alpha, beta, order_c=order_c, plan=plan)
            assert same_bits(a, b), (alpha, beta)
    finally:
        plan.destroy()
