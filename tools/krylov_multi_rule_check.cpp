// krylov_multi_rule_check.cpp -- a stand-alone program over the multi-right-hand-side Krylov solvers' host rule
// (s-blas_amd/csrc/krylov_multi_rule.cpp; no GPU, no HIP runtime) and the scalar step both solvers' device folds run
// (s-blas_amd/csrc/krylov_scalar.h, compiled for the host by that file), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/krylov_multi_rule_check.cpp s-blas_amd/csrc/krylov_multi_rule.cpp -o /tmp/krylov_multi_rule_check && /tmp/krylov_multi_rule_check
// It takes the limits, the kinds a batch accepts, the launch counts and the grid of every width from 1 to 64 at the edge
// sizes, asks the overlap predicate both multi-right-hand-side plans refuse "X overlaps B" by (krylov_multi.h, through
// multi_plan.h) a table of exact cases, and drives whole PCG and BiCGStab recurrences of scalar steps on blocks of exactly 16 slots and sums of exactly
// nd entries (so a read or write past either end is the sanitizer's to find), against a second restatement of the
// written order, with a zero, an infinity and a NaN put into every denominator.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/sblas_hip.h"
#include "../s-blas_amd/csrc/krylov_multi.h" // span_bytes, blocks_overlap: no HIP in there

#pragma clang fp contract(off)

static uint64_t state = 88172645463325252ull;
static double rnd()
{
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(int64_t)(state >> 11) / 9007199254740992.0 + 0.25; // (0.25, 1.25)
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (isnan(a) && isnan(b)); }

// the block's slots (krylov.h's KrylovSlot, restated on purpose)
enum { STATUS = 0, ITER = 1, RNORM = 2, BNORM = 3, ALPHA = 4, BETA = 5, OMEGA = 6, WHICH = 7, RHO = 8, TOL = 9, MAX_ITER = 10, ZERO_X = 11 };

struct Block {
    std::vector<double> v = std::vector<double>(16, -7.0); // exactly the contract's size, on the heap
    double &f(int k) { return v[(size_t)k]; }
    int64_t i(int k) const
    {
        int64_t x;
        memcpy(&x, &v[(size_t)k], 8);
        return x;
    }
};

static int step(int op, int flag, std::vector<double> d, Block &b, double rtol = 0.0, double atol = 0.0, int64_t max_iter = 0)
{
    return sblas_krylov_scalar_step_ref(op, (int)d.size(), flag, d.data(), b.v.data(), rtol, atol, max_iter);
}

// the written order once more: one column's scalars as plain variables
struct Restated {
    int64_t status = 0, iter = 0, which = 0, max_iter = 0;
    double rnorm = 0, bnorm = 0, alpha = 0, beta = 0, omega = 0, rho = 0, tol = 0;
    static bool bad(double d) { return d == 0.0 || !isfinite(d); }
    void begin(double bb, bool bicg, double rtol, double atol, int64_t limit)
    {
        bnorm = sqrt(bb);
        const double t = rtol * bnorm;
        tol = t >= atol ? t : atol, omega = bicg ? 1.0 : 0.0, max_iter = limit;
        status = bb == 0.0 ? SBLAS_KRYLOV_CONVERGED : SBLAS_KRYLOV_RUNNING;
    }
    bool residual(double rr, bool count)
    {
        rnorm = sqrt(rr);
        if (count) ++iter;
        if (rnorm <= tol) status = SBLAS_KRYLOV_CONVERGED;
        else if (iter >= max_iter) status = SBLAS_KRYLOV_LIMIT;
        else return true;
        return false;
    }
    void down(int64_t w) { status = SBLAS_KRYLOV_BREAKDOWN, which = w; }
};

static int agree(Block &b, const Restated &r, const char *where)
{
    const bool ok = b.i(STATUS) == r.status && b.i(ITER) == r.iter && b.i(WHICH) == r.which && same(b.f(RNORM), r.rnorm) &&
                    same(b.f(BNORM), r.bnorm) && same(b.f(ALPHA), r.alpha) && same(b.f(BETA), r.beta) && same(b.f(OMEGA), r.omega) &&
                    same(b.f(RHO), r.rho) && same(b.f(TOL), r.tol);
    if (!ok) printf("the step and its restatement part at %s\n", where);
    return ok ? 0 : 1;
}

// a PCG recurrence of scalar steps; `poison` replaces the denominator of step `at` (-1: none)
static int pcg_run(int at, double poison, bool two_dots)
{
    int bad = 0;
    Block b;
    Restated r;
    const double bb = 4.0 * rnd();
    bad += step(SBLAS_KRYLOV_STEP_START_B, 0, {bb}, b, 1e-3, 0.0, 40) != SBLAS_OK;
    r.begin(bb, false, 1e-3, 0.0, 40);
    double rr = bb, rz = two_dots ? bb * rnd() : bb;
    bad += step(SBLAS_KRYLOV_STEP_START_R, 0, two_dots ? std::vector<double>{rr, rz} : std::vector<double>{rr}, b) != SBLAS_OK;
    r.rho = rz, r.residual(rr, false);
    bad += agree(b, r, "pcg start");
    for (int k = 0; k < 60; ++k) {
        double pq = rnd();
        if (k == at) pq = poison;
        bad += step(SBLAS_KRYLOV_STEP_PCG_ALPHA, 0, {pq}, b) != SBLAS_OK;
        if (r.status == SBLAS_KRYLOV_RUNNING) {
            if (Restated::bad(pq)) r.down(SBLAS_KRYLOV_DENOM_PQ);
            else r.alpha = r.rho / pq;
        }
        rr *= 0.5 * rnd(), rz = two_dots ? rr * rnd() : rr;
        bad += step(SBLAS_KRYLOV_STEP_PCG_RES, 1, two_dots ? std::vector<double>{rr, rz} : std::vector<double>{rr}, b) != SBLAS_OK;
        if (r.status == SBLAS_KRYLOV_RUNNING && r.residual(rr, true)) {
            if (Restated::bad(r.rho)) r.down(SBLAS_KRYLOV_DENOM_RHO);
            else r.beta = rz / r.rho, r.rho = rz;
        }
        bad += agree(b, r, "pcg iteration");
    }
    bad += r.status == SBLAS_KRYLOV_RUNNING; // 60 halvings meet 1e-3, or the limit of 40 does
    return bad;
}

static int bicg_run(int at, int which, double poison)
{
    int bad = 0;
    Block b;
    Restated r;
    const double bb = 4.0 * rnd();
    bad += step(SBLAS_KRYLOV_STEP_START_B, 1, {bb}, b, 1e-3, 1e-300, 40) != SBLAS_OK;
    r.begin(bb, true, 1e-3, 1e-300, 40);
    double rr = bb;
    bad += step(SBLAS_KRYLOV_STEP_START_R, 0, {rr}, b) != SBLAS_OK;
    r.rho = rr, r.residual(rr, false);
    for (int k = 0; k < 60; ++k) {
        double rv = rnd(), ts = rnd(), tt = rnd(), ss = rr * rnd(), rhr = rnd();
        if (k == at && which == 0) rv = poison;
        if (k == at && which == 1) tt = poison;
        if (k == at && which == 2) rhr = poison; // the NEXT beta's denominator
        bad += step(SBLAS_KRYLOV_STEP_BICG_ALPHA, 0, {rv}, b) != SBLAS_OK;
        if (r.status == SBLAS_KRYLOV_RUNNING) {
            if (Restated::bad(rv)) r.down(SBLAS_KRYLOV_DENOM_RV);
            else r.alpha = r.rho / rv;
        }
        bad += step(SBLAS_KRYLOV_STEP_BICG_OMEGA, 0, {ts, tt, ss}, b) != SBLAS_OK;
        if (r.status == SBLAS_KRYLOV_RUNNING) {
            if (tt == 0.0 && sqrt(ss) <= r.tol) r.omega = 0.0;
            else if (Restated::bad(tt)) r.down(SBLAS_KRYLOV_DENOM_TT);
            else r.omega = ts / tt;
        }
        rr *= 0.5 * rnd();
        bad += step(SBLAS_KRYLOV_STEP_BICG_RES, 0, {rr, rhr}, b) != SBLAS_OK;
        if (r.status == SBLAS_KRYLOV_RUNNING && r.residual(rr, true)) {
            if (Restated::bad(r.rho)) r.down(SBLAS_KRYLOV_DENOM_RHO);
            else if (Restated::bad(r.omega)) r.down(SBLAS_KRYLOV_DENOM_OMEGA);
            else r.beta = (rhr / r.rho) * (r.alpha / r.omega), r.rho = rhr;
        }
        bad += agree(b, r, "bicgstab iteration");
    }
    bad += r.status == SBLAS_KRYLOV_RUNNING;
    return bad;
}

// The overlap predicate of start (krylov_multi.h), on exact cases: two n x s blocks at byte addresses x0 and b0 with
// leading dimensions ldx and ldb, and the answer written out.  tests/test_krylov_multi_host.py reads these rows and asks
// Python's _blocks_overlap the same questions.
struct OverlapCase {
    int64_t n;
    int s;
    uintptr_t x0;
    int64_t ldx;
    uintptr_t b0;
    int64_t ldb;
    bool overlap;
};
static const OverlapCase OVERLAP_CASES[] = {
    {0, 3, 4096, 3, 4096, 3, false}, // n = 0 never overlaps, not even at one address
    {0, 3, 4096, 6, 4104, 6, false},
    {1, 3, 4096, 3, 4096, 3, true},  // n = 1: one row of s entries, 24 bytes, whatever the leading dimension
    {1, 3, 4096, 9, 4112, 9, true},
    {1, 3, 4096, 9, 4120, 9, false},
    {5, 3, 4096, 3, 4216, 3, false}, // two blocks that touch: b0 == x0 + span, span = (4 * 3 + 3) * 8 = 120
    {5, 3, 4096, 3, 4215, 3, true},  // one byte less
    {5, 3, 4096, 4, 4248, 3, false}, // each side by its own leading dimension: span = (4 * 4 + 3) * 8 = 152
    {5, 3, 4096, 4, 4247, 3, true},
    {5, 3, 4096, 6, 4120, 6, true},  // the two column halves of one (5, 6) tensor at ld = 6
    {1, 3, 4096, 6, 4120, 6, false}, // the same halves of a (1, 6) tensor: two rows side by side
};

int main()
{
    int bad = 0;
    int64_t lim[8];
    if (sblas_krylov_multi_limits(lim) != SBLAS_OK || sblas_krylov_multi_limits(nullptr) != SBLAS_E_INVALID) return 1;
    bad += lim[0] != SBLAS_KRYLOV_MULTI_MAX_RHS || lim[1] != SBLAS_KRYLOV_MULTI_TILE || lim[2] != 2048 || lim[3] != 256 || lim[6] != 3 || lim[7] != 16;
    // the kinds: none and Jacobi, nothing that is applied by launches of its own, nothing unknown
    for (int kind = -3; kind < 12; ++kind) {
        const bool takes = kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI;
        bad += (sblas_krylov_multi_precond_ok(kind) == SBLAS_OK) != takes;
        for (int64_t spmm : {(int64_t)0, (int64_t)1, (int64_t)9}) {
            bad += sblas_krylov_multi_launches(SBLAS_KRYLOV_PCG, kind, spmm) != (takes ? spmm + 5 : -1);
            bad += sblas_krylov_multi_launches(SBLAS_KRYLOV_BICGSTAB, kind, spmm) != (takes ? 2 * spmm + 8 : -1);
        }
        bad += sblas_krylov_multi_launches(SBLAS_KRYLOV_PCG, kind, -1) != -1 || sblas_krylov_multi_launches(2, kind, 1) != -1;
    }
    // the grid of every width at the edge sizes
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2047, (int64_t)2048, (int64_t)2049, (int64_t)2147483583}) {
        for (int s = -1; s <= SBLAS_KRYLOV_MULTI_MAX_RHS + 1; ++s) {
            std::vector<int64_t> g(4, -7); // exactly four
            const int rc = sblas_krylov_multi_grid(n, s, g.data());
            if (s < 1 || s > SBLAS_KRYLOV_MULTI_MAX_RHS) {
                bad += rc != SBLAS_E_INVALID || g[0] != -7;
                continue;
            }
            const int64_t cells = (n + 2047) / 2048, tiles = (s + 7) / 8;
            bad += rc != SBLAS_OK || g[0] != cells || g[1] != tiles || g[2] != cells * tiles || g[3] != s - 8 * (tiles - 1) || g[3] < 1 || g[3] > 8;
        }
    }
    bad += sblas_krylov_multi_grid(-1, 1, lim) != SBLAS_E_INVALID || sblas_krylov_multi_grid(1, 1, nullptr) != SBLAS_E_INVALID;
    // the scalar step's own refusals: a bad op, a bad nd, too few sums for the op, missing arrays -- nothing is written
    {
        Block b;
        std::vector<double> d1(1, 1.0), d2(2, 1.0);
        bad += sblas_krylov_scalar_step_ref(0, 1, 0, d1.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(10, 1, 0, d1.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_PCG_RES, 0, 0, d1.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_PCG_RES, 4, 0, d1.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_BICG_OMEGA, 2, 0, d2.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_BICG_RES, 1, 0, d1.data(), b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_RHO0, 1, 0, nullptr, b.v.data(), 0, 0, 0) != SBLAS_E_INVALID;
        bad += sblas_krylov_scalar_step_ref(SBLAS_KRYLOV_STEP_RHO0, 1, 0, d1.data(), nullptr, 0, 0, 0) != SBLAS_E_INVALID;
        for (double x : b.v) bad += x != -7.0;
    }
    // whole recurrences, clean and with every denominator poisoned at the first, a middle and a late step
    const double poisons[4] = {0.0, INFINITY, -INFINITY, NAN};
    for (int two = 0; two < 2; ++two) {
        bad += pcg_run(-1, 0.0, two != 0);
        for (int at : {0, 3, 7})
            for (double p : poisons) bad += pcg_run(at, p, two != 0);
    }
    bad += bicg_run(-1, 0, 0.0);
    for (int which = 0; which < 3; ++which)
        for (int at : {0, 2, 5})
            for (double p : poisons) bad += bicg_run(at, which, p);
    // b == 0 and a NaN b: converged at once with zero_x set; never converged
    {
        Block b;
        bad += step(SBLAS_KRYLOV_STEP_START_B, 0, {0.0}, b, 1e-8, 0.0, 10) != SBLAS_OK;
        bad += b.i(STATUS) != SBLAS_KRYLOV_CONVERGED || b.i(ZERO_X) != 1 || b.f(BNORM) != 0.0;
        const std::vector<double> before = b.v;
        bad += step(SBLAS_KRYLOV_STEP_START_R, 0, {1.0}, b) != SBLAS_OK; // frozen: nothing changes
        bad += memcmp(before.data(), b.v.data(), 16 * 8) != 0;
        Block c;
        bad += step(SBLAS_KRYLOV_STEP_START_B, 0, {NAN}, c, 1e-8, 0.0, 10) != SBLAS_OK;
        bad += step(SBLAS_KRYLOV_STEP_START_R, 0, {NAN}, c) != SBLAS_OK;
        bad += c.i(STATUS) != SBLAS_KRYLOV_RUNNING || c.i(ZERO_X) != 0;
        bad += step(SBLAS_KRYLOV_STEP_PCG_ALPHA, 0, {NAN}, c) != SBLAS_OK;
        bad += c.i(STATUS) != SBLAS_KRYLOV_BREAKDOWN || c.i(WHICH) != SBLAS_KRYLOV_DENOM_PQ || c.i(ITER) != 0;
    }
    // start's "X overlaps B", both ways round
    for (const OverlapCase &c : OVERLAP_CASES) {
        bad += sblas::blocks_overlap(c.x0, c.ldx, c.b0, c.ldb, c.n, c.s) != c.overlap;
        bad += sblas::blocks_overlap(c.b0, c.ldb, c.x0, c.ldx, c.n, c.s) != c.overlap;
    }
    printf(bad ? "krylov_multi_rule_check: %d mismatches\n" : "krylov_multi_rule_check: ok\n", bad);
    return bad ? 1 : 0;
}
