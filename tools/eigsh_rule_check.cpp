// eigsh_rule_check.cpp -- a stand-alone program over the eigenvalue plan's host rule (s-blas_amd/csrc/eigsh_rule.cpp; no
// GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/eigsh_rule_check.cpp s-blas_amd/csrc/eigsh_rule.cpp -o /tmp/eigsh_rule_check && /tmp/eigsh_rule_check
// For every mm from 1 to 64 it runs the Jacobi loop, the whole Ritz step and the rotation out of arrays of exactly the
// sizes the contract names (so a read or write past either end is the sanitizer's to find): a random symmetric T, a
// diagonal T, a NaN, beta == 0, keep at both ends; and it checks what must hold whatever the rounding: T Y = Y Theta to a
// few units of eps |T|, Y orthonormal, the order of the Ritz values, and the rotation against a second restatement.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

static uint64_t state = 88172645463325252ull;
static double rnd()
{
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    return (double)(int64_t)(state >> 11) / 9007199254740992.0 - 0.5;
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (isnan(a) && isnan(b)); }

static int64_t lim[16];

struct Blocks {
    std::vector<int64_t> blk;
    std::vector<double> mat;
    double *f() { return reinterpret_cast<double *>(blk.data()); }
    Blocks(int mm, const std::vector<double> &T, double beta, bool invariant, int64_t restarts, int64_t max_restarts)
        : blk((size_t)lim[4], 0), mat((size_t)lim[5], 0.0)
    {
        blk[0] = SBLAS_KRYLOV_RUNNING, blk[1] = restarts, blk[3] = mm, blk[10] = max_restarts, blk[12] = invariant;
        f()[4] = beta, f()[8] = 1e-8, f()[9] = 0.0;
        for (int c = 0; c < mm; ++c)
            for (int r = 0; r < mm; ++r) mat[(size_t)(lim[6] + c * lim[2] + r)] = T[(size_t)c * mm + r];
    }
};

int main()
{
    int bad = 0;
    if (sblas_eigsh_limits(lim) != SBLAS_OK || sblas_eigsh_limits(nullptr) != SBLAS_E_INVALID) return 1;
    const int M = (int)lim[0], LD = (int)lim[2];
    bad += M != SBLAS_EIGSH_MAX_NCV || lim[4] != SBLAS_EIGSH_BLOCK_SLOTS || lim[5] != SBLAS_EIGSH_MATRIX_DOUBLES;
    const double eps = ldexp(1.0, -52);
    for (int mm = 1; mm <= M; ++mm) {
        std::vector<double> T((size_t)mm * mm), D((size_t)mm * mm, 0.0);
        double fro = 0.0;
        for (int c = 0; c < mm; ++c)
            for (int r = 0; r <= c; ++r) {
                const double v = ldexp(rnd(), (int)(state % 6) - 3);
                T[(size_t)c * mm + r] = T[(size_t)r * mm + c] = v;
                fro += (r == c ? 1.0 : 2.0) * v * v;
            }
        fro = sqrt(fro);
        for (int i = 0; i < mm; ++i) D[(size_t)i * mm + i] = rnd();
        // the Jacobi loop: theta, Y of exactly mm and mm x mm entries
        {
            std::vector<double> theta((size_t)mm), Y((size_t)mm * mm);
            int sweeps = -1;
            if (sblas_eigsh_jacobi_ref(mm, T.data(), mm, theta.data(), Y.data(), mm, &sweeps) != SBLAS_OK) ++bad;
            double worst = 0.0, orth = 0.0;
            for (int c = 0; c < mm; ++c)
                for (int r = 0; r < mm; ++r) {
                    double ty = 0.0, yy = 0.0;
                    for (int l = 0; l < mm; ++l) ty += T[(size_t)l * mm + r] * Y[(size_t)c * mm + l], yy += Y[(size_t)r * mm + l] * Y[(size_t)c * mm + l];
                    worst = fmax(worst, fabs(ty - Y[(size_t)c * mm + r] * theta[(size_t)c]));
                    orth = fmax(orth, fabs(yy - (r == c ? 1.0 : 0.0)));
                }
            if (!(worst <= 64.0 * eps * fro) || !(orth <= 512.0 * eps) || sweeps < 0 || sweeps >= lim[3]) {
                printf("mm = %d: Jacobi's residual %g eps |T|, orthogonality %g eps, %d sweeps\n", mm, worst / (eps * fro), orth / eps, sweeps);
                ++bad;
            }
            // a diagonal T is left as it is, in no sweep at all
            std::vector<double> th2((size_t)mm), Y2((size_t)mm * mm);
            if (sblas_eigsh_jacobi_ref(mm, D.data(), mm, th2.data(), Y2.data(), mm, &sweeps) != SBLAS_OK || sweeps != 0) ++bad;
            for (int i = 0; i < mm; ++i) bad += !same(th2[(size_t)i], D[(size_t)i * mm + i]) || Y2[(size_t)i * mm + i] != 1.0;
        }
        // the Ritz step: keep at both ends, all three orders, beta == 0, a NaN
        const int k = mm < 4 ? 1 : 4;
        const int keeps[2] = {k, mm - 1 > k ? (mm - 1 < M - 1 ? mm - 1 : M - 1) : k};
        for (int keep : keeps)
            for (int which = 0; which < 3; ++which) {
                Blocks b(mm, T, 0.25, false, 0, 300);
                if (sblas_eigsh_ritz_ref(k, keep, which, b.f(), b.mat.data()) != SBLAS_OK) ++bad;
                const int kk = keep < mm ? keep : mm;
                const double *theta = b.mat.data() + lim[8], *Tn = b.mat.data() + lim[6];
                bool ok = b.blk[1] == 1 && b.blk[3] == kk && b.blk[13] == mm && b.blk[14] == kk && b.blk[6] == 1;
                for (int r = 1; r < mm && ok; ++r) {
                    const double a = which == 2 ? fabs(theta[r - 1]) : theta[r - 1], c = which == 2 ? fabs(theta[r]) : theta[r];
                    ok = which == 1 ? a <= c : a >= c;
                }
                for (int r = 0; r < kk && ok; ++r) ok = same(Tn[r * LD + r], theta[r]);
                if (!ok) {
                    printf("mm = %d, keep = %d, which = %d: the Ritz step's order or its block is wrong\n", mm, keep, which);
                    ++bad;
                }
            }
        {
            Blocks b(mm, T, 0.0, true, 0, 300); // an invariant subspace: every estimate 0, CONVERGED when mm >= k
            if (sblas_eigsh_ritz_ref(k, keeps[1], 0, b.f(), b.mat.data()) != SBLAS_OK || b.blk[0] != SBLAS_KRYLOV_CONVERGED) ++bad;
            for (int r = 0; r < mm; ++r) bad += b.mat[(size_t)(lim[9] + r)] != 0.0;
            if (mm < M - 1) {
                Blocks s(mm, T, 0.0, true, 0, 300); // fewer columns than k: BREAKDOWN, naming the count
                if (sblas_eigsh_ritz_ref(mm + 1, mm + 1, 1, s.f(), s.mat.data()) != SBLAS_OK) ++bad;
                bad += s.blk[0] != SBLAS_KRYLOV_BREAKDOWN || s.blk[5] != SBLAS_EIGSH_DENOM_INVARIANT || s.blk[13] != mm;
            }
            std::vector<double> N = T;
            N[(size_t)(mm - 1) * mm] = N[(size_t)mm - 1] = NAN;
            Blocks n(mm, N, 1.0, false, 0, 300);
            const std::vector<double> before = n.mat;
            if (sblas_eigsh_ritz_ref(k, keeps[0], 0, n.f(), n.mat.data()) != SBLAS_OK) ++bad;
            bad += n.blk[0] != SBLAS_KRYLOV_BREAKDOWN || n.blk[5] != SBLAS_EIGSH_DENOM_T || n.blk[1] != 0 || n.blk[6] != 0;
            for (size_t e = 0; e < before.size(); ++e) bad += !same(before[e], n.mat[e]);
            Blocks l(mm, T, 5.0, false, 2, 3);
            if (sblas_eigsh_ritz_ref(k, keeps[0], 0, l.f(), l.mat.data()) != SBLAS_OK) ++bad;
            bad += l.blk[0] != SBLAS_KRYLOV_LIMIT || l.blk[1] != 3 || l.blk[6] != 1; // the third restart is the last: LIMIT, and the rotation still acts
        }
        // the rotation: V of exactly (mm + 1) n entries, Q of exactly mm keep, against the order written once more
        for (int keep : {1, mm}) {
            const int64_t n = 37;
            std::vector<double> V((size_t)(mm + 1) * n), Q((size_t)mm * keep), W;
            for (double &v : V) v = ldexp(rnd(), (int)(state % 20) - 10);
            for (double &v : Q) v = rnd();
            W = V;
            if (sblas_eigsh_rotate_ref(n, mm, keep, V.data(), n, Q.data(), mm) != SBLAS_OK) ++bad;
            bool ok = true;
            for (int64_t row = 0; row < n && ok; ++row) {
                for (int i = 0; i < keep && ok; ++i) {
                    double acc = Q[(size_t)i * mm] * W[(size_t)row];
                    for (int l = 1; l < mm; ++l) {
                        const double p = Q[(size_t)i * mm + l] * W[(size_t)l * n + row];
                        acc = acc + p;
                    }
                    ok = same(V[(size_t)i * n + row], acc);
                }
                ok = ok && same(V[(size_t)keep * n + row], W[(size_t)mm * n + row]);
                for (int l = keep + 1; l <= mm && ok; ++l) ok = same(V[(size_t)l * n + row], W[(size_t)l * n + row]);
            }
            if (!ok) {
                printf("mm = %d, keep = %d: the rotation differs from its restatement\n", mm, keep);
                ++bad;
            }
        }
        // the scalar part of a step: T's column and row mm - 1, the count, beta's three meanings
        {
            std::vector<int64_t> blk((size_t)lim[4], 0);
            std::vector<double> mat((size_t)lim[5], 0.0), h((size_t)mm);
            for (double &v : h) v = rnd();
            double *f = reinterpret_cast<double *>(blk.data());
            blk[3] = mm - 1;
            bad += sblas_eigsh_step_ref(mm - 1, h.data(), 0.5, f, mat.data()) != 1 || blk[3] != mm || blk[2] != 1 || f[4] != 0.5;
            for (int i = 0; i < mm; ++i)
                bad += !same(mat[(size_t)(lim[6] + (mm - 1) * LD + i)], h[(size_t)i]) || !same(mat[(size_t)(lim[6] + i * LD + mm - 1)], h[(size_t)i]);
            blk[3] = mm - 1;
            bad += sblas_eigsh_step_ref(mm - 1, h.data(), 0.0, f, mat.data()) != 0 || blk[3] != mm || blk[12] != 1 || blk[0] != SBLAS_KRYLOV_RUNNING;
            blk[3] = mm - 1, blk[12] = 0;
            bad += sblas_eigsh_step_ref(mm - 1, h.data(), INFINITY, f, mat.data()) != 0 || blk[3] != mm - 1 || blk[0] != SBLAS_KRYLOV_BREAKDOWN ||
                   blk[5] != SBLAS_EIGSH_DENOM_BETA;
        }
    }
    // arguments
    {
        double one[4] = {1.0, 1.0, 1.0, 1.0};
        int64_t out[4], sz[2];
        int sweeps;
        bad += sblas_eigsh_jacobi_ref(0, one, 1, one, one, 1, &sweeps) != SBLAS_E_INVALID;
        bad += sblas_eigsh_jacobi_ref(M + 1, one, M + 1, one, one, M + 1, &sweeps) != SBLAS_E_INVALID;
        bad += sblas_eigsh_jacobi_ref(2, one, 1, one, one, 2, &sweeps) != SBLAS_E_INVALID;
        bad += sblas_eigsh_jacobi_ref(1, nullptr, 1, one, one, 1, nullptr) != SBLAS_E_INVALID;
        bad += sblas_eigsh_ritz_ref(1, 1, 3, one, one) != SBLAS_E_INVALID || sblas_eigsh_ritz_ref(2, 1, 0, one, one) != SBLAS_E_INVALID;
        bad += sblas_eigsh_ritz_ref(1, M, 0, one, one) != SBLAS_E_INVALID || sblas_eigsh_ritz_ref(1, 1, 0, nullptr, one) != SBLAS_E_INVALID;
        bad += sblas_eigsh_rotate_ref(4, 1, 2, one, 4, one, 1) != SBLAS_E_INVALID || sblas_eigsh_rotate_ref(4, 1, 1, one, 3, one, 1) != SBLAS_E_INVALID;
        bad += sblas_eigsh_rotate_ref(4, M + 1, 1, one, 4, one, M + 1) != SBLAS_E_INVALID || sblas_eigsh_rotate_ref(0, 1, 1, nullptr, 0, one, 1) != SBLAS_OK;
        bad += sblas_eigsh_launches(20, 12, out) != 74 || out[0] != 9 || out[1] != 111 || out[2] != 74 || out[3] != 2;
        bad += sblas_eigsh_launches(64, 63, out) != 11 || sblas_eigsh_launches(65, 12, out) != -1 || sblas_eigsh_launches(20, 20, out) != -1;
        bad += sblas_eigsh_launches(20, 12, nullptr) != -1;
        bad += sblas_eigsh_sizes(1000, 4, 0, 0, sz) != SBLAS_OK || sz[0] != 20 || sz[1] != 12;
        bad += sblas_eigsh_sizes(1000, 30, 0, 0, sz) != SBLAS_OK || sz[0] != 61 || sz[1] != 45;
        bad += sblas_eigsh_sizes(1000, 40, 0, 0, sz) != SBLAS_OK || sz[0] != 64 || sz[1] != 52;
        bad += sblas_eigsh_sizes(10, 4, 0, 0, sz) != SBLAS_OK || sz[0] != 9 || sz[1] != 6;
        bad += sblas_eigsh_sizes(1000, 20, 20, 0, sz) != SBLAS_E_INVALID || sblas_eigsh_sizes(1000, 4, 65, 0, sz) != SBLAS_E_INVALID;
        bad += sblas_eigsh_sizes(20, 4, 20, 0, sz) != SBLAS_E_INVALID || sblas_eigsh_sizes(1000, 4, 20, 3, sz) != SBLAS_E_INVALID;
        bad += sblas_eigsh_sizes(1000, 4, 20, 20, sz) != SBLAS_E_INVALID || sblas_eigsh_sizes(1000, 0, 20, 0, sz) != SBLAS_E_INVALID;
        bad += sblas_eigsh_sizes(1000, 4, 20, 19, sz) != SBLAS_OK || sblas_eigsh_sizes(1000, 4, 20, 4, sz) != SBLAS_OK;
    }
    if (bad) printf("eigsh rule check: %d FAILED\n", bad);
    else printf("eigsh rule check: ok\n");
    return bad != 0;
}
