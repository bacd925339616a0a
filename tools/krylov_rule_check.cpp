// krylov_rule_check.cpp -- a stand-alone program over the Krylov solvers' host rule (s-blas_amd/csrc/krylov_rule.cpp; no
// GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/krylov_rule_check.cpp s-blas_amd/csrc/krylov_rule.cpp -o /tmp/krylov_rule_check && /tmp/krylov_rule_check
// It calls sblas_krylov_dot_ref on every edge size from arrays of exactly n entries (so a read past either end is the
// sanitizer's to find) and sblas_krylov_launches on every argument class, and compares the dot with a second
// restatement of the written order.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../include/sblas_hip.h"

#pragma clang fp contract(off)

static double butterfly(std::vector<double> v)
{
    for (size_t m = 1; m < v.size(); m <<= 1) {
        std::vector<double> w(v.size());
        for (size_t l = 0; l < v.size(); ++l) w[l] = v[l] + v[l ^ m];
        v = w;
    }
    return v[0];
}

static double restated(int64_t n, const double *x, const double *y, int64_t C, int64_t W)
{
    const int64_t cells = (n + C - 1) / C;
    std::vector<double> partial((size_t)cells);
    for (int64_t c = 0; c < cells; ++c) {
        std::vector<double> lane((size_t)W, 0.0);
        for (int64_t e = c * C; e < n && e < (c + 1) * C; ++e) { // ascending e visits every lane's elements in its order
            const double prod = x[e] * y[e];
            lane[(size_t)((e - c * C) % W)] = lane[(size_t)((e - c * C) % W)] + prod;
        }
        partial[(size_t)c] = butterfly(lane);
    }
    std::vector<double> lane((size_t)W, 0.0);
    for (int64_t c = 0; c < cells; ++c) lane[(size_t)(c % W)] = lane[(size_t)(c % W)] + partial[(size_t)c];
    return butterfly(lane);
}

int main()
{
    int64_t lim[5];
    if (sblas_krylov_limits(lim) != SBLAS_OK || sblas_krylov_limits(nullptr) != SBLAS_E_INVALID) return 1;
    const int64_t C = lim[0], W = lim[1];
    const int64_t sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5, W * C + 3};
    int bad = 0;
    uint64_t state = 88172645463325252ull;
    for (int64_t n : sizes) {
        std::vector<double> x((size_t)n), y((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            state ^= state << 13, state ^= state >> 7, state ^= state << 17;
            x[(size_t)i] = ldexp((double)(int64_t)(state >> 11) / 9007199254740992.0 - 0.5, (int)(state % 600) - 300);
            state ^= state << 13, state ^= state >> 7, state ^= state << 17;
            y[(size_t)i] = ldexp((double)(int64_t)(state >> 11) / 9007199254740992.0 - 0.5, (int)(state % 600) - 300);
        }
        const double got = sblas_krylov_dot_ref(n, x.data(), y.data()), want = restated(n, x.data(), y.data(), C, W);
        if (memcmp(&got, &want, 8) != 0 && !(isnan(got) && isnan(want))) {
            printf("n = %lld: %a, restated %a\n", (long long)n, got, want);
            ++bad;
        }
    }
    if (sblas_krylov_dot_ref(5, nullptr, nullptr) != 0.0 || sblas_krylov_dot_ref(-1, nullptr, nullptr) != 0.0) ++bad;
    int64_t lower[12] = {0}, upper[12] = {0};
    lower[5] = 3, upper[5] = 7;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_NONE, nullptr, nullptr) != 6;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_JACOBI, nullptr, nullptr) != 6;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_ILU0, lower, upper) != 18;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_BICGSTAB, SBLAS_PRECOND_NONE, nullptr, nullptr) != 10;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_BICGSTAB, SBLAS_PRECOND_ILU0, lower, upper) != 30;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_ILU0, nullptr, upper) != -1;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_ILU0, lower, nullptr) != -1;
    bad += sblas_krylov_launches(2, SBLAS_PRECOND_NONE, nullptr, nullptr) != -1;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, 3, nullptr, nullptr) != -1;
    lower[5] = -1;
    bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_ILU0, lower, upper) != -1;
    // every kind (and the codes on either side), with each info missing, negative or good: an applied kind adds its M^-1
    // once to PCG and twice to BiCGStab, ILU(0) from both infos and a cycle or a polynomial from the lower one alone
    for (int precond = -1; precond <= 5; ++precond)
        for (int lo = 0; lo < 3; ++lo)
            for (int up = 0; up < 3; ++up) {
                lower[5] = lo == 1 ? -1 : 3, upper[5] = up == 1 ? -1 : 7;
                const int64_t *li = lo ? lower : nullptr, *ui = up ? upper : nullptr;
                const bool solves = precond == SBLAS_PRECOND_ILU0, single = precond == SBLAS_PRECOND_AMG || precond == SBLAS_PRECOND_CHEBYSHEV;
                const bool refused = precond < 0 || precond > 4 || (solves && (lo != 2 || up != 2)) || (single && lo != 2);
                const int64_t apply = solves ? 10 : 3;
                bad += sblas_krylov_launches(SBLAS_KRYLOV_PCG, precond, li, ui) != (refused ? -1 : solves || single ? 8 + apply : 6);
                bad += sblas_krylov_launches(SBLAS_KRYLOV_BICGSTAB, precond, li, ui) != (refused ? -1 : solves || single ? 10 + 2 * apply : 10);
            }
    if (bad) printf("krylov rule check: %d FAILED\n", bad);
    else printf("krylov rule check: ok\n");
    return bad != 0;
}
