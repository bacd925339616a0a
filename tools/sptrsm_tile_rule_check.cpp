// sptrsm_tile_rule_check.cpp -- a stand-alone program over the host rule of the tiled triangular solve and of ILU(0)'s
// seat under the multi-right-hand-side Krylov solvers (s-blas_amd/csrc/sptrsv_plan.cpp and krylov_multi_rule.cpp; no GPU,
// no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sptrsm_tile_rule_check.cpp s-blas_amd/csrc/sptrsv_plan.cpp s-blas_amd/csrc/krylov_multi_rule.cpp \
//       -o /tmp/sptrsm_tile_rule_check && /tmp/sptrsm_tile_rule_check
// It takes the limits, the grid of a wide launch at the edge unit counts and widths up to the ones whose grid no longer
// fits (into arrays of exactly four entries, so a write past the end is the sanitizer's to find, and with sums that must
// not wrap), the kinds a batch takes with a pair, and the launches of an iteration with the two solves in it against the
// sequences written out as lists.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../include/sblas_hip.h"

// the launches of one iteration as the solver enqueues them (krylov_multi.hip), one string a launch
static std::vector<std::string> pcg_sequence(int64_t spmm, int64_t lower, int64_t upper)
{
    std::vector<std::string> q(spmm, "spmm");
    for (const char *k : {"dots (p, q)", "fold alpha", "x r update", "fold residual"}) q.push_back(k);
    q.insert(q.end(), (size_t)lower, "L solve on r into z"), q.insert(q.end(), (size_t)upper, "U solve on z in place");
    for (const char *k : {"dots (r, z)", "fold beta", "p update"}) q.push_back(k);
    return q;
}

static std::vector<std::string> bicgstab_sequence(int64_t spmm, int64_t lower, int64_t upper)
{
    std::vector<std::string> q{"p update"};
    q.insert(q.end(), (size_t)lower, "L solve on p into p^"), q.insert(q.end(), (size_t)upper, "U solve on p^ in place");
    q.insert(q.end(), (size_t)spmm, "spmm");
    for (const char *k : {"dots (r^, v)", "fold alpha", "s update"}) q.push_back(k);
    q.insert(q.end(), (size_t)lower, "L solve on s into s^"), q.insert(q.end(), (size_t)upper, "U solve on s^ in place");
    q.insert(q.end(), (size_t)spmm, "spmm");
    for (const char *k : {"dots (t, s) (t, t) (s, s)", "fold omega", "x r update", "fold residual and beta"}) q.push_back(k);
    return q;
}

int main()
{
    int bad = 0;
    int64_t most = 0;
    {
        std::vector<int64_t> lim(4, -7); // exactly four
        bad += sblas_sptrsm_tile_limits(lim.data()) != SBLAS_OK || sblas_sptrsm_tile_limits(nullptr) != SBLAS_E_INVALID;
        bad += lim[0] != SBLAS_SPTRSM_TILE || lim[0] != 8 || lim[1] != 256 || lim[3] != INT_MAX;
        int64_t single[4], multi[8];
        bad += sblas_hip_sptrsv_limits(single) != SBLAS_OK || sblas_krylov_multi_limits(multi) != SBLAS_OK;
        bad += lim[2] != single[1] || lim[0] != multi[1]; // the single solve's chain workgroup, the solvers' tile
        most = lim[3];
    }
    // the grid: 64 four-lane units a workgroup, eight columns a tile
    for (int64_t units : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4095, (int64_t)4097,
                          (int64_t)2147483647, (int64_t)4294967296, INT64_MAX}) {
        for (int64_t s : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)64, (int64_t)65, (int64_t)1000,
                          (int64_t)1 << 31, (int64_t)1 << 34, (int64_t)1 << 40, INT64_MAX - 3, INT64_MAX}) {
            std::vector<int64_t> g(4, -7);
            const int rc = sblas_sptrsm_tile_grid(units, s, g.data());
            const int64_t blocks = units < 0 ? 0 : units / 64 + (units % 64 != 0), tiles = s < 1 ? 0 : s / 8 + (s % 8 != 0);
            const bool fits = blocks == 0 ? tiles <= most : tiles <= most / blocks; // no product that could wrap
            if (units < 0 || s < 1 || !fits) {
                bad += rc != SBLAS_E_INVALID || g[0] != -7 || g[3] != -7;
                continue;
            }
            bad += rc != SBLAS_OK || g[0] != blocks || g[1] != tiles || g[2] != blocks * tiles || g[2] > most;
            bad += g[3] != s - 8 * (tiles - 1) || g[3] < 1 || g[3] > 8;
        }
    }
    bad += sblas_sptrsm_tile_grid(1, 1, nullptr) != SBLAS_E_INVALID;
    // the kinds: with a pair ILU(0) alone; what the older questions answer is what it was
    for (int kind = -3; kind < 12; ++kind) {
        const bool pair = kind == SBLAS_PRECOND_ILU0;
        bad += (sblas_krylov_multi_precond_pair_ok(kind) == SBLAS_OK) != pair;
        bad += (sblas_krylov_multi_precond_plan_ok(kind) == SBLAS_OK) != (kind == SBLAS_PRECOND_AMG);
        bad += (sblas_krylov_multi_precond_ok(kind) == SBLAS_OK) != (kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI);
        for (int64_t spmm : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)17}) {
            for (int64_t lower : {(int64_t)0, (int64_t)1, (int64_t)11, (int64_t)48}) {
                for (int64_t upper : {(int64_t)0, (int64_t)1, (int64_t)11, (int64_t)48}) {
                    const int64_t pcg = sblas_krylov_multi_launches_pair(SBLAS_KRYLOV_PCG, kind, spmm, lower, upper);
                    const int64_t bicg = sblas_krylov_multi_launches_pair(SBLAS_KRYLOV_BICGSTAB, kind, spmm, lower, upper);
                    if (pair) {
                        bad += pcg != (int64_t)pcg_sequence(spmm, lower, upper).size() || pcg != spmm + 5 + lower + upper + 2;
                        bad += bicg != (int64_t)bicgstab_sequence(spmm, lower, upper).size() || bicg != 2 * spmm + 8 + 2 * (lower + upper);
                        // the AMG count with the two solves in the cycle's place
                        bad += pcg != sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_PCG, SBLAS_PRECOND_AMG, spmm, lower + upper);
                        bad += bicg != sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_BICGSTAB, SBLAS_PRECOND_AMG, spmm, lower + upper);
                    } else {
                        bad += pcg != -1 || bicg != -1;
                    }
                    bad += sblas_krylov_multi_launches_pair(2, kind, spmm, lower, upper) != -1;
                    bad += sblas_krylov_multi_launches_pair(-1, kind, spmm, lower, upper) != -1;
                }
                bad += sblas_krylov_multi_launches_pair(SBLAS_KRYLOV_PCG, kind, spmm, lower, -1) != -1;
                bad += sblas_krylov_multi_launches_pair(SBLAS_KRYLOV_PCG, kind, spmm, -1, lower) != -1;
            }
        }
        bad += sblas_krylov_multi_launches_pair(SBLAS_KRYLOV_PCG, kind, -1, 1, 1) != -1;
        // the older functions keep returning -1 for ILU(0)
        if (pair) bad += sblas_krylov_multi_launches(SBLAS_KRYLOV_PCG, kind, 2) != -1 || sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_PCG, kind, 2, 3) != -1;
    }
    printf(bad ? "sptrsm_tile_rule_check: %d mismatches\n" : "sptrsm_tile_rule_check: ok\n", bad);
    return bad ? 1 : 0;
}
