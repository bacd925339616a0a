// amg_multi_rule_check.cpp -- a stand-alone program over the host rule of the block AMG cycle and of its seat under the
// multi-right-hand-side Krylov solvers (s-blas_amd/csrc/amg_rule.cpp and krylov_multi_rule.cpp; no GPU, no HIP runtime),
// made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/amg_multi_rule_check.cpp s-blas_amd/csrc/amg_rule.cpp s-blas_amd/csrc/ilu0_plan.cpp \
//       s-blas_amd/csrc/krylov_multi_rule.cpp -o /tmp/amg_multi_rule_check && /tmp/amg_multi_rule_check
// It takes the limits, the grid of a multi-column row kernel for every width from -1 to 65 at the edge unit counts (into
// arrays of exactly four entries, so a write past the end is the sanitizer's to find), the kinds a batch takes with a
// plan, and the launches of an iteration with a block cycle in it against the sequences written out as lists.
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../include/sblas_hip.h"

// the launches of one iteration as the solver enqueues them (krylov_multi.hip), one string a launch
static std::vector<std::string> pcg_sequence(int64_t spmm, int64_t cycle, bool amg)
{
    std::vector<std::string> q(spmm, "spmm");
    for (const char *k : {"dots (p, q)", "fold alpha", "x r update", "fold residual"}) q.push_back(k);
    if (amg) {
        q.insert(q.end(), (size_t)cycle, "cycle");
        q.push_back("dots (r, z)"), q.push_back("fold beta");
    }
    q.push_back("p update");
    return q;
}

static std::vector<std::string> bicgstab_sequence(int64_t spmm, int64_t cycle, bool amg)
{
    std::vector<std::string> q{"p update"};
    if (amg) q.insert(q.end(), (size_t)cycle, "cycle on p");
    q.insert(q.end(), (size_t)spmm, "spmm");
    for (const char *k : {"dots (r^, v)", "fold alpha", "s update"}) q.push_back(k);
    if (amg) q.insert(q.end(), (size_t)cycle, "cycle on s");
    q.insert(q.end(), (size_t)spmm, "spmm");
    for (const char *k : {"dots (t, s) (t, t) (s, s)", "fold omega", "x r update", "fold residual and beta"}) q.push_back(k);
    return q;
}

int main()
{
    int bad = 0;
    {
        std::vector<int64_t> lim(4, -7); // exactly four
        bad += sblas_amg_multi_limits(lim.data()) != SBLAS_OK || sblas_amg_multi_limits(nullptr) != SBLAS_E_INVALID;
        bad += lim[0] != SBLAS_AMG_MULTI_MAX_RHS || lim[1] != SBLAS_AMG_MULTI_TILE || lim[2] != 256 || lim[3] != 0;
        int64_t single[8], multi[8];
        bad += sblas_amg_limits(single) != SBLAS_OK || sblas_krylov_multi_limits(multi) != SBLAS_OK;
        bad += lim[2] != single[2] || lim[0] != multi[0] || lim[1] != multi[1]; // the cycle's workgroup, the solvers' blocks
    }
    // the grid: 64 four-lane units a workgroup, eight columns a tile
    for (int64_t units : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4095, (int64_t)4097,
                          (int64_t)2147483647, (int64_t)4294967296}) {
        for (int s = -1; s <= SBLAS_AMG_MULTI_MAX_RHS + 1; ++s) {
            std::vector<int64_t> g(4, -7);
            const int rc = sblas_amg_multi_grid(units, s, g.data());
            if (units < 0 || s < 1 || s > SBLAS_AMG_MULTI_MAX_RHS) {
                bad += rc != SBLAS_E_INVALID || g[0] != -7 || g[3] != -7;
                continue;
            }
            const int64_t blocks = units / 64 + (units % 64 != 0), tiles = (s + 7) / 8;
            bad += rc != SBLAS_OK || g[0] != blocks || g[1] != tiles || g[2] != blocks * tiles || g[3] != s - 8 * (tiles - 1) || g[3] < 1 || g[3] > 8;
        }
    }
    bad += sblas_amg_multi_grid(1, 1, nullptr) != SBLAS_E_INVALID;
    // the kinds: with a plan AMG alone; without one none and Jacobi, as before
    for (int kind = -3; kind < 12; ++kind) {
        const bool alone = kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI, with_plan = kind == SBLAS_PRECOND_AMG;
        bad += (sblas_krylov_multi_precond_plan_ok(kind) == SBLAS_OK) != with_plan;
        bad += (sblas_krylov_multi_precond_ok(kind) == SBLAS_OK) != alone;
        for (int64_t spmm : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)17}) {
            for (int64_t cycle : {(int64_t)0, (int64_t)1, (int64_t)11, (int64_t)48, (int64_t)1 << 40}) {
                const int64_t pcg = sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_PCG, kind, spmm, cycle);
                const int64_t bicg = sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_BICGSTAB, kind, spmm, cycle);
                if (with_plan && cycle <= 48) {
                    bad += pcg != (int64_t)pcg_sequence(spmm, cycle, true).size() || pcg != spmm + 5 + cycle + 2;
                    bad += bicg != (int64_t)bicgstab_sequence(spmm, cycle, true).size() || bicg != 2 * spmm + 8 + 2 * cycle;
                } else if (with_plan) {
                    bad += pcg != spmm + 7 + cycle || bicg != 2 * spmm + 8 + 2 * cycle;
                } else if (alone && cycle == 0) { // the old function, and the written sequence without a cycle
                    bad += pcg != sblas_krylov_multi_launches(SBLAS_KRYLOV_PCG, kind, spmm) || pcg != (int64_t)pcg_sequence(spmm, 0, false).size();
                    bad += bicg != sblas_krylov_multi_launches(SBLAS_KRYLOV_BICGSTAB, kind, spmm) ||
                           bicg != (int64_t)bicgstab_sequence(spmm, 0, false).size();
                } else {
                    bad += pcg != -1 || bicg != -1;
                }
                bad += sblas_krylov_multi_launches_ex(2, kind, spmm, cycle) != -1 || sblas_krylov_multi_launches_ex(-1, kind, spmm, cycle) != -1;
            }
            bad += sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_PCG, kind, spmm, -1) != -1;
        }
        bad += sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_PCG, kind, -1, 1) != -1 || sblas_krylov_multi_launches_ex(SBLAS_KRYLOV_BICGSTAB, kind, -1, 0) != -1;
        // the old function gives what it gave
        bad += sblas_krylov_multi_launches(SBLAS_KRYLOV_PCG, kind, 2) != (alone ? 7 : -1);
    }
    printf(bad ? "amg_multi_rule_check: %d mismatches\n" : "amg_multi_rule_check: ok\n", bad);
    return bad ? 1 : 0;
}
