// gmres_multi_rule_check.cpp -- a stand-alone program over the multi-right-hand-side GMRES's host rule
// (s-blas_amd/csrc/gmres_multi_rule.cpp; no GPU, no HIP runtime), made to be built with a host sanitizer:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/gmres_multi_rule_check.cpp s-blas_amd/csrc/gmres_multi_rule.cpp s-blas_amd/csrc/gmres_rule.cpp \
//       s-blas_amd/csrc/krylov_multi_rule.cpp -o /tmp/gmres_multi_rule_check && /tmp/gmres_multi_rule_check
// It takes the limits, the grid of every width from 1 to 64 at the edge sizes, the launch counts of every door at the
// ends of the restart range against the single solver's rule, and the three predicates over every kind -- every output
// array exactly as long as the contract says and on the heap, so a write past its end is the sanitizer's to find.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../include/sblas_hip.h"

// what one block M^-1 costs through each door, as the rule is written in the header
static int64_t apply_of(int kind, int64_t lo, int64_t up)
{
    if (lo < 0 || up < 0) return -1;
    if (kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI) return lo == 0 && up == 0 ? 0 : -1;
    if (kind == SBLAS_PRECOND_AMG) return up == 0 ? lo : -1;
    if (kind == SBLAS_PRECOND_ILU0) return lo + up;
    return -1;
}

int main()
{
    int bad = 0;
    std::vector<int64_t> lim(8, -7), single(8, -7), multi(8, -7);
    if (sblas_gmres_multi_limits(lim.data()) != SBLAS_OK || sblas_gmres_multi_limits(nullptr) != SBLAS_E_INVALID) return 1;
    if (sblas_gmres_limits(single.data()) != SBLAS_OK || sblas_krylov_multi_limits(multi.data()) != SBLAS_OK) return 1;
    bad += lim[0] != SBLAS_GMRES_MULTI_MAX_RHS || lim[0] != multi[0] || lim[1] != SBLAS_GMRES_MULTI_TILE || lim[1] != multi[1];
    bad += lim[2] != 2048 || lim[2] != multi[2] || lim[3] != 256 || lim[3] != multi[3];
    bad += lim[4] != SBLAS_GMRES_MULTI_MAX_RESTART || lim[4] != single[0] || lim[5] != 3 || lim[6] != 16 || lim[6] * 8 != single[5];
    bad += lim[7] * 8 != single[6];

    // the grid of every width at the edge sizes
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2047, (int64_t)2048, (int64_t)2049, (int64_t)2147483583}) {
        for (int s = -1; s <= SBLAS_GMRES_MULTI_MAX_RHS + 1; ++s) {
            std::vector<int64_t> g(4, -7); // exactly four
            const int rc = sblas_gmres_multi_grid(n, s, g.data());
            if (s < 1 || s > SBLAS_GMRES_MULTI_MAX_RHS) {
                bad += rc != SBLAS_E_INVALID || g[0] != -7;
                continue;
            }
            const int64_t cells = (n + 2047) / 2048, tiles = (s + 7) / 8;
            bad += rc != SBLAS_OK || g[0] != cells || g[1] != tiles || g[2] != cells * tiles || g[3] != s - 8 * (tiles - 1) || g[3] < 1 || g[3] > 8;
        }
    }
    bad += sblas_gmres_multi_grid(-1, 1, lim.data()) != SBLAS_E_INVALID || sblas_gmres_multi_grid(1, 1, nullptr) != SBLAS_E_INVALID;

    // the predicates over every kind, the range ends and beyond
    for (int kind = -3; kind < 12; ++kind) {
        bad += (sblas_gmres_multi_precond_ok(kind) == SBLAS_OK) != (kind == SBLAS_PRECOND_NONE || kind == SBLAS_PRECOND_JACOBI);
        bad += (sblas_gmres_multi_precond_plan_ok(kind) == SBLAS_OK) != (kind == SBLAS_PRECOND_AMG);
        bad += (sblas_gmres_multi_precond_pair_ok(kind) == SBLAS_OK) != (kind == SBLAS_PRECOND_ILU0);
        // what this plan takes through one door, the PCG / BiCGStab plan takes through its three creates
        bad += sblas_gmres_multi_precond_ok(kind) != sblas_krylov_multi_precond_ok(kind);
        bad += sblas_gmres_multi_precond_plan_ok(kind) != sblas_krylov_multi_precond_plan_ok(kind);
        bad += sblas_gmres_multi_precond_pair_ok(kind) != sblas_krylov_multi_precond_pair_ok(kind);
    }

    // the launches: the single solver's with the product's launches in the SpMV's place
    for (int m : {-1, 0, 1, 2, 30, 64, 65}) {
        for (int kind = -1; kind < 7; ++kind) {
            for (int64_t spmm : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)4}) {
                for (int64_t lo : {(int64_t)-1, (int64_t)0, (int64_t)11}) {
                    for (int64_t up : {(int64_t)-1, (int64_t)0, (int64_t)7}) {
                        std::vector<int64_t> out(4, -7); // exactly four
                        const int64_t cycle = sblas_gmres_multi_launches(m, kind, spmm, lo, up, out.data());
                        const int64_t apply = apply_of(kind, lo, up);
                        if (m < 1 || m > SBLAS_GMRES_MULTI_MAX_RESTART || spmm < 0 || apply < 0) {
                            bad += cycle != -1 || out[0] != -7 || out[3] != -7;
                            continue;
                        }
                        bad += out[0] != 8 + spmm + apply || out[1] != 3 + apply || out[2] != 3 + spmm || out[3] != 5 + spmm;
                        bad += cycle != m * out[0] + out[1] + out[2];
                        // against sblas_gmres_launches of the same kind, whose SpMV is one launch
                        std::vector<int64_t> li(12, 0), ui(12, 0), ref(4, -7);
                        li[5] = lo, ui[5] = up;
                        const int64_t one = sblas_gmres_launches(m, kind, li.data(), ui.data(), ref.data());
                        bad += one < 0 || out[0] != ref[0] - 1 + spmm || out[1] != ref[1] || out[2] != ref[2] - 1 + spmm || out[3] != ref[3] - 1 + spmm;
                    }
                }
            }
        }
    }
    bad += sblas_gmres_multi_launches(30, SBLAS_PRECOND_NONE, 1, 0, 0, nullptr) != -1;
    printf(bad ? "gmres_multi_rule_check: %d mismatches\n" : "gmres_multi_rule_check: ok\n", bad);
    return bad ? 1 : 0;
}
