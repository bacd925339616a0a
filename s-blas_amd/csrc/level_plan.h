// level_plan.h -- the host side of a level plan, shared by the triangular solves (sptrsv.hip) and ILU(0) (ilu0.hip): the rows
// sorted by (level, row), every level packed into four-lane units, and the cut of the levels into launches.  No HIP in
// here: level_plan.cpp is testable on a CPU box, and sblas_sptrsv_pack exports the packer with a neutral record.
#pragma once
#include <stdint.h>
#include <vector>
#include "sptrsv.h"

namespace sblas {

// The rows by (level, row).  level l is perm[level_ptr[l] .. level_ptr[l + 1] - 1], widths[l] rows, and the units
// level_unit_ptr[l] .. level_unit_ptr[l + 1] - 1.
struct LevelOrder {
    std::vector<int32_t> perm, level_ptr;
    std::vector<int64_t> level_unit_ptr, widths;
};

// A unit is four lanes of a launch.  A row of G(p) lanes is G(p) / 4 consecutive units, unit_of(row, q) for q = 0 ..
// G(p) / 4 - 1, and starts on a multiple of G(p) / 4 units of its level (its butterfly stays inside one DPP row, or is one
// wave, and a lane's place in its row is its place in the level modulo G(p)); `pad` fills the gaps.  Rows ascend inside a
// level.  level: every row's level, below n_levels.
template <typename U, typename F>
void level_pack(int64_t n, const int32_t *rowptr, const int32_t *level, int64_t n_levels, F unit_of, const U &pad, LevelOrder &o,
                std::vector<U> &units)
{
    // rows by (level, row): a counting sort, stable in the row
    std::vector<int32_t> &lp = o.level_ptr;
    lp.assign((size_t)n_levels + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++lp[(size_t)level[i] + 1];
    o.widths.assign(lp.begin() + 1, lp.end());
    for (int64_t l = 0; l < n_levels; ++l) lp[l + 1] += lp[l];
    o.perm.resize((size_t)n);
    std::vector<int32_t> fillpos(lp.begin(), lp.end() - 1);
    for (int64_t i = 0; i < n; ++i) o.perm[fillpos[level[i]]++] = (int32_t)i;
    units.clear();
    units.reserve((size_t)n + (size_t)n / 4);
    o.level_unit_ptr.assign((size_t)n_levels + 1, 0);
    for (int64_t l = 0; l < n_levels; ++l) {
        const size_t first = units.size();
        o.level_unit_ptr[l] = (int64_t)first;
        for (int32_t k = lp[l]; k < lp[l + 1]; ++k) {
            const int32_t i = o.perm[k];
            const size_t per_row = (size_t)1 << (sptrsv_group_shift((int64_t)rowptr[i + 1] - rowptr[i]) - 2); // units of this row
            while ((units.size() - first) % per_row) units.push_back(pad);
            for (size_t q = 0; q < per_row; ++q) units.push_back(unit_of(i, (int32_t)q));
        }
    }
    o.level_unit_ptr[n_levels] = (int64_t)units.size();
}

struct Launch {
    int64_t l0, l1; // levels
    bool chain;
};

struct LaunchList {
    std::vector<Launch> launches;
    int64_t wide = 0, chains = 0, widest = 0; // launches of each kind; rows of the widest level
};

// sblas_sptrsv_schedule on the widths, as launches.  chain_rows: the resolved one (> 0).
int level_launches(const std::vector<int64_t> &widths, int flags, int64_t chain_rows, LaunchList &out);

} // namespace sblas
