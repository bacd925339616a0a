// level_plan.cpp -- the parts of level_plan.h that are no template: the launch list, and the packer behind the C ABI with
// the neutral record (row, unit number within the row).  Pure functions of host arrays; no GPU call in this file.
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include "../../include/sblas_hip.h"
#include "level_plan.h"

namespace sblas {

int level_launches(const std::vector<int64_t> &widths, int flags, int64_t chain_rows, LaunchList &out)
{
    const int64_t n_levels = (int64_t)widths.size();
    std::vector<uint8_t> kind((size_t)n_levels);
    std::vector<int64_t> lfirst((size_t)n_levels + 1);
    int64_t n_launches = 0;
    const int rc = sblas_sptrsv_schedule(n_levels, widths.data(), flags, chain_rows, kind.data(), lfirst.data(), &n_launches);
    if (rc != SBLAS_OK) return rc;
    for (int64_t w : widths) out.widest = w > out.widest ? w : out.widest;
    for (int64_t q = 0; q < n_launches; ++q) {
        const bool chain = kind[q] == SBLAS_SPTRSV_LAUNCH_CHAIN;
        out.launches.push_back(Launch{lfirst[q], lfirst[q + 1], chain});
        ++(chain ? out.chains : out.wide);
    }
    return SBLAS_OK;
}

} // namespace sblas

extern "C" int sblas_sptrsv_pack(int64_t n, const int32_t *rowptr, const int32_t *level, int64_t n_levels, int32_t *perm_out,
                                 int32_t *level_ptr_out, int64_t *level_unit_ptr_out, int32_t *unit_row_out, int32_t *unit_q_out,
                                 int64_t *n_units)
{
    if (n_units) *n_units = 0;
    if (n < 0 || n > INT_MAX - 64 || n_levels < 0 || n_levels > n || !n_units || !rowptr || (n > 0 && !level)) return SBLAS_E_INVALID;
    for (int64_t i = 0; i < n; ++i)
        if (level[i] < 0 || level[i] >= n_levels) return SBLAS_E_INVALID;
    sblas::LevelOrder o;
    std::vector<std::pair<int32_t, int32_t>> units; // (row, unit number within the row)
    sblas::level_pack(n, rowptr, level, n_levels, [](int32_t i, int32_t q) { return std::make_pair(i, q); }, std::make_pair(-1, 0), o, units);
    *n_units = (int64_t)units.size();
    if (perm_out) std::copy(o.perm.begin(), o.perm.end(), perm_out);
    if (level_ptr_out) std::copy(o.level_ptr.begin(), o.level_ptr.end(), level_ptr_out);
    if (level_unit_ptr_out) std::copy(o.level_unit_ptr.begin(), o.level_unit_ptr.end(), level_unit_ptr_out);
    for (size_t u = 0; u < units.size(); ++u) {
        if (unit_row_out) unit_row_out[u] = units[u].first;
        if (unit_q_out) unit_q_out[u] = units[u].second;
    }
    return SBLAS_OK;
}
