// krylov_rule.cpp -- the host rule of the Krylov solvers (krylov.hip): the limits, the pinned dot product restated in
// plain C++, and the launch count of one iteration.  Pure functions of host arrays; no GPU call in this file, so it is
// testable on a CPU box (and under a host sanitizer).
#include <stdint.h>
#include <vector>
#include "../../include/sblas_hip.h"
#include "krylov.h"
#include "precond_rule.h"

#pragma clang fp contract(off) // a product is rounded, then the sum: as on the device

namespace {

// the butterfly l ^ 1, l ^ 2, ... l ^ 128 over all 256 lanes, as written: lane 0 holds the result
double butterfly(double *v, double *w)
{
    for (int m = 1; m < sblas::KRYLOV_LANES; m <<= 1) {
        for (int l = 0; l < sblas::KRYLOV_LANES; ++l) w[l] = v[l] + v[l ^ m];
        for (int l = 0; l < sblas::KRYLOV_LANES; ++l) v[l] = w[l];
    }
    return v[0];
}

} // namespace

extern "C" {

int sblas_krylov_limits(int64_t out[5])
{
    if (!out) return SBLAS_E_INVALID;
    out[0] = sblas::KRYLOV_CELL, out[1] = sblas::KRYLOV_LANES, out[2] = sblas::KRYLOV_PCG_VECTORS, out[3] = sblas::KRYLOV_BICGSTAB_VECTORS;
    out[4] = sblas::KRYLOV_MAX_DOTS;
    return SBLAS_OK;
}

double sblas_krylov_dot_ref(int64_t n, const double *x, const double *y)
{
    using namespace sblas;
    if (n <= 0 || !x || !y) return 0.0;
    const int64_t cells = krylov_cells(n);
    std::vector<double> partial((size_t)cells);
    double v[KRYLOV_LANES], w[KRYLOV_LANES];
    for (int64_t c = 0; c < cells; ++c) {
        for (int t = 0; t < KRYLOV_LANES; ++t) {
            double acc = 0.0;
            for (int k = 0; k < KRYLOV_PER_LANE; ++k) {
                const int64_t i = c * KRYLOV_CELL + t + (int64_t)k * KRYLOV_LANES;
                if (i < n) {
                    const double prod = x[i] * y[i];
                    acc = acc + prod;
                }
            }
            v[t] = acc;
        }
        partial[(size_t)c] = butterfly(v, w);
    }
    for (int t = 0; t < KRYLOV_LANES; ++t) {
        double acc = 0.0;
        for (int64_t c = t; c < cells; c += KRYLOV_LANES) acc = acc + partial[(size_t)c];
        v[t] = acc;
    }
    return butterfly(v, w);
}

int64_t sblas_krylov_launches(int method, int precond, const int64_t *lower_info, const int64_t *upper_info)
{
    if (method != SBLAS_KRYLOV_PCG && method != SBLAS_KRYLOV_BICGSTAB) return -1;
    const int64_t apply = sblas::precond_launches(precond, lower_info, upper_info); // launches of one M^-1
    if (apply < 0) return -1;
    if (method == SBLAS_KRYLOV_PCG) {
        // SpMV; (p, q): stage 1, fold; x / r update; fold; p update -- with an applied M^-1: M^-1, (r, z): stage 1, fold
        return sblas::precond_applied(precond) ? 8 + apply : 6;
    }
    // p update; SpMV; (r^, v): stage 1, fold; s update; SpMV; (t, s), (t, t) and (s, s): stage 1, fold; x / r update; fold
    return 10 + 2 * apply;
}

} // extern "C"
