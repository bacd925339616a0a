// krylov.h -- the sizes krylov.hip's kernels and krylov_rule.cpp's host rule agree on, and the layout of the device
// scalar block.  No HIP in here: krylov_rule.cpp is testable on a CPU box.
#pragma once
#include <stdint.h>

namespace sblas {

// A dot product is cut into cells of KRYLOV_CELL consecutive elements, one workgroup of KRYLOV_LANES lanes a cell; the
// second stage is one workgroup of KRYLOV_LANES lanes over the cells' sums (include/sblas_hip.h states the order).
constexpr int KRYLOV_CELL = 2048;
constexpr int KRYLOV_LANES = 256;
constexpr int KRYLOV_PER_LANE = KRYLOV_CELL / KRYLOV_LANES;
constexpr int KRYLOV_MAX_DOTS = 3; // dots of one pass over memory
static_assert(KRYLOV_LANES == 256, "the fold is four waves of 64: steps 1 .. 32 inside a wave, 64 and 128 across");
static_assert(KRYLOV_CELL % KRYLOV_LANES == 0, "every lane of a full cell takes the same number of elements");

inline int64_t krylov_cells(int64_t n) { return (n + KRYLOV_CELL - 1) / KRYLOV_CELL; }

// Work vectors a plan owns, n doubles each (the ILU(0) solves' temporary is one more).
//   PCG       r, p, q, z                        (z is r itself without a preconditioner, but the slot is kept)
//   BiCGStab  r, r^, p, v, s, t, p^, s^         (p^ and s^ are p and s themselves without a preconditioner)
constexpr int KRYLOV_PCG_VECTORS = 4;
constexpr int KRYLOV_BICGSTAB_VECTORS = 8;

// The device scalar block: KRYLOV_BLOCK_SLOTS eight-byte slots.  Every scalar of the recurrence lives here and is read
// by the update kernels from here; the host never passes one.  status / iterations / max_iter / which are int64.
enum KrylovSlot {
    KS_STATUS = 0,  // SBLAS_KRYLOV_RUNNING / _CONVERGED / _BREAKDOWN / _LIMIT
    KS_ITER = 1,    // finished iterations
    KS_RNORM = 2,   // |r| of the recurrence
    KS_BNORM = 3,   // |b|
    KS_ALPHA = 4,
    KS_BETA = 5,
    KS_OMEGA = 6,
    KS_WHICH = 7,   // SBLAS_KRYLOV_DENOM_* of a breakdown, else 0
    KS_RHO = 8,     // PCG: (r, z); BiCGStab: (r^, r)
    KS_TOL = 9,     // max(rtol * |b|, atol)
    KS_MAX_ITER = 10,
    KS_ZERO_X = 11, // b == 0: start's vector pass writes x = 0
    KRYLOV_BLOCK_SLOTS = 16
};

} // namespace sblas
