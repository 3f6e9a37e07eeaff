// Anderson acceleration of the device Picard loops in update space (include/kkt.h,
// kkt_anderson_set / _step / _reset): the ring of secant pairs in HBM,
// three streaming kernels and the small Cholesky solve on the host.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "../../include/kkt.h"
#include "devmem.hpp"

namespace kkt {

struct System;

constexpr int ANDERSON_MAX = KKT_ANDERSON_MAX_DEPTH;
// dot products of one Gram pass at c columns: the lower triangle of G, then r
constexpr int anderson_dots(int c) { return c * (c + 1) / 2 + c; }
constexpr int ANDERSON_DOTS_MAX = anderson_dots(ANDERSON_MAX);   // 44
// Workgroups of the Gram pass's first stage: fixed, so that the partial sums -- and with them
// every bit of G and r -- do not depend on the device's CU count.
constexpr int ANDERSON_BLOCKS = 512;
constexpr int ANDERSON_THREADS = 256;

// the columns of one launch, oldest first
struct AndersonCols {
    const double *dF[ANDERSON_MAX];
    const double *dX[ANDERSON_MAX];
    double gamma[ANDERSON_MAX];
};

struct AndersonMixer {
    int depth = 0;
    double beta = 1.0, cond_max = 1.0e7;
    int64_t n = 0;           // the handle's local vector length
    DevPool mem;             // the history: dF, dX (depth each) and f_prev; the reduction scratch
    double *d_dF[ANDERSON_MAX] = {}, *d_dX[ANDERSON_MAX] = {};
    double *d_fprev = nullptr;
    double *d_part = nullptr;   // ANDERSON_BLOCKS x ANDERSON_DOTS_MAX partials, then the sums
    // the ring: the next pair enters slot `head`, whose dX already holds the last step when
    // `have_prev`; the `count` pairs kept are the slots before it
    int head = 0, count = 0;
    bool have_prev = false;
    int slot(int j) const { return ((head - count + j) % depth + depth) % depth; }   // j-th oldest
};

// dF_new = f - f_prev, f_prev = f
void launch_anderson_push(hipStream_t s, const double *f, double *f_prev, double *dF_new,
                          int64_t n);
// part + ANDERSON_BLOCKS * ANDERSON_DOTS_MAX receives the anderson_dots(c) sums: G's lower
// triangle row by row (i >= j: i (i + 1) / 2 + j), then r; c in 1 .. ANDERSON_MAX
void launch_anderson_gram(hipStream_t s, const AndersonCols &cols, int c, const double *f,
                          int64_t n, double *part);
// s = beta f - sum_j gamma_j (dX_j + beta dF_j) into u (which holds f) and into dX_new, which
// may be one of cols.dX (the oldest pair's slot of a full ring)
void launch_anderson_mix(hipStream_t s, const AndersonCols &cols, int c, double beta, double *u,
                         double *dX_new, int64_t n);

// The condition rule on the host: G (lower triangle as above, c0 columns) and r in, the number of
// oldest columns dropped out; gamma of the c0 - dropped kept columns.
int anderson_solve(const double *tri, int c0, double cond_max, double *gamma);

void anderson_set(System &S, int depth, double beta, double cond_max);
void anderson_step(System &S, double *d_u, kkt_anderson_info *info);
void anderson_reset(System &S);
void debug_anderson_op(System &S, kkt_anderson_op *op);

}  // namespace kkt
