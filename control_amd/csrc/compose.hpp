// What the device re-linearisation plans share (relin.hpp, reaction.hpp): the checks of a plan's
// arrays, the composition of assembled per-level values D into block values with its
// copy-on-write, and what follows from a rank's level windows (levels.hpp) alike for both: target
// checks, halo exchange, state copies, data uploads, debug copies, residual norms.  DESIGN.md
// section 6.6.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/kkt.h"
#include "devmem.hpp"
#include "levels.hpp"

namespace kkt {

struct System;
struct Pattern;

constexpr int RELIN_NQ = 7;        // Radon's 7-point rule
constexpr int RELIN_EV = 36;       // P2 element matrix entries
constexpr int RELIN_EP = 9;        // P1 element matrix entries

// workgroups of 256 threads over n items, at most cap of them: the rest is grid-stride
static inline int grid_of(int64_t n, int cap) {
    int64_t g = (n + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// One target block of a composition: dst = alpha D(^T) + gamma M on a SELL value array.
struct ComposeJob {
    double *dst;
    const int32_t *sell2csr;   // CSR position of every SELL slot (-1: padding)
    const int32_t *col;        // SELL column of every slot
    const uint8_t *colmask;    // Dirichlet columns zeroed (null: none)
    int64_t npadded;
    const double *D;           // the level's scalar values (CSR of the scalar pattern)
    const double *M;           // scalar mass values
    const int32_t *tperm;      // transpose permutation of the scalar pattern, null: D itself
    int64_t nnz_s;             // scalar nnz: positions of the second component fold onto it
    double alpha, gamma;
};

// What composition needs of one scalar space of a plan.
struct ComposeSpace {
    const char *name = "";                  // in messages: the plan's <name> pattern
    std::vector<int32_t> indptr, indices;   // the scalar pattern, on the host
    int64_t nnz = 0;
    int ncomp = 1;   // a block holds the pattern once per component (1 or 2), component-major
    const double *d_D = nullptr;   // D_n levels of nnz values, from level D_l0
    int D_l0 = 0, D_n = 0;
    const double *d_M = nullptr;
    const int32_t *d_tperm = nullptr;
};

// The composing side of a plan: its spaces (a recipe's `space` indexes them), the job table and
// the target patterns already proven equal to a space's.
struct Composer {
    int n_t = 0;   // global time levels: the range of a recipe's level
    std::vector<ComposeSpace> spaces;
    DevBuf<ComposeJob> d_jobs;   // regrown with the largest job count seen
    int jobs_cap = 0;
    std::set<std::tuple<const void *, int, int>> checked;   // (system, pattern id, space)
};

// Host-only checks (plan_checks.cpp: nothing of HIP).  Each fails with KKT_ERR_ARG and a message
// that begins with `what`, the API entry and the array: a sorted CSR of nrows x ncols; lists that
// hold each of n_entries element entries once, ascending per stored position; t[t[k]] == k; n
// indices below bound.
void check_csr(const std::string &what, const int32_t *ip, const int32_t *ix, int64_t nrows,
               int64_t ncols, int64_t nnz);
void check_lists(const std::string &what, const int32_t *cptr, const int32_t *clist, int64_t nnz,
                 int64_t n_entries);
void check_perm(const std::string &what, const int32_t *t, int64_t nnz);
void check_range(const std::string &what, const int32_t *idx, int64_t n, int64_t bound);
// Q is sp's pattern once per component: component c in the rows and columns from c n, the
// positions from c nnz
bool pattern_is_space(const Pattern &Q, const ComposeSpace &sp);

// one pattern: D[l nnz + k] = nu K[k] + the contributions of position k in list order (n_t levels
// of E, per_level doubles each)
void launch_relin_gather_one(hipStream_t s, const int32_t *cptr, const int32_t *clist,
                             const double *E, int64_t per_level, const double *K, double nu,
                             int64_t nnz, int n_t, double *D);
void launch_relin_compose(hipStream_t s, const ComposeJob *d_jobs, int njobs, int64_t max_padded);

// Every recipe validated against the target T and the plan's spaces, nothing written: a job per
// recipe, dst and colmask still open.  `api`: the entry called, first in every message.
std::vector<ComposeJob> compose_jobs(const char *api, System &T, Composer &C, int n,
                                     const kkt_relin_recipe *rec);
// Value arrays shared with another block made private, the jobs uploaded and run on T's stream,
// the host waiting; the blocks are set and T's preconditioner stale.
void compose_run(System &T, Composer &C, std::vector<ComposeJob> &jobs,
                 const kkt_relin_recipe *rec);

// The head of a plan's *_apply, each a KKT_ERR_ARG that begins with `api`: the recipe list, the
// device, a finalized target, and a target sharded like the plan's handle PS.
void check_apply_target(const char *api, const System &T, const System &PS, int n,
                        const kkt_relin_recipe *rec);

// One level of v up and one of zeta down, after the update and before the assembly: v of my last
// block is the first level of the window above, zeta of my first block the last of the window
// below.  Levels (row_len doubles) are contiguous: nothing is packed.  One rank: nothing.
void exchange_iterate_halos(System &S, const LevelWindows &w, double *d_v, double *d_zeta,
                            int64_t row_len);

// Host <-> device copies on a stream, then a wait; a null host pointer skips its span.
struct CopySpan {
    double *dev, *host;
    int64_t len;
};
void copy_spans(hipStream_t s, bool download, const std::vector<CopySpan> &spans);
// v and zeta between host arrays of the global shapes and a rank's windows: an upload reads the
// windows, a download writes the owned levels (levels.hpp) and leaves the rest as it is
std::vector<CopySpan> iterate_spans(const LevelWindows &w, bool download, double *d_v,
                                    double *d_zeta, double *v, double *zeta, int64_t row_len);

// n bytes, 1 on the n_bc Dirichlet dofs; and the data rows of the owned blocks, lo..hi-1 of the
// adjoint rows and m+lo..m+hi-1 of the state rows of `data` (2 m rows of row_len)
uint8_t *upload_bc_mask(DevPool &mem, const int32_t *bc_idx, int64_t n_bc, int64_t n);
double *upload_data_rows(DevPool &mem, const LevelWindows &w, const double *data, int64_t row_len);

// One array a plan's debug entry copies to the host: `levels` levels of per_level doubles;
// needs_assembly: work of the last assembly, refused before the first
struct DebugArray {
    const double *src;
    int64_t per_level;
    int levels;
    bool needs_assembly;
};
void copy_debug_array(const char *api, System &S, const std::vector<DebugArray> &arrays,
                      bool assembled, int which, double *out, int64_t cap);

// S's scratch vector for the raw residual rows a right-hand side is transformed from
double *raw_rows(System &S);
// ||r|| over S's local rows into d_red[0] on S's stream (d_red: REDUCE_BLOCKS * MDOT_MAX + 2
// doubles; a time shard sums over its ranks: the same norm on each), and read back after what the
// caller enqueued behind it (a right-hand side)
void launch_residual_norm(System &S, const double *r, double *d_red);
void read_residual_norm(System &S, const double *d_red, double *norm);

}  // namespace kkt
