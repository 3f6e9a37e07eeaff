// Device re-linearisation of the scalar reaction problem (include/kkt.h,
// kkt_set_reaction_relinearisation): P1 element matrices of a polynomial reaction coefficient,
// their gather and composition into block values (compose.hpp), the Picard residual and the
// update of the iterate.  DESIGN.md section 6.6a.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/kkt.h"
#include "compose.hpp"
#include "devmem.hpp"

namespace kkt {

struct System;

constexpr int REACTION_MAX_DEGREE = 4;

struct ReactionCoef {
    int degree;
    double c[REACTION_MAX_DEGREE + 1];
};

struct ReactionPlan {
    int n_t = 0, m = 0;   // time levels, unknown blocks per family
    // the element: nodes per cell (3: triangles, 4: tetrahedra), quadrature points (7: Radon's
    // rule, 15: Stroud's T3:5-1) and entries of one element matrix, nv * nv
    int nv = 0, nq = 0, ep = 0;
    bool CN = false;
    int64_t ne = 0, n1 = 0, nnz = 0;
    double tau = 0.0, beta = 0.0;
    ReactionCoef coef{};
    DevPool mem;   // everything below but the job table
    int32_t *d_cells = nullptr;
    double *d_W = nullptr, *d_lam = nullptr;
    int32_t *d_ip = nullptr, *d_ix = nullptr, *d_tperm = nullptr, *d_cptr = nullptr,
            *d_clist = nullptr;
    double *d_L = nullptr, *d_M = nullptr;
    uint8_t *d_bc = nullptr;    // n1 bytes: Dirichlet dofs
    double *d_data = nullptr;   // 2m x n1 data rows
    // work: element matrices (n_t x ne x ep) and D (n_t x nnz) of the last assembly
    double *d_E = nullptr, *d_D = nullptr;
    bool assembled = false;
    double *d_v = nullptr, *d_zeta = nullptr;   // the iterate, n_t x n1 each
    double *d_red = nullptr;                    // reduction scratch + result
    Composer compose;                           // one space: the scalar pattern
};

// E[(l ne + e) ep + nv a + b] of every (element, level) at the iterate's v; the kernel is chosen
// by the plan's element
void launch_reaction_elements(hipStream_t s, const ReactionPlan &P);
// rows [r0 | r1] of Instationary.non_linear_res_eval, 2m x n1
void launch_reaction_residual(hipStream_t s, const ReactionPlan &P, double *d_r);
// Crank-Nicolson: b = [T_1 r0 | T_2 r1]
void launch_reaction_rhs(hipStream_t s, const ReactionPlan &P, const double *d_r, double *d_b);
void launch_reaction_update(hipStream_t s, const ReactionPlan &P, double *d_u);

// host side (reaction.cpp), behind the C-ABI of the same names
void reaction_set(System &S, const kkt_reaction_desc *d);
void reaction_apply(System &T, System &plan, int assemble, int n, const kkt_relin_recipe *rec);
void reaction_state(System &S, int download, double *v, double *zeta);
void reaction_iterate(System &S, double **v, double **zeta);
void reaction_residual(System &S, double *d_out, int rhs, double *norm);
void reaction_update(System &S, double *d_u);
void reaction_debug_array(System &S, int which, double *out, int64_t cap);

}  // namespace kkt
