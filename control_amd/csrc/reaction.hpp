// Device re-linearisation of the scalar reaction problem (include/kkt.h,
// kkt_set_reaction_relinearisation): element matrices of a polynomial reaction coefficient,
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
    // the element: nodes per cell (3: P1 triangles, 4: P1 tetrahedra, 6: P2 triangles, 9: Q2
    // quadrilaterals), quadrature points (7: Radon's rule, 15: Stroud's T3:5-1, 25: the 5 x 5
    // conical rule, or the 5 x 5 Gauss-Legendre product rule on Q2) and entries of one
    // element matrix, nv * nv.  d_lam: the nq x nv values of the shape functions at the points
    int nv = 0, nq = 0, ep = 0;
    // n_t == 1: the stationary system [[M, D^T], [D, -(1/beta) M]] of Control.Stationary.  One
    // level of everything, every window [0, 1), tau unused; the element kernels, the gather, the
    // composition and the update run as on one level, the residual rows are their own kernel.
    bool stationary = false;
    // n_t, m, CN, the rank's block rows and the levels of v, zeta and D it holds (levels.hpp): the
    // rows read the same neighbours as RelinPlan's; the data rows are the owned blocks'
    LevelWindows w;
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
    double *d_data = nullptr;   // 2 nl x n1 data rows (the owned rows)
    // CN on a time shard: the neighbours' raw residual rows the time transforms read,
    // [adjoint: block hi | state: block lo - 1], n1 each
    double *d_rhalo = nullptr;
    // work: element matrices (D_n x ne x ep) and D (D_n x nnz) of the last assembly
    double *d_E = nullptr, *d_D = nullptr;
    bool assembled = false;
    double *d_v = nullptr, *d_zeta = nullptr;   // the iterate: v_n x n1 and z_n x n1
    double *d_red = nullptr;                    // reduction scratch + result
    Composer compose;                           // one space: the scalar pattern
};

// E[(s ne + e) ep + nv a + b] of every (element, level of the D window) at the iterate's v,
// s = level - D_l0; the kernel is chosen by the plan's element
void launch_reaction_elements(hipStream_t s, const ReactionPlan &P);
// the owned rows [r0 | r1] of Instationary.non_linear_res_eval, 2 nl x n1
void launch_reaction_residual(hipStream_t s, const ReactionPlan &P, double *d_r);
// the rows [r0 | r1] of Stationary.non_linear_res_eval, 2 x n1 (a stationary plan)
void launch_reaction_stationary_residual(hipStream_t s, const ReactionPlan &P, double *d_r);
// Crank-Nicolson: b = [T_1 r0 | T_2 r1]; across a shard boundary from P.d_rhalo
void launch_reaction_rhs(hipStream_t s, const ReactionPlan &P, const double *d_r, double *d_b);
void launch_reaction_update(hipStream_t s, const ReactionPlan &P, double *d_u);

// host side (reaction.cpp), behind the C-ABI of the same names
void reaction_set(System &S, const kkt_reaction_desc *d);
void reaction_apply(System &T, System &plan, int assemble, int n, const kkt_relin_recipe *rec);
void reaction_state(System &S, int download, double *v, double *zeta);
void reaction_iterate(System &S, double **v, double **zeta);
void reaction_residual(System &S, double *d_out, int rhs, double *norm);
void reaction_update(System &S, double *d_u);
// kkt_debug_reaction_array: E or D of the last assembly (the D window), or the v / zeta window
void reaction_debug_array(System &S, int which, double *out, int64_t cap);
// kkt_reaction_window: [v_l0, v_end, z_l0, z_end, D_l0, D_end, lo, hi), half-open ranges
void reaction_window(System &S, int out[8]);

}  // namespace kkt
