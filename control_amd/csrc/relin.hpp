// Device re-linearisation of the Picard loop (include/kkt.h, kkt_set_relinearisation):
// convection assembly of the Taylor-Hood discretisation into block values, the non-linear
// residual and the update of the iterate.  DESIGN.md section 6.6.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/kkt.h"
#include "compose.hpp"
#include "devmem.hpp"

namespace kkt {

struct System;

struct RelinPlan {
    // n_t, m, CN, the rank's block rows and the levels of v, zeta and D it holds (levels.hpp); p,
    // mu and the data rows are the owned blocks'
    LevelWindows w;
    // n_t == 1: the stationary system of Control.Stationary.incompressible_non_linear_solve,
    // outer blocks [[M, D^T], [D, -(1/beta) M]] with B / B^T.  One level, every window [0, 1),
    // tau unused; its velocity rows are not backward Euler's (launch_relin_stationary_residual)
    bool stationary = false;
    int64_t ne = 0, n2 = 0, n1 = 0, nv = 0, nnz2 = 0, nnz1 = 0;
    double nu = 0.0, tau = 0.0, beta = 0.0;
    // the element: nodes per cell of the velocity (6: P2 triangles, 9: Q2 quadrilaterals) and of
    // the pressure, quadrature points, and the entries of the two element matrices
    int kv = 6, kp = 3, nq = RELIN_NQ, ev = RELIN_EV, ep = RELIN_EP;
    DevPool mem;   // everything below but the job table
    int32_t *d_V = nullptr;
    double *d_W = nullptr, *d_phi = nullptr, *d_gphi = nullptr, *d_lam = nullptr,
           *d_glam = nullptr;
    double *d_jinv = nullptr;   // Q2-Q1: ne x 2, and gphi / glam are the reference tables
    // scalar P2 pattern (one velocity component) and P1 pattern
    int32_t *d_ip2 = nullptr, *d_ix2 = nullptr, *d_t2 = nullptr, *d_tp = nullptr;
    double *d_K2 = nullptr, *d_M2 = nullptr, *d_Kp = nullptr, *d_Mp = nullptr;
    // contribution lists: CSR over stored positions of flat element-entry indices, ascending
    int32_t *d_cptr2 = nullptr, *d_clist2 = nullptr, *d_cptrp = nullptr, *d_clistp = nullptr;
    // B (n1 x nv) and B^T (nv x n1)
    int32_t *d_Bip = nullptr, *d_Bix = nullptr, *d_BTip = nullptr, *d_BTix = nullptr;
    double *d_Bv = nullptr, *d_BTv = nullptr;
    uint8_t *d_bc = nullptr;   // nv bytes: Dirichlet velocity dofs
    double *d_data = nullptr;  // 2 nl x nv data rows of the velocity residual (the owned rows)
    // CN on a time shard: the neighbours' raw residual rows the time transforms read, velocity
    // [adjoint: block hi | state: block lo - 1] (nv each), pressure [v: lo - 1 | zeta: hi] (n1)
    double *d_rhalo = nullptr;
    // work: element matrices and the assembled D per level of the D window
    double *d_Ev = nullptr, *d_Ep = nullptr, *d_D2 = nullptr, *d_Dp = nullptr;
    bool assembled = false;
    // the iterate: v (v_n x nv), zeta (z_n x nv), p, mu (nl x n1)
    double *d_v = nullptr, *d_zeta = nullptr, *d_p = nullptr, *d_mu = nullptr;
    double *d_red = nullptr;   // reduction scratch + result
    Composer compose;   // spaces: velocity (two components of the P2 pattern), pressure
};

// element matrices of every (element, level of the D window): Ev[(s ne + e) 36 + 6a + b],
// Ep[... 9 + 3c + d] (Q2-Q1: ... 81 + 9a + b, ... 16 + 4c + d), s = level - D_l0; d_v: the plan's
// v window.  Dispatches on the plan's element (kv).
void launch_relin_elements(hipStream_t s, const RelinPlan &P, const double *d_v);
// D[l nnz + k] = nu K[k] + sum of the contributions of position k in list order
void launch_relin_gather(hipStream_t s, const RelinPlan &P);
// velocity and pressure rows of the residual in the outer system's vector layout
void launch_relin_residual(hipStream_t s, const RelinPlan &P, double *d_r);
// the rows [r00 | r01 | r10 | r11] of Stationary.incompressible_non_linear_solve's evaluate(), a
// stationary plan's; they are the solve's right-hand side as they are
void launch_relin_stationary_residual(hipStream_t s, const RelinPlan &P, double *d_r);
// the solve's right-hand side from the residual: pressure rows times tau, CN time transforms
void launch_relin_rhs(hipStream_t s, const RelinPlan &P, const double *d_r, double *d_b);
// v, zeta, mu, p += the update's blocks, the update zeroed; zeta zero on the Dirichlet dofs
void launch_relin_update(hipStream_t s, const RelinPlan &P, double *d_u);

// host side (relin.cpp), behind the C-ABI of the same names
void relin_set(System &S, const kkt_relin_desc *d);
void relin_apply(System &T, System &plan, const double *d_v, int n, const kkt_relin_recipe *rec);
void relin_state(System &S, int download, double *v, double *zeta, double *p, double *mu);
void relin_iterate(System &S, double **v, double **zeta, double **p, double **mu);
void relin_residual(System &S, double *d_out, int rhs, double *norm);
void relin_update(System &S, double *d_u);
// kkt_debug_relin_array: Ev, Ep, D2 or Dp of the last assembly (the D window), or the v / zeta
// window of the iterate, copied to the host
void relin_debug_array(System &S, int which, double *out, int64_t cap);
// kkt_picard_window: [v_l0, v_end, z_l0, z_end, D_l0, D_end, lo, hi), half-open ranges
void relin_window(System &S, int out[8]);

}  // namespace kkt
