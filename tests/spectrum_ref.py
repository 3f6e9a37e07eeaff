"""Dense references for the Chebyshev intervals of the built-in preconditioner's sub-solves.

``schur_solve_map`` lists, in the order the preconditioner emits them, the Schur sub-solves of
one application with the block and shift of their matrix ``blk + c M`` (``pc_stationary`` /
``pc_instationary_BE`` / ``pc_instationary_CN`` of the oracle); ``jacobi_spectra`` solves the
Jacobi-scaled matrix densely on the interior dofs.
"""
import numpy as np
import scipy.sparse as sp


def schur_solve_map(kind, blocks, n, tau, beta, epsilon=1.0e-3):
    """[(sweep, level, block, c)] of one application, emission order.  ``n``: blocks per
    variable (BE: n_t, CN: n_t - 1, stationary: 1)."""
    _, b01, b10, _ = blocks
    if kind == "stationary":
        c = 1.0 / beta**0.5
        return [("first", 0, b10[(0, 0)], c), ("second", 0, b01[(0, 0)], c)]
    if kind == "BE":
        shift = tau / beta**0.5

        def coef(i):
            return 0.0 if i == 0 else ((epsilon**0.5) * shift if i == n - 1 else shift)
    elif kind == "CN":
        my_const = 0.5 * tau / beta**0.5

        def coef(i):
            return my_const
    else:
        raise ValueError(kind)
    out = [("forward", i, b10[(i, i)], coef(i)) for i in range(n)]
    out += [("backward", i, b01[(i, i)], coef(i)) for i in range(n - 1, -1, -1)]
    return out


def assembled(blk, c, M, nodes):
    """``assemble_with_bcs(blk + c M)`` as the oracle forms it."""
    from oracle import kkt_oracle as ko
    return ko.assemble_with_bcs(blk if c == 0.0 else blk + c * M, nodes)


def value_key(blk, c):
    """Identity of the values of ``blk + c M`` (same M): the shift's bits and the block's entries."""
    B = sp.csr_matrix(blk, copy=True)
    B.sum_duplicates()
    B.eliminate_zeros()
    B.sort_indices()
    return (np.float64(c).tobytes(), B.shape, B.indptr.tobytes(), B.indices.tobytes(),
            B.data.tobytes())


def distinct_solved_matrices(p, epsilon=1.0e-3):
    """Number of distinct value sets among the matrices the sub-solves of the heat-type problem
    ``p`` (``control_amd.problems.heat_problem``) solve with."""
    kind = "CN" if p["CN"] else "BE"
    M, nodes = p["sd"].M, p["nodes"]
    return len({value_key(assembled(blk, c, M, nodes), c)
                for _, _, blk, c in schur_solve_map(kind, p["blocks"], p["m"], p["tau"], p["beta"],
                                                    epsilon)})


def jacobi_spectra(A, nodes, nonsym_eigs=True):
    """Of ``A`` (bc-assembled) restricted to the interior dofs, D = diag(A):
    ``lmin`` / ``lmax`` of D^-1/2 (A + A^T)/2 D^-1/2, ``rho_skew`` of D^-1/2 (A - A^T)/2 D^-1/2,
    ``symmetric`` (A == A^T exactly) and, for non-symmetric A, the eigenvalues ``ev`` of D^-1 A."""
    keep = np.setdiff1d(np.arange(A.shape[0]), np.asarray(nodes))
    Ai = sp.csr_matrix(A)[keep][:, keep].toarray()
    d = np.diag(Ai).copy()
    s = 1.0 / np.sqrt(d)
    H = 0.5 * (Ai + Ai.T)
    S = 0.5 * (Ai - Ai.T)
    lam = np.linalg.eigvalsh(s[:, None] * H * s[None, :])
    out = dict(lmin=float(lam[0]), lmax=float(lam[-1]), symmetric=not S.any(), n=len(keep))
    if out["symmetric"]:
        out["rho_skew"] = 0.0
        out["ev"] = None
    else:
        mu = np.linalg.eigvalsh(1j * (s[:, None] * S * s[None, :]))
        out["rho_skew"] = float(np.max(np.abs(mu)))
        out["ev"] = np.linalg.eigvals(Ai / d[:, None]) if nonsym_eigs else None
    return out


def neumann_spectrum(K):
    """Smallest non-zero and largest eigenvalue of D^-1/2 K D^-1/2 (K singular: constants)."""
    Kd = sp.csr_matrix(K).toarray()
    s = 1.0 / np.sqrt(np.diag(Kd))
    lam = np.linalg.eigvalsh(s[:, None] * Kd * s[None, :])
    tol = 1e-10 * lam[-1]
    assert abs(lam[0]) < tol < lam[1], "expected exactly one zero eigenvalue"
    return float(lam[1]), float(lam[-1])
