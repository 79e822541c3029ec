"""Extended-precision truth for the reduced camera system S dx = b_s: plain NumPy in numpy.longdouble.

TEST INFRASTRUCTURE ONLY.  Imports nothing from visfs_amd and nothing from the oracle, so that neither implementation can lean on
the other's arithmetic: a solver under test is held to `rel_err_ld(x, truth of ITS OWN system)`, and the criterion every solver form
has to meet is the project's  e_device <= FACTOR * max(e_oracle, FLOOR)  (as accurate on its system as the checker is on its own).

pcg_truth   restates LinearSolverPCG::solve as oracle/visfs_ba_oracle.c (pcg_solve) does: block-Jacobi preconditioner, tolerance 1e-6,
            at most 6 * n_blocks iterations, the absolute floor 0.5 * dn carried from the previous solve.
solve_truth solves the SPD system by a long-double Cholesky with residual refinement.
"""
import numpy as np

LD = np.longdouble
FACTOR, FLOOR = 10.0, 1e-13                     # the project's criterion: e_device <= FACTOR * max(e_oracle, FLOOR)


def rel_err_ld(x, truth):
    """max |x - truth| / max |truth| with the difference taken in long double."""
    x = np.asarray(x, dtype=LD); truth = np.asarray(truth, dtype=LD)
    if truth.size == 0:
        return 0.0
    return float(np.abs(x - truth).max() / max(np.abs(truth).max(), LD(1e-300)))


def within_criterion(e, eo, factor=FACTOR, floor=FLOOR):
    return e <= factor * max(eo, floor)


def block_jacobi_inverses(S, n_blocks):
    """Inverses of the 6x6 diagonal blocks: fp64 inverse, refined by two Newton steps X <- X (2I - A X) in long double."""
    S = np.asarray(S)
    J = np.zeros((n_blocks, 6, 6), dtype=LD)
    I2 = 2 * np.eye(6, dtype=LD)
    for b in range(n_blocks):
        A64 = np.asarray(S[6 * b:6 * b + 6, 6 * b:6 * b + 6], dtype=np.float64)
        A = A64.astype(LD)
        X = np.linalg.inv(A64).astype(LD)
        for _ in range(2):
            X = X @ (I2 - A @ X)
        J[b] = X
    return J


def _precondition(J, r):
    return np.einsum("brc,bc->br", J, r.reshape(-1, 6)).reshape(-1)


def pcg_truth(S, b, n_blocks, floor=-1.0, stop_after=None):
    """(x, iterations, floor_out, floor_was_binding, closest).  `closest` is the smallest |dn / d0 - 1| over all stopping tests:
    how near the input brings the recurrence to one of its own thresholds (a property of the input, judged on the truth).
    stop_after: leave the loop after that many iterations whatever the test says (the sensitivity tests take x one step early)."""
    n = 6 * n_blocks
    S = np.asarray(S, dtype=np.float64).reshape(n, n).astype(LD)
    b = np.asarray(b, dtype=np.float64).reshape(n).astype(LD)
    J = block_jacobi_inverses(S, n_blocks)
    x = np.zeros(n, dtype=LD)
    r = b.copy()
    d = _precondition(J, r)
    dn = r @ d
    d0 = LD(1e-6) * dn
    binding = False
    floor = LD(floor)
    if floor > 0 and floor > d0:
        d0 = floor; binding = True
    closest = np.inf
    it = 0
    while it < n:
        if d0 > 0:
            closest = min(closest, float(abs(dn / d0 - 1)))
        if dn <= d0 or (stop_after is not None and it >= stop_after):
            break
        q = S @ d
        a = dn / (d @ q)
        x = x + a * d
        r = r - a * q
        sv = _precondition(J, r)
        dold = dn
        dn = r @ sv
        d = sv + (dn / dold) * d
        it += 1
    return x, it, float(LD(0.5) * dn), binding, closest


def cholesky_ld(A):
    """Lower Cholesky factor of an SPD matrix in long double (column by column)."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lj = L[j, :j]
        piv = A[j, j] - Lj @ Lj
        if not piv > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(piv)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ Lj) / L[j, j]
    return L


def _chol_solve(L, b):
    n = L.shape[0]
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_truth(S, b):
    """(x, relative residual): the solution of the SPD system in long double.  A long-double Cholesky, then residual refinement in long
    double until the residual stops falling.  Relative residual: |b - S x|_inf / (|S|_inf |x|_inf + |b|_inf)."""
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    b = np.asarray(b, dtype=LD).reshape(n)
    L = cholesky_ld(S)
    x = _chol_solve(L, b)
    res = np.abs(b - S @ x).max()
    for _ in range(8):
        x2 = x + _chol_solve(L, b - S @ x)
        res2 = np.abs(b - S @ x2).max()
        if not res2 < res:
            break
        x, res = x2, res2
    scale = np.abs(S).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return x, float(res / max(scale, LD(1e-300)))
