"""Stand-in for python-control (golden-vector generation only): the one function
lqr_controller_world_frame.py:129 calls."""
import numpy as np
from scipy.linalg import solve_continuous_are


def lqr(A, B, Q, R):
    """(K, S, E) of the continuous-time LQR: S solves the algebraic Riccati equation, K = R^-1 B^T S,
    E = eig(A - B K)."""
    A, B, Q, R = (np.atleast_2d(np.asarray(m, np.float64)) for m in (A, B, Q, R))
    S = solve_continuous_are(A, B, Q, R)
    K = np.linalg.solve(R, B.T @ S)
    return K, S, np.linalg.eigvals(A - B @ K)
