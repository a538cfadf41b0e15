"""The systems of tests/test_dense_tiles_gpu.py and their reference: the designed tile patterns of tests/tile_replay.py up to 15
tile columns and full lower triangles, a diagonally dominant random matrix of each pattern, and a Cholesky factor with its
solutions computed column by column in numpy.longdouble.  tests/test_tile_schedule_host.py checks on the CPU that numpy's fp64
factor of every one of them stays under a tenth of L_TOL from the long-double one."""
import functools

import numpy as np

import tile_replay as R

NB = R.NB
FULL_T = (1, 2, 4, 5, 8, 9, 12, 13, 14, 15)
PATTERNS = {k: v for k, v in R.designed_patterns().items() if v.shape[0] <= 15}
PATTERNS.update({"full%d" % T: np.tril(np.ones((T, T), dtype=bool)) for T in FULL_T})
EDGE_PATTERNS, EDGE_SHORT = ["fill6", "meet3", "tree15"], [1, 64, 65]   # n = n_pad - 1, - 64, - 65
INDEFINITE_CASE = ("chain8", 5)


# ---- the reference ----

def longdouble_reference(A, rhs):
    """(L, [x per right-hand side]) of the symmetric positive definite A, column by column in numpy.longdouble"""
    n = A.shape[0]
    Al = A.astype(np.longdouble)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = Al[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    xs = []
    for b in rhs:
        y = b.astype(np.longdouble)
        for j in range(n):
            y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
        for j in range(n - 1, -1, -1):
            y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
        xs.append(y)
    return L, xs


@functools.lru_cache(maxsize=None)
def case(name, n_short=3):
    """the system of a pattern with n = n_pad - n_short, its second right-hand side and its reference; shared, not to be changed"""
    nz = PATTERNS[name]
    n_pad = nz.shape[0] * NB
    n = n_pad - n_short
    A, b = R.random_system(nz, n, seed=11)
    b2 = np.random.default_rng(12).uniform(-1.0, 1.0, n)
    L_ref, (x_ref, x2_ref) = longdouble_reference(A, [b, b2])
    F = R.fill(nz)[0]
    mask = np.kron(F, np.ones((NB, NB), dtype=bool))  # the entries of the filled pattern's tiles
    out = {"nz": nz, "n": n, "n_pad": n_pad, "A": A, "b": b, "b2": b2, "L_ref": L_ref, "x_ref": x_ref, "x2_ref": x2_ref, "F": F,
           "mask": mask, "M": R.padded_matrix(A, b, n_pad)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def all_cases():
    """(pattern, n_pad - n) of every system the GPU tests use"""
    return [(name, 3) for name in PATTERNS] + [(name, n_short) for name in EDGE_PATTERNS for n_short in EDGE_SHORT] + [INDEFINITE_CASE]
