"""numpy replica of the missing-dyad imputation step (csrc/kernels_missing.hpp), for tests: the draws'
counter scheme, the probabilities, and the step applied to a dense network."""
import numpy as np

from gof_stats import u53

STREAM_MISSING = 8


def uniforms(philox4x32, seed, chain, it, index, directed):
    """the uniform of every (t, i, j) row of `index`: Philox4x32-10 at counter (min(i, j) | (t & 255) << 24,
    max(i, j) | (t >> 8) << 24, it, chain << 8 | 8); an undirected dyad takes the first u53, the arc
    i -> j the first when i < j and the second otherwise"""
    index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
    t, i, j = index[:, 0], index[:, 1], index[:, 2]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    r0, r1, r2, r3 = philox4x32(seed, lo | ((t & 255) << 24), hi | ((t >> 8) << 24), it,
                                (chain << 8) | STREAM_MISSING)
    a, b = u53(r0, r1), u53(r2, r3)
    return np.where(i > j, b, a) if directed else a


def probabilities(X, ic, radii, index, directed):
    """p of every (t, i, j) row of `index` at positions X (T, N, D): expit(b - d), or the directed model
    b_in (1 - d / r_j) + b_out (1 - d / r_i)"""
    index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
    t, i, j = index[:, 0], index[:, 1], index[:, 2]
    df = X[t, i] - X[t, j]
    d = np.sqrt((df * df).sum(-1))
    ic = np.ravel(ic)
    if directed:
        eta = ic[0] * (1 - d / radii[j]) + ic[1] * (1 - d / radii[i])
    else:
        eta = ic[0] - d
    return 1.0 / (1.0 + np.exp(-eta))


def step(philox4x32, Y, X, ic, radii, index, seed, chain, it, directed):
    """one imputation step on the dense 0/1 network Y (T, N, N), in place; returns (draws, p, u)"""
    index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
    p = probabilities(X, ic, radii, index, directed)
    u = uniforms(philox4x32, seed, chain, it, index, directed)
    y = u < p
    t, i, j = index[:, 0], index[:, 1], index[:, 2]
    Y[t, i, j] = y
    if not directed:
        Y[t, j, i] = y
    return y, p, u
