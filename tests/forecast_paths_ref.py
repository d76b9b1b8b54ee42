"""numpy replica of the multi-step forecast draws (csrc/kernels_forecast_paths.hpp), for tests: the counter
layout, the label rule and the laws of the positions, plus the mean edge probability of given paths.

Randoms of (node i, step h = 1..H, RNG index q): Philox4x32-10 keyed by the seed at counter
(i, h | draw << 16, q, 9).  draw 0: the first u53 is the label uniform; draw 1 + d // 2: the two uniforms of
the Box-Muller pair of coordinates d, d + 1."""
import numpy as np

from gof_stats import u53

STREAM_FORECAST = 9
TWO_PI = 6.283185307179586476925286766559


def counter(i, h, draw, index):
    """the four counter words of a draw"""
    return i, h | (draw << 16), index, STREAM_FORECAST


def label_uniforms(philox4x32, seed, index, h, N):
    r0, r1, _, _ = philox4x32(seed, *counter(np.arange(N), h, 0, index))
    return u53(r0, r1)


def normals(philox4x32, seed, index, h, N, D):
    """(N, D) standard normals of step h"""
    eps = np.empty((N, D))
    for d in range(0, D, 2):
        r0, r1, r2, r3 = philox4x32(seed, *counter(np.arange(N), h, 1 + d // 2, index))
        u0, u1 = u53(r0, r1), u53(r2, r3)
        r = np.sqrt(-2.0 * np.log(u0))
        a = TWO_PI * u1
        eps[:, d] = r * np.cos(a)
        if d + 1 < D:
            eps[:, d + 1] = r * np.sin(a)
    return eps


def draw_labels(u, rows):
    """smallest k with u * c_{K-1} <= c_k, c the running sum of the raw row in index order (sequential double
    adds: np.cumsum of a 1-d float64 row adds in index order), capped at K - 1; rows (N, K)"""
    c = np.cumsum(rows, axis=1)
    thr = u * c[:, -1]
    hit = thr[:, None] <= c
    return np.where(hit.any(axis=1), hit.argmax(axis=1), rows.shape[1] - 1).astype(np.int32)


def paths(philox4x32, seed, first_index, X0, H, sigma_sq=None, z0=None, trans=None, mu=None, sigma=None, lmbda=None):
    """(S, H, N, D) positions and (S, H, N) int32 labels (None for the random walk) of the trajectories
    started at X0 (S, N, D); sample s uses RNG index first_index + s"""
    S, N, D = X0.shape
    P = np.empty((S, H, N, D))
    mixture = z0 is not None
    L = np.empty((S, H, N), dtype=np.int32) if mixture else None
    for s in range(S):
        x = np.array(X0[s], dtype=np.float64)
        z = np.array(z0[s], dtype=np.int64) if mixture else None
        for h in range(1, H + 1):
            eps = normals(philox4x32, seed, first_index + s, h, N, D)
            if mixture:
                u = label_uniforms(philox4x32, seed, first_index + s, h, N)
                z = draw_labels(u, trans[s][z]).astype(np.int64)
                x = lmbda[s] * mu[s][z] + (1.0 - lmbda[s]) * x + np.sqrt(sigma[s][z])[:, None] * eps
                L[s, h - 1] = z
            else:
                x = x + np.sqrt(sigma_sq) * eps
            P[s, h - 1] = x
    return P, L


def mean_probas(P, ic, radii=None):
    """(H, N, N): mean over the samples of expit(eta) at the paths P (S, H, N, D); ic (S, 2); radii (S, N) for
    the directed model eta = b_in (1 - d / r_j) + b_out (1 - d / r_i), else eta = b - d; zero diagonal"""
    S, H, N, _ = P.shape
    out = np.zeros((H, N, N))
    for s in range(S):
        d = np.sqrt(((P[s][:, :, None, :] - P[s][:, None, :, :]) ** 2).sum(-1))
        if radii is not None:
            eta = ic[s, 0] * (1 - d / radii[s][None, None, :]) + ic[s, 1] * (1 - d / radii[s][None, :, None])
        else:
            eta = ic[s, 0] - d
        out += 1.0 / (1.0 + np.exp(-eta))
    out /= S
    idx = np.arange(N)
    out[:, idx, idx] = 0.0
    return out
