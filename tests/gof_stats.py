"""numpy statistics of dense networks in the layout of the engine's goodness-of-fit records
(include/dynetlsm_hip.h, dlsm_gof_simulate): R = 2 + 3N int64 per time step - edges, mutual,
deg_out[N], deg_in[N], esp[N] - plus the bit (un)packing and the draws' counter scheme, for tests."""
import numpy as np


def records(Y, directed):
    """(T, N, N) 0/1 -> (T, 2 + 3N) int64; shared partners through a float64 product (exact: the
    counts are far below 2^53)"""
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    out = np.zeros((T, 2 + 3 * N), dtype=np.int64)
    up = np.triu(np.ones((N, N), dtype=bool), 1)
    for t in range(T):
        A = Y[t]
        Af = A.astype(np.float64)
        P = np.rint(Af @ Af).astype(np.int64)          # P[i, j] = #m with i -> m -> j
        if directed:
            out[t, 0] = A.sum()
            out[t, 1] = (A & A.T & up).sum()
            out[t, 2:2 + N] = np.bincount(A.sum(1), minlength=N)[:N]
            out[t, 2 + N:2 + 2 * N] = np.bincount(A.sum(0), minlength=N)[:N]
            out[t, 2 + 2 * N:] = np.bincount(P[A], minlength=N)[:N]
        else:
            E = A & up
            out[t, 0] = E.sum()
            out[t, 2:2 + N] = np.bincount(A.sum(1), minlength=N)[:N]
            out[t, 2 + 2 * N:] = np.bincount(P[E], minlength=N)[:N]
    return out


def records_loops(Y, directed):
    """the same by plain loops over the definitions (small networks)"""
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    out = np.zeros((T, 2 + 3 * N), dtype=np.int64)
    for t in range(T):
        A = Y[t]
        for i in range(N):
            dout = sum(int(A[i, j]) for j in range(N))
            din = sum(int(A[j, i]) for j in range(N))
            out[t, 2 + dout] += 1
            if directed:
                out[t, 2 + N + din] += 1
            for j in range(N):
                if not A[i, j] or (not directed and j <= i):
                    continue
                out[t, 0] += 1
                if directed and j > i and A[j, i]:
                    out[t, 1] += 1
                k = sum(1 for m in range(N) if A[i, m] and A[m, j])
                out[t, 2 + 2 * N + k] += 1
    return out


def row_words(N):
    return ((N + 31) // 32 + 3) // 4 * 4


def unpack(bits, N):
    """(..., N, W) uint32 rows -> (..., N, N) bool: bit j % 32 of word j // 32 of row i = Y[i, j]"""
    bits = np.ascontiguousarray(bits, dtype='<u4')
    b = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder='little')
    return b[..., :N].astype(bool)


def probabilities(X, ic, radii, directed):
    """(T, N, N) edge probabilities of one posterior sample: expit(b - d) or the directed model of
    metrics.py; zero diagonal"""
    d = np.sqrt(((X[:, :, None, :] - X[:, None, :, :]) ** 2).sum(-1))
    if directed:
        eta = ic[0] * (1 - d / radii[None, None, :]) + ic[1] * (1 - d / radii[None, :, None])
    else:
        eta = ic[0] - d
    p = 1.0 / (1.0 + np.exp(-eta))
    idx = np.arange(X.shape[1])
    p[:, idx, idx] = 0.0
    return p


def uniforms(philox4x32, seed, index, T, N, directed):
    """(T, N, N) uniforms of the draws at RNG index `index` (kernels_gof.hpp): Philox4x32-10 at counter
    (min(i, j), max(i, j), index, t << 8 | 7); arc i -> j takes the first u53 when i < j (undirected:
    always), the second otherwise; 1 on the diagonal (never an edge)"""
    i, j = np.triu_indices(N, 1)
    U = np.ones((T, N, N))
    for t in range(T):
        r0, r1, r2, r3 = philox4x32(seed, i, j, index, (t << 8) | 7)
        a = u53(r0, r1)
        b = u53(r2, r3)
        U[t, i, j] = a
        U[t, j, i] = b if directed else a
    return U


def u53(hi, lo):
    hi = np.asarray(hi, dtype=np.uint64); lo = np.asarray(lo, dtype=np.uint64)
    k = (hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)
    return (k + 1.0) * (1.0 / 9007199254740992.0)
