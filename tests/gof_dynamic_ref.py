"""numpy replica of the engine's goodness-of-fit records over time (include/dynetlsm_hip.h,
dlsm_gof_dynamic_simulate) from boolean (T, N, N) networks, for tests: overlap (T, T), steps
(T - 1, 2N) - persist_degree[N], formed_sp[N] - and geodesic (T, N), all int64.  A dyad is an
unordered pair i < j (undirected) or an arc i -> j (directed)."""
import numpy as np


def _dyads(N, directed):
    return ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)


def overlap(Y, directed):
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    E = Y & _dyads(N, directed)
    return np.array([[(E[t] & E[u]).sum() for u in range(T)] for t in range(T)], dtype=np.int64)


def steps(Y, directed):
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    out = np.zeros((max(T - 1, 0), 2 * N), dtype=np.int64)
    dy = _dyads(N, directed)
    for t in range(T - 1):
        A, B = Y[t], Y[t + 1]
        out[t, :N] = np.bincount((A & B).sum(1), minlength=N)[:N]
        Af = A.astype(np.float64)
        P = np.rint(Af @ Af).astype(np.int64)          # P[i, j] = #m with i -> m -> j at t
        out[t, N:] = np.bincount(P[B & ~A & dy], minlength=N)[:N]
    return out


def distances(A):
    """(N, N) int64 shortest-path lengths along the arcs of boolean A by levels of boolean matrix
    products; 0 on the diagonal and where there is no path"""
    N = A.shape[0]
    Af = A.astype(np.float32)
    dist = np.zeros((N, N), dtype=np.int64)
    visited = np.eye(N, dtype=bool)
    frontier = visited.copy()
    for level in range(1, N):
        frontier = ((frontier.astype(np.float32) @ Af) > 0) & ~visited
        if not frontier.any():
            break
        dist[frontier] = level
        visited |= frontier
    return dist


def geodesic(Y, directed):
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    out = np.zeros((T, N), dtype=np.int64)
    dy = _dyads(N, directed)
    for t in range(T):
        out[t] = np.bincount(distances(Y[t])[dy], minlength=N)[:N]
    return out


def records(Y, directed):
    return overlap(Y, directed), steps(Y, directed), geodesic(Y, directed)


def records_loops(Y, directed):
    """the same by plain loops over the definitions (small networks)"""
    Y = np.asarray(Y) != 0
    T, N, _ = Y.shape
    pairs = [(i, j) for i in range(N) for j in range(N) if (i != j if directed else i < j)]
    ov = np.zeros((T, T), dtype=np.int64)
    st = np.zeros((max(T - 1, 0), 2 * N), dtype=np.int64)
    geo = np.zeros((T, N), dtype=np.int64)
    for t in range(T):
        for u in range(T):
            ov[t, u] = sum(1 for i, j in pairs if Y[t, i, j] and Y[u, i, j])
    for t in range(T - 1):
        A, B = Y[t], Y[t + 1]
        for i in range(N):
            st[t, sum(1 for j in range(N) if A[i, j] and B[i, j])] += 1
        for i, j in pairs:
            if B[i, j] and not A[i, j]:
                st[t, N + sum(1 for m in range(N) if A[i, m] and A[m, j])] += 1
    for t in range(T):
        A = Y[t]
        for s in range(N):
            dist = {s: 0}
            queue = [s]
            while queue:
                v = queue.pop(0)
                for m in range(N):
                    if A[v, m] and m not in dist:
                        dist[m] = dist[v] + 1
                        queue.append(m)
            for j in range(N):
                if j != s and (directed or j > s):
                    geo[t, dist.get(j, 0)] += 1
    return ov, st, geo
