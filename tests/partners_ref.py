"""Host restatement of the per-node link prediction (numpy): for every ordered pair (i, j), i != j, the posterior-mean
edge probability and the standard deviation of p_s of topk_ref.values (undirected models: symmetrised, the value of
{i, j} in both rows), which partners of a row are eligible under ``among``, and per (t, i) all eligible partners j
ranked by a stable sort on (-pbar, j) - (pbar, j) unless ``largest``.  Written independently of dynetlsm_amd/ranking.py
and csrc/kernels_partners.hpp; dense (S, T, N, N) arrays, for the small shapes of the tests."""
import numpy as np

import proba_ref
import topk_ref

AMONG = topk_ref.AMONG


def values(Xs, ic, radii, directed):
    """topk_ref.values with every ordered pair filled: 'exists' (T, N, N) is i != j, and an undirected model has
    the (pbar, sd) of {i, j} at (i, j) and at (j, i)"""
    base = topk_ref.values(Xs, ic, radii, directed)
    T, N = base['exists'].shape[:2]
    out = {'exists': np.broadcast_to(~np.eye(N, dtype=bool), (T, N, N))}
    for key in ('pw', 'pw_ld', 'pw_pt'):
        out[key] = base[key] if directed else base[key] + base[key].transpose(0, 2, 1, 3)    # zero where i >= j
    return out


def eligible_partners(Y, directed, among, mask=None):
    """(T, N, N) boolean per ordered pair (i, j): j is an eligible partner of i.  An undirected model reads the tie
    and the mask of {i, j} at (min, max) and either orientation of the mask excludes the dyad."""
    Y = np.asarray(Y) != 0
    T, N = Y.shape[:2]
    exists = np.broadcast_to(~np.eye(N, dtype=bool), (T, N, N))
    m = np.zeros((T, N, N), dtype=bool) if mask is None else np.asarray(mask) != 0
    if not directed:
        up = np.triu(np.ones((N, N), dtype=bool), 1)
        Y = Y & up
        Y = Y | Y.transpose(0, 2, 1)
        m = m | m.transpose(0, 2, 1)
    observed = exists & ~m
    return Y, {'non_ties': observed & ~Y, 'ties': observed & Y, 'observed': observed, 'missing': exists & m,
               'all': exists.copy()}[among]


def reference(Y, Xs, ic, radii, directed, among, largest, mask=None, base=None):
    """Everything the tests compare: ``values`` (``base``, if it has been computed for these samples); 'Y' (T, N, N)
    the tie that row i reads for partner j; 'eligible' (T, N, N); 'rank': [t][i] the eligible partners of the row in
    rank order; 'eligible_n' (T, N)"""
    out = dict(values(Xs, ic, radii, directed) if base is None else base)
    out['Y'], out['eligible'] = eligible_partners(Y, directed, among, mask)
    T, N = out['eligible'].shape[:2]
    rank = []
    for t in range(T):
        rows = []
        for i in range(N):
            j = np.nonzero(out['eligible'][t, i])[0]                  # ascending
            v = out['pw'][t, i, j, 0]
            rows.append(j[np.argsort(-v if largest else v, kind='stable')])
        rank.append(rows)
    out['rank'] = rank
    out['eligible_n'] = out['eligible'].sum(axis=2)
    return out


def tolerances(ref):
    """((T, N, N) tolerance of pbar, of sd): proba_ref.tolerance, 16 eps + 4 ulp of the value with eps the
    reference's own error on this input"""
    return proba_ref.tolerance(ref, 0)[0], proba_ref.tolerance(ref, 1)[0]


def row_cut_is_decided(ref, t, i, k, tol):
    """topk_ref.cut_is_decided for the row (t, i): the first k partners are the same set for every ranking within
    ``tol`` (T, N, N) of the reference's values - the k-th and the (k + 1)-th value differ by more than twice the
    tolerance, or they lie in a group of bit-equal values whose neighbours on both sides are that far away (the group
    is then cut by j).  True as well when k takes every eligible partner."""
    j = ref['rank'][t][i]
    n = j.size
    if k >= n:
        return True
    v = ref['pw'][t, i, j, 0]
    w = 2.0 * tol[t, i, j]

    def apart(a, b):                  # positions a, b = a + 1 of the ranking
        return abs(v[a] - v[b]) > max(w[a], w[b])

    if apart(k - 1, k):
        return True
    if v[k - 1] != v[k]:
        return False
    lo = k - 1
    while lo > 0 and v[lo - 1] == v[k]:
        lo -= 1
    hi = k
    while hi + 1 < n and v[hi + 1] == v[k]:
        hi += 1
    return (lo == 0 or apart(lo - 1, lo)) and (hi == n - 1 or apart(hi, hi + 1))
