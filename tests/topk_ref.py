"""Host restatement of the link prediction (numpy): the posterior-mean edge probability pbar of every dyad
(score_ref.posterior_mean_proba) and the standard deviation of p_s (proba_ref.summaries) in float64, in np.longdouble
and on probabilities moved by +-4 ulp, which dyads are eligible under ``among``, and per time step all eligible dyads
ranked by a stable sort on (-pbar, i, j) - (pbar, i, j) unless ``largest``.  Written independently of
dynetlsm_amd/ranking.py and csrc/kernels_topk.hpp; dense (S, T, N, N) arrays, for the small shapes of the tests."""
import numpy as np

import proba_ref
import score_ref

AMONG = ('non_ties', 'ties', 'observed', 'missing', 'all')


def eligible_dyads(Y, directed, among, mask=None):
    """(T, N, N) boolean: the dyads of the model (undirected: i < j) that the ranking chooses from"""
    Y = np.asarray(Y)
    T, N = Y.shape[:2]
    exists = np.broadcast_to(score_ref.dyad_mask(N, directed), (T, N, N))
    observed = score_ref.scored_dyads(T, N, directed, mask)          # undirected: either orientation masks
    tie = Y != 0
    return {'non_ties': observed & ~tie, 'ties': observed & tie, 'observed': observed,
            'missing': exists & ~observed, 'all': exists.copy()}[among]


def ranked(values, eligible, largest):
    """per time step (i, j) of all eligible dyads, ranked: a stable sort by the value (descending if ``largest``)
    of the dyads in (i, j) order"""
    out = []
    for t in range(eligible.shape[0]):
        i, j = np.nonzero(eligible[t])                                # row-major: (i, j) ascending
        v = values[t][i, j]
        order = np.argsort(-v if largest else v, kind='stable')
        out.append((i[order], j[order]))
    return out


def values(Xs, ic, radii, directed):
    """'exists' (T, N, N) boolean and 'pw', 'pw_ld', 'pw_pt' (T, N, N, 2) = (pbar, sd) of every dyad in float64,
    longdouble and on the perturbed probabilities (what proba_ref.tolerance reads), zero where no dyad is: the part
    of the reference that does not depend on the network, ``among`` or ``largest``"""
    eta = score_ref.linear_predictor(Xs, ic, radii, directed)
    S, T, N = eta.shape[:3]
    exists = np.broadcast_to(score_ref.dyad_mask(N, directed), (T, N, N))
    out = {'exists': exists}
    p64 = proba_ref.expit(eta)
    pld = proba_ref.expit(score_ref.linear_predictor(Xs, ic, radii, directed, np.longdouble))
    for key, p in (('pw', p64), ('pw_ld', pld), ('pw_pt', proba_ref.perturbed(p64))):
        pbar = score_ref.posterior_mean_proba(eta) if key == 'pw' else p.sum(axis=0) / S
        pw = np.stack([pbar, proba_ref.summaries(p, 0.9)[1]], axis=-1)
        out[key] = np.where(exists[..., None], pw, p.dtype.type(0))
    return out


def reference(Y, Xs, ic, radii, directed, among, largest, mask=None, base=None):
    """Everything the tests compare: ``values`` (``base``, if it has been computed for these samples) and 'eligible'
    (T, N, N) boolean; 'Y' the ties; 'rank': per time step (i, j) of every eligible dyad in rank order;
    'eligible_t' (T,)"""
    out = dict(values(Xs, ic, radii, directed) if base is None else base)
    out['Y'] = np.asarray(Y) != 0
    out['eligible'] = eligible_dyads(Y, directed, among, mask)
    out['rank'] = ranked(out['pw'][..., 0], out['eligible'], largest)
    out['eligible_t'] = out['eligible'].sum(axis=(1, 2))
    return out


def tolerances(ref):
    """((T, N, N) tolerance of pbar, of sd): proba_ref.tolerance, 16 eps + 4 ulp of the value with eps the
    reference's own error on this input"""
    return proba_ref.tolerance(ref, 0)[0], proba_ref.tolerance(ref, 1)[0]


def cut_is_decided(ref, t, k, tol):
    """The first k of time step t are the same set for every ranking within ``tol`` of the reference's values: the
    k-th and the (k + 1)-th value differ by more than twice the tolerance, or they lie in a group of bit-equal values
    whose neighbours on both sides are that far away (the group is then cut by (i, j)).  True as well when k takes
    every eligible dyad."""
    i, j = ref['rank'][t]
    n = i.size
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


def tile_rows(D):
    return 32 if D <= 4 else 16


def tiles_reaching(ref, D, directed, k, largest):
    """(per time step the tiles - tile_rows(D) x 64 dyads - whose extreme key of the eligible dyads reaches the key of
    the k-th, the tiles of a time step that hold a dyad at all): what the second pass must visit"""
    T, N = ref['eligible'].shape[:2]
    TI = tile_rows(D)
    keys = score_ref.key(ref['pw'][..., 0])
    reach = []
    n_tiles = 0
    for bi in range(-(-N // TI)):
        for bj in range(-(-N // 64)):
            n_tiles += bool(ref['exists'][0, bi * TI:(bi + 1) * TI, bj * 64:(bj + 1) * 64].any())
    for t in range(T):
        i, j = ref['rank'][t]
        if not i.size:
            reach.append(0)
            continue
        kappa = keys[t, i[min(k, i.size) - 1], j[min(k, i.size) - 1]]
        n = 0
        for bi in range(-(-N // TI)):
            for bj in range(-(-N // 64)):
                sl = (t, slice(bi * TI, (bi + 1) * TI), slice(bj * 64, (bj + 1) * 64))
                kk = keys[sl][ref['eligible'][sl]]
                if kk.size:
                    n += bool(kk.max() >= kappa) if largest else bool(kk.min() <= kappa)
        reach.append(n)
    return np.array(reach), n_tiles
