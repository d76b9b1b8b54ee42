"""Host restatement of the tie dynamics (numpy): for every dyad and every step u = t -> t + 1 the mean and the
standard deviation (ddof 1) of d_s = p_{s,t+1} - p_{s,t}, p = expit(eta), in float64, in np.longdouble and on
probabilities moved by +-4 ulp, the integer numbers of samples in which eta rose and fell, and the integer tables of
the scored steps built from its own float64 values with Python ints.  Written independently of
dynetlsm_amd/dynamics.py and csrc/kernels_dynamics.hpp; dense (S, T, N, N) arrays, for the small shapes of the
tests.  eta is score_ref.linear_predictor, expit / fix / perturbed are proba_ref's."""
import numpy as np

import proba_ref
import score_ref

UNIT = proba_ref.UNIT


def signs_are_stable(*etas):
    """The precondition of comparing the counts of risen and fallen samples exactly: in every eta (S, T, N, N)
    given - the float64 one and the longdouble one -, each eta_{t+1} - eta_t is either exactly 0 or larger in
    magnitude than 1e-9 max(1, |eta|), far beyond what the device's fused sum of squares can move"""
    for eta in etas:
        diff = eta[:, 1:] - eta[:, :-1]
        scale = np.maximum(1, np.maximum(np.abs(eta[:, 1:]), np.abs(eta[:, :-1])))
        if not np.all((diff == 0) | (np.abs(diff) > 1e-9 * scale)):
            return False
    return True


def _moments(p):
    """(delta_mean, delta_sd) (T - 1, N, N) of the probabilities p (S, T, N, N), in p's dtype"""
    d = p[:, 1:] - p[:, :-1]
    return d.mean(axis=0), d.std(axis=0, ddof=1)


def _fix(a):
    """llrint(x 2^32) of an array in [0, 1] as int64 (the product is exact; rint rounds half to even)"""
    return np.rint(np.asarray(a, dtype=np.float64) * UNIT).astype(np.int64)


def up_bin(up, n_bins, S):
    return np.minimum(np.asarray(up, dtype=np.int64) * n_bins // S, n_bins - 1)


def tables(Y, scored, pbar0, pbar1, persist, delta_mean, up, down, min_count, n_bins, S):
    """the integer tables of the scored steps (U, N, N): transitions [U][4][4], hist_up [U][n_bins], node_changes
    [U][N][4], node_turnover [U][N][2], all Python ints (every sum is below 2^63: an int64 holds it)"""
    U, N = scored.shape[:2]
    y = np.asarray(Y) != 0
    cls = 2 * y[:-1].astype(np.int64) + y[1:]
    tr = np.zeros((U, 4, 4), dtype=np.int64)
    hist = np.zeros((U, n_bins), dtype=np.int64)
    changes = np.zeros((U, N, 4), dtype=np.int64)
    turn = np.zeros((U, N, 2), dtype=np.int64)
    u, i, j = np.nonzero(scored)
    c = cls[u, i, j]
    for v, a in enumerate((np.ones(scored.shape, dtype=np.int64), _fix(pbar0), _fix(pbar1), _fix(persist))):
        np.add.at(tr, (u, c, v), a[u, i, j])
    np.add.at(hist, (u, up_bin(up, n_bins, S)[u, i, j]), 1)
    rose = (up >= min_count).astype(np.int64)[u, i, j]
    fell = (down >= min_count).astype(np.int64)[u, i, j]
    np.add.at(changes, (u, i, 0), rose)
    np.add.at(changes, (u, j, 1), rose)
    np.add.at(changes, (u, i, 2), fell)
    np.add.at(changes, (u, j, 3), fell)
    q = _fix(np.abs(delta_mean))[u, i, j]
    np.add.at(turn, (u, i, 0), q)
    np.add.at(turn, (u, j, 1), q)
    return tuple(a.astype(object).tolist() for a in (tr, hist, changes, turn))


def reference(Y, Xs, ic, radii, directed, min_count, n_bins, mask=None):
    """Everything the tests compare.  U = T - 1 steps.  'exists' and 'scored' (U, N, N) boolean (scored: the dyad
    is unmasked at t and at t + 1); 'pw', 'pw_ld', 'pw_pt' (U, N, N, 4) = (delta_mean, delta_sd, prob_up, prob_down)
    in float64, longdouble and on the perturbed probabilities (the two probabilities are those of float64 in all
    three), zero where no dyad is; 'up', 'down' (U, N, N) int64; 'pbar0', 'pbar1', 'persist' (U, N, N) float64;
    'transitions', 'hist_up', 'node_changes', 'node_turnover' as ``tables`` builds them; 'eta', 'eta_ld' for
    ``signs_are_stable``"""
    Y = np.asarray(Y)
    T, N = Y.shape[:2]
    S = np.shape(Xs)[0]
    exists = np.broadcast_to(score_ref.dyad_mask(N, directed), (T - 1, N, N))
    unmasked = score_ref.scored_dyads(T, N, directed, mask)
    scored = unmasked[:-1] & unmasked[1:]
    eta = score_ref.linear_predictor(Xs, ic, radii, directed)
    eta_ld = score_ref.linear_predictor(Xs, ic, radii, directed, np.longdouble)
    out = {'exists': exists, 'scored': scored, 'eta': eta, 'eta_ld': eta_ld}
    up = np.where(exists, (eta[:, 1:] > eta[:, :-1]).sum(axis=0), 0).astype(np.int64)
    down = np.where(exists, (eta[:, 1:] < eta[:, :-1]).sum(axis=0), 0).astype(np.int64)
    out['up'], out['down'] = up, down
    p64 = proba_ref.expit(eta)
    for key, p in (('pw', p64), ('pw_ld', proba_ref.expit(eta_ld)), ('pw_pt', proba_ref.perturbed(p64))):
        mean, sd = _moments(p)
        pw = np.stack([mean, sd, (up / np.float64(S)).astype(p.dtype), (down / np.float64(S)).astype(p.dtype)],
                      axis=-1)
        out[key] = np.where(exists[..., None], pw, p.dtype.type(0))
    out['pbar0'], out['pbar1'] = p64[:, :-1].mean(axis=0), p64[:, 1:].mean(axis=0)
    out['persist'] = (p64[:, :-1] * p64[:, 1:]).mean(axis=0)
    (out['transitions'], out['hist_up'], out['node_changes'], out['node_turnover']) = tables(
        Y, scored, out['pbar0'], out['pbar1'], out['persist'], out['pw'][..., 0], up, down, min_count, n_bins, S)
    return out


def tolerance(ref, c):
    """(tol, eps) of column c (0: delta_mean, 1: delta_sd) of the pointwise quadruple: 16 eps + 4 ulp of the value,
    eps the reference's own error on this input - the larger of max |float64 - longdouble| and the largest change
    under the perturbation"""
    a64 = ref['pw'][..., c]
    eps = max(float(np.max(np.abs(a64.astype(np.longdouble) - ref['pw_ld'][..., c]))),
              float(np.max(np.abs(a64 - ref['pw_pt'][..., c]))))
    return 16.0 * eps + 4.0 * np.spacing(np.abs(a64)), eps
