"""Host restatement of the posterior edge probabilities (numpy): mean, standard deviation (ddof 1) and the
equal-tailed interval (np.quantile, the default definition) of p_s = expit(eta_s) of every dyad in float64, in
np.longdouble and on probabilities moved by +-4 ulp, and the integer tables of the scored dyads built from its own
posterior mean with Python ints.  Written independently of dynetlsm_amd/probabilities.py and
csrc/kernels_proba.hpp; dense (S, T, N, N) arrays, for the small shapes of the tests.  eta is
score_ref.linear_predictor."""
import numpy as np

import score_ref

UNIT = 1 << 32                         # the tables hold probabilities in units of 2^-32


def expit(eta):
    """expit in eta's dtype, without overflow"""
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1 / (1 + e), e / (1 + e))


def summaries(p, level):
    """(mean, sd, lower, upper) over axis 0 of the probabilities p (S, ...), in p's dtype"""
    alpha = (1.0 - level) / 2.0
    lower, upper = np.quantile(p, [alpha, 1.0 - alpha], axis=0)
    return p.mean(axis=0), p.std(axis=0, ddof=1), lower, upper


def perturbed(p, seed=77):
    """every p_s moved by +-4 ulp with random signs: the allowance of the device's exp and division"""
    rng = np.random.RandomState(seed)
    return p + (rng.randint(0, 2, p.shape) * 2 - 1) * 4 * np.spacing(p)


def fix(x):
    """llrint(x 2^32) as a Python int (the product is exact; rint rounds half to even)"""
    return int(np.rint(np.float64(x) * UNIT))


def mean_bin(pbar, n_bins):
    return np.minimum(np.floor(np.asarray(pbar, dtype=np.float64) * n_bins), n_bins - 1).astype(np.int64)


def width_bin(width, edges):
    return np.searchsorted(np.asarray(edges, dtype=np.float64), width, side='right')


def tables(Y, pw, scored, n_bins, edges):
    """the integer tables of the scored dyads from the pointwise (T, N, N, 4): calib [T][n_bins][3], brier [T],
    node_sums [T][N][2], hist [T][len(edges) + 1], all Python ints"""
    T, N = scored.shape[:2]
    calib = [[[0, 0, 0] for _ in range(n_bins)] for _ in range(T)]
    brier = [0] * T
    node = [[[0, 0] for _ in range(N)] for _ in range(T)]
    hist = [[0] * (len(edges) + 1) for _ in range(T)]
    for t, i, j in np.argwhere(scored):
        pbar, y = pw[t, i, j, 0], int(Y[t, i, j] != 0)
        q = fix(pbar)
        row = calib[t][int(mean_bin(pbar, n_bins))]
        row[0] += 1
        row[1] += y
        row[2] += q
        brier[t] += fix((y - pbar) * (y - pbar))
        node[t][i][0] += q
        node[t][j][1] += q
        hist[t][int(width_bin(pw[t, i, j, 3] - pw[t, i, j, 2], edges))] += 1
    return calib, brier, node, hist


def bins_are_stable(pw, scored, n_bins, edges, margin=1e-12):
    """the bin of every scored dyad's mean is the same at pbar (1 +- margin), that of its width at width +- margin"""
    pbar = pw[..., 0][scored]
    width = (pw[..., 3] - pw[..., 2])[scored]
    return bool(np.all(mean_bin(pbar * (1 - margin), n_bins) == mean_bin(pbar * (1 + margin), n_bins)) and
                np.all(width_bin(width - margin, edges) == width_bin(width + margin, edges)))


def reference(Y, Xs, ic, radii, directed, level, n_bins, edges, mask=None):
    """Everything the tests compare: 'exists' and 'scored' (T, N, N) boolean; 'pw', 'pw_ld', 'pw_pt' (T, N, N, 4)
    = (mean, sd, lower, upper) in float64, longdouble and on the perturbed probabilities, zero where no dyad is;
    'calib', 'brier', 'node_sums', 'hist' as ``tables`` builds them from 'pw'"""
    Y = np.asarray(Y)
    T, N = Y.shape[:2]
    exists = np.broadcast_to(score_ref.dyad_mask(N, directed), (T, N, N))
    scored = score_ref.scored_dyads(T, N, directed, mask)
    out = {'exists': exists, 'scored': scored}
    p64 = expit(score_ref.linear_predictor(Xs, ic, radii, directed))
    pld = expit(score_ref.linear_predictor(Xs, ic, radii, directed, np.longdouble))
    for key, p in (('pw', p64), ('pw_ld', pld), ('pw_pt', perturbed(p64))):
        pw = np.stack(summaries(p, level), axis=-1)
        out[key] = np.where(exists[..., None], pw, p.dtype.type(0))
    out['calib'], out['brier'], out['node_sums'], out['hist'] = tables(Y, out['pw'], scored, n_bins, edges)
    return out


def tolerance(ref, c):
    """(tol, eps) of column c of the pointwise quadruple: 16 eps + 4 ulp of the value, eps the reference's own
    error on this input - the larger of max |float64 - longdouble| and the largest change under the perturbation"""
    a64 = ref['pw'][..., c]
    eps = max(float(np.max(np.abs(a64.astype(np.longdouble) - ref['pw_ld'][..., c]))),
              float(np.max(np.abs(a64 - ref['pw_pt'][..., c]))))
    return 16.0 * eps + 4.0 * np.spacing(np.abs(a64)), eps


def calibration(calib_rows, brier_fix):
    """brute force from one table [n_bins][3] and its Brier sum: (n, reliability rows (n, ties, predicted,
    observed), brier, ece) in float64, NaN where empty"""
    n = sum(r[0] for r in calib_rows)
    rows, ece = [], 0.0
    for nb, ties, s in calib_rows:
        if nb:
            pred, obs = s / UNIT / nb, ties / nb
            ece += nb / n * abs(obs - pred)
        else:
            pred = obs = float('nan')
        rows.append((nb, ties, pred, obs))
    return n, rows, (brier_fix / UNIT / n if n else float('nan')), (ece if n else float('nan'))
