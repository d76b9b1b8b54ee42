"""Host restatement of the initialisation pipeline with the number format as an argument (float64 or
np.longdouble), written from oracle/init_oracle.py and independently of dynetlsm_amd/csrc/kernels_init.hpp:
SMACOF, the Sarkar-Moore eigen step, the sums behind the conditional MLEs (with the sum of |term| of each,
which the rounding bound of the device's sums is stated in) and scikit-learn's Lloyd loop as
dlsm_init_kmeans_lloyd runs it; and the case tables of tests/test_gpu_init_shapes.py with the inputs they run
on.  tests/test_init_ref_cpu.py pins the float64 form to the oracle and to the reference's outputs, and holds
every case to the conditions under which the reference is a reference (the replicas agree with each other,
no stopping test is decided by rounding, no eigenvalue gap or score gap is small).

TEST INFRASTRUCTURE ONLY."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import init_oracle as io

LD = np.longdouble
U = 2.0 ** -53


def _pairwise(X):
    diff = X[:, None, :] - X[None, :, :]
    return np.sqrt((diff * diff).sum(-1))


# ---- SMACOF ------------------------------------------------------------------------------------------------
def smacof_single(delta, X0, max_iter=300, eps=1e-6, dtype=np.float64, crit=None):
    """init_oracle.smacof_single, expression for expression, in ``dtype``; ``crit`` (a list) receives the
    value every evaluated stopping test compared with eps"""
    delta = np.asarray(delta, dtype=dtype)
    N = delta.shape[0]
    X = np.array(X0, dtype=dtype)
    dis = _pairwise(X)
    old_stress = None
    for it in range(max_iter):
        dis = dis.copy()
        dis[dis == 0] = 1e-5
        ratio = delta / dis
        B = -ratio
        B[np.arange(N), np.arange(N)] += ratio.sum(axis=1)
        X = B.dot(X) / N
        dis = _pairwise(X)
        stress = ((dis - delta) ** 2).sum() / 2
        if old_stress is not None:
            c = (old_stress - stress) / ((dis ** 2).sum() / 2)
            if crit is not None:
                crit.append(c)
            if c < eps:
                break
        old_stress = stress
    return X, stress, it + 1


def perturbed(X0, seed, ulps=4.0, together=()):
    """every entry of X0 moved by ``ulps`` ulp with random signs; the rows listed in ``together`` get the
    signs of the first of them (coincident rows stay coincident: separated by a few ulp they would be pushed
    apart by a whole dissimilarity, another input altogether)"""
    sign = np.where(np.random.RandomState(seed).rand(*X0.shape) < 0.5, -1.0, 1.0)
    for r in together[1:]:
        sign[..., r, :] = sign[..., together[0], :]
    return X0 + sign * ulps * np.spacing(np.abs(X0))


# ---- eigen step --------------------------------------------------------------------------------------------
def gmds_matrix(delta, X_prev, lmbda, dtype=np.float64):
    delta, X_prev = np.asarray(delta, dtype=dtype), np.asarray(X_prev, dtype=dtype)
    N = X_prev.shape[0]
    lmbda = dtype(lmbda)
    alpha, beta = 1.0 / (1.0 + lmbda), lmbda / (1.0 + lmbda)
    H = np.eye(N, dtype=dtype) - np.ones((N, N), dtype=dtype) / N
    return alpha * H.dot((-0.5 * delta ** 2).dot(H)) + beta * X_prev.dot(X_prev.T)


def _procrustes_onto(X_ref, X):
    """init_oracle.procrustes_onto; the D x D singular value decomposition of the long-double cross product
    runs in float64 (numpy has no other), so the rotation, and with it the result, carries float64's rounding
    of a D x D orthogonal matrix - the N-long sums before and after it do not"""
    U_, _, Vt = np.linalg.svd(np.asarray(X.T.dot(X_ref), dtype=np.float64))
    return X.dot(U_.dot(Vt).astype(X.dtype))


def gmds_step(delta, X_prev, lmbda=10.0, dtype=np.float64, return_all=False):
    """init_oracle.gmds_step in ``dtype``.  numpy has a symmetric eigensolver for float64 only: in long double
    the float64 eigenpairs of the long-double matrix are refined in long double (Rayleigh quotient, and the
    first-order correction of the vector over the float64 eigenbasis; three rounds)."""
    N, D = np.shape(X_prev)
    G = gmds_matrix(delta, X_prev, lmbda, dtype)
    w, E = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    w, E = w[::-1], E[:, ::-1]
    if dtype == np.float64:
        evals, evecs = w[:D], E[:, :D]
    else:
        El, wl = E.astype(dtype), w.astype(dtype)
        evals, evecs = np.empty(D, dtype=dtype), np.empty((N, D), dtype=dtype)
        for m in range(D):
            v = El[:, m].copy()
            for _ in range(3):
                v /= np.sqrt(v.dot(v))
                Gv = G.dot(v)
                theta = v.dot(Gv)
                c = El.T.dot(Gv - theta * v)
                den = theta - wl
                den[m] = 1.0
                c = c / den
                c[m] = 0.0
                v = v + El.dot(c)
            v /= np.sqrt(v.dot(v))
            evals[m], evecs[:, m] = v.dot(G.dot(v)), v
    X = evecs * np.sqrt(evals)
    Xp = np.asarray(X_prev, dtype=dtype)
    if dtype == np.float64:
        out = io.procrustes_onto(Xp, X)
    else:
        out = _procrustes_onto(Xp, X)
    return (out, evals, w) if return_all else (out, evals)


# ---- sums behind the conditional MLEs ----------------------------------------------------------------------
def _terms(eta, Y):
    """(y eta - log(1 + e^eta), y - expit(eta)) through e = exp(-|eta|): finite for every eta (the oracle's
    1 / (1 + exp(-eta)) overflows to the right limit past |eta| = 709 in float64, with a warning)"""
    e = np.exp(-np.abs(eta))
    sp = np.maximum(eta, 0) + np.log1p(e)
    return Y * eta - sp, Y - np.where(eta >= 0, 1, e) / (1 + e)


def mle_sums_undirected(Y, X, log_scale, intercept, squared=False, dtype=np.float64):
    """init_oracle.mle_sums_undirected in ``dtype`` -> (sums[3], sum of |term| of each), slice by slice"""
    T, N, _ = Y.shape
    X = np.asarray(X, dtype=dtype)
    scale = np.exp(dtype(log_scale))
    iu = np.triu(np.ones((N, N), dtype=bool), 1)
    off = ~np.eye(N, dtype=bool)
    s, a = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
    for t in range(T):
        dist = _pairwise(X[t])
        sd = scale * (dist ** 2 if squared else dist)
        ll, step = _terms(dtype(intercept) - sd, Y[t].astype(dtype))
        for k, term in enumerate((ll[iu], (-sd * step)[off], 0.5 * step[off])):
            s[k] += term.sum()
            a[k] += np.abs(term).sum()
    return s, a


def mle_sums_directed(Y, X, radii, b_in, b_out, squared=False, dtype=np.float64):
    """init_oracle.mle_sums_directed in ``dtype`` -> (sums[3], sum of |term| of each), slice by slice"""
    T, N, _ = Y.shape
    X, radii = np.asarray(X, dtype=dtype), np.asarray(radii, dtype=dtype)
    off = ~np.eye(N, dtype=bool)
    s, a = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
    for t in range(T):
        dist = _pairwise(X[t])
        if squared:
            dist = dist ** 2
        d_in = 1 - dist / radii[None, :]
        d_out = 1 - dist / radii[:, None]
        ll, step = _terms(dtype(b_in) * d_in + dtype(b_out) * d_out, Y[t].astype(dtype))
        for k, term in enumerate((ll[off], (d_in * step)[off], (d_out * step)[off])):
            s[k] += term.sum()
            a[k] += np.abs(term).sum()
    return s, a


def mle_sum_bound(T, N, abs_terms):
    """|device - exact| of one sum: (A + 16) 2^-53 sum |term|, A the additions on the longest path of the
    device's summation - ceil(N / 64) in a lane, the 6 levels of the wavefront's sum, the workgroup's 4
    wavefronts, ceil(records / 1024) in a thread of the final sum, the 6 + 4 levels of its workgroup's sum -
    and 16 roundings for the square root, the exponential, log1p and the division behind one term; never looser
    than the rtol 1e-10 / atol 1e-9 of test_gpu_init.py (applied by the caller, which knows the value)"""
    records = -(-N // 4) * T
    A = -(-N // 64) + 6 + 4 + -(-records // 1024) + 10
    return (A + 16) * U * np.asarray(abs_terms, dtype=LD)


# ---- Lloyd iterations --------------------------------------------------------------------------------------
def kmeans_lloyd(X, seeds, max_iter=300, tol=0.0, dtype=np.float64):
    """scikit-learn's _kmeans_single_lloyd as dlsm_init_kmeans_lloyd runs it: E-step = first minimum of
    |c|^2 - 2 x.c, M-step = mean of the members; the loop ends when a cluster emptied (the caller's business),
    when no label changed, when the summed squared shift of the centres is <= tol, or by count, and unless no
    label changed one more E-step follows.  Returns labels, centers, n_iter, emptied, and what decides whether
    the answer is well defined: ``history``, (labels changed, summed squared shift) of every iteration,
    ``min_gap``, the smallest non-zero gap between best and second-best score over all E-steps relative to the
    magnitude sum |c|^2 + 2 |x|.|c| of the terms of either score, ``ties``, the number of exact score ties met,
    ``tol_margin``, the smallest |shift - tol| / tol met, and ``members``, the labels the centres are the
    means of (the last M-step's; ``labels`` are those of the E-step after it)."""
    X = np.asarray(X, dtype=dtype)
    C = np.array(seeds, dtype=dtype)
    N, K = X.shape[0], C.shape[0]
    labels = np.full(N, -1)
    out = SimpleNamespace(emptied=False, min_gap=np.inf, ties=0, tol_margin=np.inf, strict=False, history=[])
    absX = np.abs(X)

    def e_step(C):
        c2 = (C * C).sum(axis=1)
        score = c2[None, :] - 2 * X.dot(C.T)
        lab = np.argmin(score, axis=1)                                # the first minimum
        if K > 1:
            mag = c2[None, :] + 2 * absX.dot(np.abs(C).T)
            two = np.argsort(score, axis=1, kind='stable')[:, :2]
            rows = np.arange(N)
            gap = score[rows, two[:, 1]] - score[rows, two[:, 0]]
            rel = gap / np.maximum(mag[rows, two[:, 0]], mag[rows, two[:, 1]])
            out.ties += int((gap == 0).sum())
            if (gap > 0).any():
                out.min_gap = min(out.min_gap, float(rel[gap > 0].min()))
        return lab

    it, strict = 0, False
    while it < max_iter:
        new = e_step(C)
        changed = int((new != labels).sum())
        labels = new
        counts = np.bincount(labels, minlength=K)
        if (counts == 0).any():
            out.emptied = True
            out.labels, out.centers, out.n_iter = labels, C, it + 1
            return out
        Cn = np.stack([X[labels == k].sum(axis=0) / counts[k] for k in range(K)])
        shift = ((Cn - C) ** 2).sum()
        C, out.members = Cn, labels                                   # whose means the centres are
        it += 1
        out.history.append((changed, float(shift)))
        if changed == 0:
            strict = True
            break
        if tol > 0:
            out.tol_margin = min(out.tol_margin, abs(float(shift) - tol) / tol)
        if shift <= tol:
            break
    if not strict:
        labels = e_step(C)
    out.labels, out.centers, out.n_iter, out.strict = labels, C, it, strict
    return out


def center_bound(X, labels, centers):
    """(ceil(N / 256) + 9) 2^-53 sum_members |x| / count + 1 ulp: the strided sum of a thread, the 6 + 2
    levels of the workgroup's sum, the division"""
    N, K = X.shape[0], centers.shape[0]
    A = -(-N // 256) + 9
    sabs = np.stack([np.abs(X[labels == k]).sum(axis=0) / max((labels == k).sum(), 1) for k in range(K)])
    return A * U * sabs + np.spacing(np.abs(np.asarray(centers, dtype=np.float64)))


# ============================================================================================================
# The inputs and case tables of tests/test_gpu_init_shapes.py.  Every seed below was chosen so that the case
# meets its condition in tests/test_init_ref_cpu.py; a case that stops meeting it gets another seed.
# ============================================================================================================
@functools.lru_cache(maxsize=None)
def network(T, N, D, seed, directed=False):
    """dynetlsm_amd.synthetic.synthetic_lsm_network at density 0.1 up to N = 130 and 0.03 above"""
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    return synthetic_lsm_network(T=T, N=N, D=D, density=0.1 if N <= 130 else 0.03, seed=seed, directed=directed)


@functools.lru_cache(maxsize=None)
def hops(T, N, D, seed, t, variant=None):
    Y = network(T, N, D, seed)['Y'][t]
    if variant == 'edgeless':
        Y = np.zeros_like(Y)
    return io.hop_matrix(Y)


# ---- SMACOF: name -> N, d, starts, max_iter, the eps values, network seed, start seed.  The starts are
# uniform on [0, spread_r)^d with a spread per start, which is what makes the runs stop at different iterations.
SMACOF_CASES = {
    # one lane of a row's wavefront makes a second trip; the largest n_init (the grid's y extent and the
    # records' indexing by run); 20 iterations: the paths past one trip do not depend on the count
    'n65_64_starts': dict(N=65, d=2, n_init=64, max_iter=20, eps=(1e-6,), net=1, start=1),
    # three trips, 33 workgroups of which the last holds two rows
    'n130_d2': dict(N=130, d=2, n_init=3, max_iter=300, eps=(1e-6, 1e-3), net=2, start=2),
    'n130_d3': dict(N=130, d=3, n_init=3, max_iter=300, eps=(1e-6, 1e-3), net=2, start=3),
    'n130_d5': dict(N=130, d=5, n_init=3, max_iter=300, eps=(1e-6, 1e-3), net=2, start=5),
    'n130_d8': dict(N=130, d=8, n_init=3, max_iter=300, eps=(1e-6, 1e-3), net=2, start=38),
    # one dimension: ill-conditioned in the reference.  max_iter is the largest count at which the float64 and
    # long-double replicas still agree to 1e-10 of the scale, and that is 1: the Guttman transform of a line is
    # (1/N) sum_j delta_ij sign(x_i - x_j), multiples of 1/N among which two of 130 nodes coincide after the first
    # iteration (every one of 36 starts tried); from then on the oracle's form adds and subtracts 1e5 delta_ij x
    # for the coincident pair, and the rounding of that decides on which side of each other the two land
    'n130_d1': dict(N=130, d=1, n_init=3, max_iter=1, eps=(1e-6,), net=2, start=1),
    # rows 3 and 77 of every start coincide: dis == 0 off the diagonal
    'n130_d2_coincident': dict(N=130, d=2, n_init=3, max_iter=50, eps=(1e-6,), net=2, start=4, together=(3, 77)),
    # 258 workgroups: the check's 256 threads stride over the records; the last workgroup holds two rows
    'n1030_d2': dict(N=1030, d=2, n_init=2, max_iter=6, eps=(1e-6,), net=3, start=6),
}
SPREADS = (1.0, 0.05, 4.0)


def smacof_starts(name):
    c = SMACOF_CASES[name]
    rng = np.random.RandomState(c['start'])
    X0 = rng.uniform(size=(c['n_init'], c['N'], c['d']))
    X0 *= np.array([SPREADS[r % len(SPREADS)] for r in range(c['n_init'])])[:, None, None]
    if 'together' in c:
        a, b = c['together']
        X0[:, b] = X0[:, a]
    return X0


def smacof_delta(name):
    c = SMACOF_CASES[name]
    return hops(2, c['N'], 2, c['net'], 0)


def smacof_network(name):
    c = SMACOF_CASES[name]
    return network(2, c['N'], 2, c['net'])['Y']


@functools.lru_cache(maxsize=None)
def smacof_reference(name, eps):
    """per start: the float64 answer, the long-double answer, the float64 answer from the start moved by
    4 ulp, and the values the stopping tests saw in either precision.  -> namespace of arrays over the starts:
    X64, Xld, Xpt, s64, sld, spt, n64, nld, crit64, critld"""
    c = SMACOF_CASES[name]
    delta, X0 = smacof_delta(name), smacof_starts(name)
    Xp = perturbed(X0, 100 + c['start'], together=c.get('together', ()))
    max_iter = c['max_iter']
    r = SimpleNamespace(X64=[], Xld=[], Xpt=[], s64=[], sld=[], spt=[], n64=[], nld=[], crit64=[], critld=[])
    for k in range(c['n_init']):
        c64, cld = [], []
        X, s, n = smacof_single(delta, X0[k], max_iter, eps, np.float64, c64)
        Xl, sl, nl = smacof_single(delta, X0[k], max_iter, eps, LD, cld)
        Xq, sq, _ = smacof_single(delta, Xp[k], max_iter, eps, np.float64)
        r.X64.append(X); r.Xld.append(Xl); r.Xpt.append(Xq)
        r.s64.append(s); r.sld.append(sl); r.spt.append(sq)
        r.n64.append(n); r.nld.append(nl); r.crit64.append(c64); r.critld.append(cld)
    for k in ('X64', 'Xld', 'Xpt', 's64', 'sld', 'spt', 'n64', 'nld'):
        setattr(r, k, np.array(getattr(r, k)))
    return r


def smacof_tolerances(r):
    """ic_ref.tolerance's rule, 16 eps + 4 ulp, with eps the larger of |float64 - long double| and the change
    under the 4 ulp move of the start; capped by test_gpu_init.py's 1e-8 of the scale (X) and 1e-9 relative
    (stress).  -> (tol_X, eps_X, tol_s, eps_s), the tolerances with the shapes of X64 and s64"""
    eps_X = float(max(np.abs(r.X64.astype(LD) - r.Xld).max(), np.abs(r.X64 - r.Xpt).max()))
    eps_s = float(max(np.abs(r.s64.astype(LD) - r.sld).max(), np.abs(r.s64 - r.spt).max()))
    scale = np.abs(r.X64).max(axis=(1, 2), keepdims=True)
    tol_X = np.minimum(16 * eps_X + 4 * np.spacing(np.abs(r.X64)), 1e-8 * scale)
    tol_s = np.minimum(16 * eps_s + 4 * np.spacing(np.abs(r.s64)), 1e-9 * np.abs(r.s64))
    return tol_X, eps_X, tol_s, eps_s


# ---- eigen step: (N, d) -> (the network's seed, the dimension of the space it was drawn in); X_prev is the
# float64 replica's SMACOF answer on slice 0 from a uniform start (300 iterations; 6 at N = 1030, where an
# iteration of the replica takes a tenth of a second), the step is that of slice 1.  At N = 1030 a network
# drawn in two dimensions has a third eigenvalue so far below the second that Lanczos is done with 24 vectors
# at every lambda (six seeds tried); drawn in three, lambda = 0 takes 32.
GMDS_CASES = {(65, 8): (11, 2), (130, 3): (12, 2), (261, 2): (13, 2), (1030, 2): (16, 3)}
GMDS_LAMBDAS = (10.0, 0.5, 0.0)
GMDS_EDGELESS = ((130, 3), (10.0, 0.5))            # at lambda = 0 the matrix of an edgeless slice is H / 2
GMDS_UNCONVERGED = ((130, 3), 0.0, (8, 16))


@functools.lru_cache(maxsize=None)
def gmds_input(N, d, variant=None):
    """(Y (2, N, N), delta of slice 1, X_prev)"""
    seed, latent = GMDS_CASES[(N, d)]
    Y = network(2, N, latent, seed)['Y']
    if variant == 'edgeless':
        Y = Y.copy()
        Y[1] = 0
    X0 = np.random.RandomState(seed).uniform(size=(N, d))
    X_prev = smacof_single(hops(2, N, latent, seed, 0), X0, 6 if N > 300 else 300)[0]
    return Y, hops(2, N, latent, seed, 1, variant), X_prev


def lanczos_vectors(G, d, seed, tol=1e-12, kmax=256):
    """the number of Lanczos vectors after which the top d Ritz pairs of the dense matrix G meet the residual
    test max_m |beta_k s_km| <= tol max |theta|, looked at when the count is a multiple of 8 (run_gmds_step's
    schedule), from a random start; float64, two passes of Gram-Schmidt against every earlier vector.  The
    count belongs to the spectrum much more than to the start: it tells, without a device, whether a case
    reaches the columns it is there for."""
    N = G.shape[0]
    q = np.random.RandomState(seed).rand(N) - 0.5
    Q, al, be = [q / np.sqrt(q.dot(q))], [], []
    kk = 0
    for k in range(min(kmax, N)):
        w = G.dot(Q[k])
        a = w.dot(Q[k])
        w = w - a * Q[k] - (be[-1] * Q[k - 1] if k else 0.0)
        Qm = np.array(Q)
        for _ in range(2):
            w = w - Qm.T.dot(Qm.dot(w))
        b = np.sqrt(w.dot(w))
        al.append(a)
        be.append(b)
        Q.append(w / b if b > 0 else w * 0.0)
        kk = k + 1
        if kk < d or (kk % 8 and kk != kmax):
            continue
        theta, S = np.linalg.eigh(np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1))
        theta, S = theta[::-1][:d], S[:, ::-1][:, :d]
        if np.abs(b * S[-1]).max() <= tol * np.abs(theta).max() or kk == N:
            break
    return kk


@functools.lru_cache(maxsize=None)
def gmds_reference(N, d, lmbda, variant=None):
    """init_oracle.gmds_step's (X, evals) and every eigenvalue of the dense matrix, descending"""
    _, delta, X_prev = gmds_input(N, d, variant)
    X, evals, w = gmds_step(delta, X_prev, lmbda, return_all=True)
    return X, evals, w


# ---- MLE sums: (T, N, d), the network's seed and what is done to it.  Positions: the network's X_init.
MLE_UNDIRECTED = {
    (1, 65, 1): dict(net=21),
    (2, 130, 3): dict(net=22),
    (3, 257, 8): dict(net=23, empty=1, complete=2),         # slice 1 without edges, slice 2 complete
    (6, 700, 2): dict(net=24),                              # 1050 records
}
MLE_DIRECTED = {
    (2, 130, 2): dict(net=25, isolated=17),                 # node 17 has no ties at all: the radii's reg path
    (5, 900, 5): dict(net=26, empty=3),                     # 1125 records
}
# a point near the oracle's optimum on each input (its BFGS answer rounded to two digits)
MLE_NEAR_OPTIMUM = {       # (case, directed, squared)
    ((1, 65, 1), False, False): (0.02, -1.01), ((1, 65, 1), False, True): (-1.28, -1.56),
    ((2, 130, 3), False, False): (0.11, 0.90), ((2, 130, 3), False, True): (-1.73, -0.53),
    ((3, 257, 8), False, False): (-1.06, 1.12), ((3, 257, 8), False, True): (-22.89, -0.65),
    ((6, 700, 2), False, False): (-0.01, -1.50), ((6, 700, 2), False, True): (-1.44, -2.28),
    ((2, 130, 2), True, False): (0.60, 0.53), ((5, 900, 5), True, False): (0.68, 0.69),
}
# init_oracle.scale_intercept_mle on the (6, 700, 2) input, recorded: its BFGS run takes a minute of host time
# (test_init_ref_cpu.py holds the point to be stationary for the oracle's own sums)
MLE_ORACLE_OPTIMUM_6_700_2 = (-0.014462171372143848, -1.501201492804799)
ETA_EXTREME = 800.0


@functools.lru_cache(maxsize=None)
def mle_input(key, directed):
    """(Y, X, radii or None)"""
    T, N, d = key
    c = (MLE_DIRECTED if directed else MLE_UNDIRECTED)[key]
    net = network(T, N, d, c['net'], directed)
    Y, X = net['Y'].copy(), net['X_init']
    if 'empty' in c:
        Y[c['empty']] = 0
    if 'complete' in c:
        Y[c['complete']] = 1 - np.eye(N)
    if not directed:
        return Y, X, None
    if 'isolated' in c:
        Y[:, c['isolated'], :] = 0
        Y[:, :, c['isolated']] = 0
    radii = io.initialize_radii(Y)
    return Y, X / N, radii                                  # generalized_mds's scale for the directed model


def mle_points(key, directed, squared=False):
    """the BFGS starting point, a point near the optimum, and one at which |eta| reaches ETA_EXTREME on the
    farthest dyad (so exp(-|eta|) underflows for part of them)"""
    Y, X, radii = mle_input(key, directed)
    far = max(_pairwise(X[t]).max() for t in range(X.shape[0]))
    if squared:
        far = far ** 2
    if not directed:
        return [(0.0, 1.0), MLE_NEAR_OPTIMUM[(key, False, squared)], (float(np.log(ETA_EXTREME / far)), 1.0)]
    worst = 0.0
    for t in range(X.shape[0]):
        dist = _pairwise(X[t]) ** (2 if squared else 1)
        worst = max(worst, np.abs((1 - dist / radii[None, :]) + (1 - dist / radii[:, None])).max())
    b = ETA_EXTREME / worst
    return [(0.0, 0.0), MLE_NEAR_OPTIMUM[(key, True, squared)], (float(b), float(b))]


# ---- Lloyd iterations: (N, F, K) and the seed of the data; the seeds of the clusters are data rows
KMEANS_CASES = {(257, 3, 2): 31, (300, 80, 64): 32, (300, 80, 101): 33}
KMEANS_SEPARATION = {(257, 3, 2): 3.0, (300, 80, 64): 3.0, (300, 80, 101): None}
KMEANS_STOPS = ('max_iter_1', 'max_iter_2', 'tol', 'labels')


def kmeans_input(key, stop='labels'):
    """(X centred (N, F), seeds (K, F), max_iter, tol): K groups around well-separated centres, the seeds one
    data row of each group in turn"""
    N, F, K = key
    rng = np.random.RandomState(KMEANS_CASES[key])
    group = np.arange(N) % K
    if KMEANS_SEPARATION[key] is None:      # no groups: a three-dimensional cloud embedded in F dimensions
        X = rng.randn(N, 3).dot(rng.randn(3, F)) + 0.05 * rng.randn(N, F)
    else:
        X = rng.randn(K, F)[group] * KMEANS_SEPARATION[key] + rng.randn(N, F)
    X -= X.mean(axis=0)
    # seeds: rows 0 .. K-1 belong to groups 0 .. K-1; two seeds share a group and one group has none, so that
    # the centres move for a few iterations
    rows = np.arange(K)
    rows[K - 1] = K - 2 + K if K > 2 else K - 1
    seeds = X[rows].copy()
    max_iter, tol = {'max_iter_1': (1, 0.0), 'max_iter_2': (2, 0.0), 'tol': (300, None),
                     'labels': (300, 0.0)}[stop]
    if tol is None:
        tol = KMEANS_TOL[key]
    return X, seeds, max_iter, tol


# a tol that the summed squared shift of the centres falls below while labels are still changing
KMEANS_TOL = {(257, 3, 2): 0.05, (300, 80, 64): 100.0, (300, 80, 101): 50.0}


def kmeans_ties():
    """integer coordinates: sample 0 is equidistant from centres 0 < 2 (and nearer to them than to centre 1),
    samples 2 and 3 are duplicates on the bisector of centres 1 and 2 -> (X, seeds); every score is a small
    integer on both sides"""
    rng = np.random.RandomState(41)
    seeds = np.array([[-20.0, 0.0], [40.0, 60.0], [20.0, 0.0]])
    v = rng.randint(-3, 4, size=(3, 40, 2)).astype(np.float64)
    body = np.concatenate([seeds[k] + np.concatenate([v[k], -v[k]]) for k in range(3)])   # means = the seeds
    # (0, -7): 449 from centres 0 and 2; (30, 30): 1000 from centres 1 and 2, twice.  The first minimum puts
    # them in clusters 0 and 1, where their mirror images about the centre keep the mean on the seed: the centres
    # do not move (shift 0 <= tol 0 ends the loop after one iteration) and the E-step that follows sees the same
    # integer scores, ties included
    special = np.array([[0.0, -7.0], [-40.0, 7.0], [30.0, 30.0], [30.0, 30.0], [50.0, 90.0], [50.0, 90.0]])
    X = np.concatenate([special, body])
    return X, seeds


TIE_ROWS = dict(between_0_and_2=0, duplicates_between_1_and_2=(2, 3))


# ---- the pipeline at a middle size
PIPELINE_CASE = dict(T=3, N=130, d=2, net={False: 51, True: 52}, rs=5)


def pipeline_input(directed):
    c = PIPELINE_CASE
    return network(c['T'], c['N'], c['d'], c['net'][directed], directed)['Y']


# ---- the parametrisations shared by test_init_ref_cpu.py (conditions) and test_gpu_init_shapes.py (values)
SMACOF_RUNS = [(name, eps) for name, c in SMACOF_CASES.items() for eps in c['eps']]
GMDS_RUNS = ([(N, d, lm, None) for (N, d) in GMDS_CASES for lm in GMDS_LAMBDAS] +
             [GMDS_EDGELESS[0] + (lm, 'edgeless') for lm in GMDS_EDGELESS[1]])
MLE_RUNS = ([(k, False, sq) for k in MLE_UNDIRECTED for sq in (False, True)] +
            [(k, True, False) for k in MLE_DIRECTED])
