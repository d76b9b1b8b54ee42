"""tests/init_ref.py without a GPU: its float64 form against oracle/init_oracle.py (bit for bit where both
state the same expression, 1e-13 where the sums are taken in another order) and against the reference's own
outputs (tests/golden/init.npz, wide_init.npz, kmeans.npz) at the tolerances of test_init_oracle_golden.py;
and, for every case of its tables, the conditions under which tests/test_gpu_init_shapes.py may hold the
device to it.  A case that stops meeting its condition gets another seed in the table; nothing here skips."""
import numpy as np
import pytest

import init_ref as ir
from conftest import INIT_CASES, load_golden
from oracle import init_oracle as io

LD = ir.LD


# ---- the replica is the oracle ------------------------------------------------------------------------------
def test_smacof_replica_is_the_oracle_bit_for_bit(golden_init):
    inputs = [(golden_init['u_D'][0], np.random.RandomState(3).uniform(size=(40, 2)), 300, 1e-6),
              (golden_init['u3_D'][1], np.random.RandomState(4).uniform(size=(25, 3)), 300, 1e-3),
              (ir.smacof_delta('n65_64_starts'), ir.smacof_starts('n65_64_starts')[5], 12, 1e-6)]
    for delta, X0, max_iter, eps in inputs:
        crit = []
        X, s, n = ir.smacof_single(delta, X0, max_iter, eps, crit=crit)
        Xo, so, no = io.smacof_single(delta, X0, max_iter, eps)
        np.testing.assert_array_equal(X, Xo)
        assert s == so and n == no and len(crit) == n - 1
        Xl, sl, nl = ir.smacof_single(delta, X0, max_iter, eps, LD)
        assert Xl.dtype == LD and nl == n
        assert np.abs(Xl - X).max() < 1e-10 * np.abs(X).max()


@pytest.mark.parametrize('tag,directed,D', INIT_CASES)
def test_gmds_replica_is_the_oracle_and_its_long_double_form_agrees(golden_init, tag, directed, D):
    Y = golden_init[tag + '_Y']
    Xg = golden_init[tag + '_X'] * (Y.shape[1] if directed else 1.0)
    for lmbda in (10.0, 0.5):
        delta = golden_init[tag + '_D'][1]
        X, ev = ir.gmds_step(delta, Xg[0], lmbda)
        Xo, eo = io.gmds_step(delta, Xg[0], lmbda)
        np.testing.assert_array_equal(X, Xo)
        np.testing.assert_array_equal(ev, eo)
        Xl, el = ir.gmds_step(delta, Xg[0], lmbda, LD)
        assert Xl.dtype == LD and el.dtype == LD
        np.testing.assert_allclose(el.astype(np.float64), ev, rtol=1e-12)
        assert np.abs(Xl - X).max() < 1e-10 * np.abs(X).max()


def test_mle_sum_replicas_are_the_oracle(golden_init):
    """the replica sums slice by slice and goes through exp(-|eta|): 1e-13 of sum |term|"""
    g = golden_init
    for tag in ('u', 'u8'):
        Y, X = g[tag + '_Y'], g[tag + '_X']
        for p in [(0.0, 1.0), (0.2, 0.7), (-1.0, 3.0)]:
            for sq in (False, True):
                s, a = ir.mle_sums_undirected(Y, X, p[0], p[1], sq)
                assert (np.abs(s - io.mle_sums_undirected(Y, X, p[0], p[1], sq)) <= 1e-13 * a).all()
                sl, al = ir.mle_sums_undirected(Y, X, p[0], p[1], sq, LD)
                assert sl.dtype == LD and (np.abs(sl - s) <= 1e-13 * a).all() and (np.abs(al - a) <= 1e-13 * a).all()
    for tag in ('d', 'd6'):
        Y, X, radii = g[tag + '_Y'], g[tag + '_X'], g[tag + '_radii']
        for p in [(0.0, 0.0), (0.4, -0.3)]:
            s, a = ir.mle_sums_directed(Y, X, radii, p[0], p[1])
            assert (np.abs(s - io.mle_sums_directed(Y, X, radii, p[0], p[1])) <= 1e-13 * a).all()
            sl, _ = ir.mle_sums_directed(Y, X, radii, p[0], p[1], False, LD)
            assert (np.abs(sl - s) <= 1e-13 * a).all()


# ---- the replica is the reference ---------------------------------------------------------------------------
def test_mle_sums_match_the_reference(golden_init):
    g = golden_init
    for tag in ('u', 'u3', 'u5', 'u8'):
        Y, X = g[tag + '_Y'], g[tag + '_X']
        for p, f, gr in zip(g[tag + '_mle_points'], g[tag + '_mle_f'], g[tag + '_mle_g']):
            for dtype in (np.float64, LD):
                s = ir.mle_sums_undirected(Y, X, p[0], p[1], dtype=dtype)[0].astype(np.float64)
                np.testing.assert_allclose(s[0], f, rtol=1e-11)
                np.testing.assert_allclose(s[1:], gr, rtol=1e-10, atol=1e-9)
    for tag in ('d', 'd6'):
        Y, X, radii = g[tag + '_Y'], g[tag + '_X'], g[tag + '_radii']
        for p, f, gr in zip(g[tag + '_mle_points'], g[tag + '_mle_f'], g[tag + '_mle_g']):
            s = ir.mle_sums_directed(Y, X, radii, p[0], p[1])[0]
            np.testing.assert_allclose(s[0], f, rtol=1e-11)
            np.testing.assert_allclose(s[2], gr[1], rtol=1e-10, atol=1e-9)   # (the in-gradient: see the oracle's test)


@pytest.mark.parametrize('tag,directed,D', INIT_CASES)
def test_pipeline_of_replicas_matches_the_reference(golden_init, tag, directed, D):
    """latent_space.py:47-95 assembled from the replica's SMACOF (best of four) and eigen steps"""
    Y, X_ref = golden_init[tag + '_Y'], golden_init[tag + '_X']
    T, N, _ = Y.shape
    rng = np.random.RandomState(int(golden_init[tag + '_seed']))
    runs = [ir.smacof_single(golden_init[tag + '_D'][0], rng.uniform(size=N * D).reshape(N, D)) for _ in range(4)]
    X = np.empty((T, N, D))
    X[0] = runs[int(np.argmin([r[1] for r in runs]))][0]
    for t in range(1, T):
        X[t] = ir.gmds_step(golden_init[tag + '_D'][t], X[t - 1])[0]
    if directed:
        X /= N
    assert np.abs(X - X_ref).max() < 2e-6 * np.abs(X_ref).max()


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd'])
def test_lloyd_replica_matches_the_reference(tag):
    """initialization._kmeans with the replica's loop in the device's place, against tests/golden/kmeans.npz"""
    from dynetlsm_amd import initialization as im
    g = load_golden('kmeans.npz')
    X, K = g[tag + '_X'], int(g[tag + '_K'])
    T, N, D = X.shape
    rs = np.random.RandomState(int(g[tag + '_seed']))
    Xc = np.array(np.moveaxis(X, 0, -1).reshape(N, T * D), dtype=np.float64, order='C')
    tol = np.mean(np.var(Xc, axis=0)) * 1e-4
    mean = Xc.mean(axis=0)
    Xc -= mean
    seeds = im.kmeans_plusplus_seeds(Xc, K, rs)
    for dtype in (np.float64, LD):
        r = ir.kmeans_lloyd(Xc, seeds, 300, tol, dtype)
        assert not r.emptied
        np.testing.assert_array_equal(r.labels, g[tag + '_labels'][0])
        centers = np.stack([(r.centers[k].astype(np.float64) + mean).reshape(-1, T).T.mean(axis=0) for k in range(K)])
        np.testing.assert_allclose(centers, g[tag + '_centers'], rtol=1e-12, atol=1e-13)
    assert rs.rand() == float(g[tag + '_next_draw'])


# ---- conditions: SMACOF -------------------------------------------------------------------------------------
SMACOF_RUNS, GMDS_RUNS, MLE_RUNS = ir.SMACOF_RUNS, ir.GMDS_RUNS, ir.MLE_RUNS


@pytest.mark.parametrize('name,eps', SMACOF_RUNS, ids=lambda v: str(v))
def test_smacof_case_is_one_the_reference_agrees_with_itself_on(name, eps):
    c = ir.SMACOF_CASES[name]
    r = ir.smacof_reference(name, eps)
    np.testing.assert_array_equal(r.n64, r.nld)
    for crit in r.crit64 + r.critld:
        assert all(abs(float(v) - eps) >= 1e-6 * eps for v in crit)
    scale = np.abs(r.X64).max(axis=(1, 2), keepdims=True)
    assert (np.abs(r.X64.astype(LD) - r.Xld) <= 1e-10 * scale).all()
    tol_X, eps_X, tol_s, eps_s = ir.smacof_tolerances(r)
    print('%s eps %g: n_iter %s, reference eps X %.2e stress %.2e' % (name, eps, r.n64[:6], eps_X, eps_s))
    assert (tol_X <= 1e-8 * scale).all() and (tol_s <= 1e-9 * np.abs(r.s64)).all()
    if eps == 1e-3:      # the runs stop before max_iter, at different iterations, odd and even ones
        assert (r.n64 < c['max_iter']).all() and len(set(r.n64)) == len(r.n64)
        assert (r.n64 % 2 == 1).any() and (r.n64 % 2 == 0).any()
    else:
        assert (r.n64 == c['max_iter']).all()


def test_smacof_case_shapes():
    c = ir.SMACOF_CASES
    assert c['n65_64_starts']['n_init'] == 64                   # dlsm_init_smacof's limit
    for name in c:
        N = c[name]['N']
        assert N > 64 and N % 64 != 0 and N % 4 != 0
        delta = ir.smacof_delta(name)
        assert delta.shape == (N, N) and delta.max() > 2
    assert -(-c['n1030_d2']['N'] // 4) > 256
    X0 = ir.smacof_starts('n130_d2_coincident')
    a, b = c['n130_d2_coincident']['together']
    assert (X0[:, a] == X0[:, b]).all() and ir.smacof_delta('n130_d2_coincident')[a, b] > 0
    Xp = ir.perturbed(X0, 1, together=(a, b))
    assert (Xp[:, a] == Xp[:, b]).all() and (Xp != X0).all()
    assert (np.abs(Xp - X0) <= 4 * np.spacing(np.abs(X0))).all()


def test_smacof_in_one_dimension_has_a_reference_for_one_iteration_only():
    """the table's max_iter of the d = 1 case is the largest the replicas agree at"""
    name = 'n130_d1'
    assert ir.SMACOF_CASES[name]['max_iter'] == 1
    delta, X0 = ir.smacof_delta(name), ir.smacof_starts(name)
    worst = 0.0
    for k in range(X0.shape[0]):
        a = ir.smacof_single(delta, X0[k], 2)[0]
        b = ir.smacof_single(delta, X0[k], 2, dtype=LD)[0]
        worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
    assert worst > 1e-10, worst


# ---- conditions: eigen step ---------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d,lmbda,variant', GMDS_RUNS)
def test_gmds_case_has_separated_eigenvalues(N, d, lmbda, variant):
    _, delta, X_prev = ir.gmds_input(N, d, variant)
    X, evals, w = ir.gmds_reference(N, d, lmbda, variant)
    gaps = (w[:d] - w[1:d + 1]) / w[0]
    print('N %d d %d lambda %g %s: smallest gap %.3f' % (N, d, lmbda, variant, gaps.min()))
    assert gaps.min() >= 0.01 and w[d - 1] > 0
    if variant == 'edgeless':
        assert delta.max() == 1.0 and (delta + np.eye(N) == 1.0).all()
    Xo, eo = io.gmds_step(delta, X_prev, lmbda)
    np.testing.assert_array_equal(X, Xo)
    if lmbda == 0 and N >= 130:     # the case is there for the Gram-Schmidt coefficients of columns 16 and up
        G = ir.gmds_matrix(delta, X_prev, lmbda)
        counts = [ir.lanczos_vectors(G, d, seed) for seed in range(3)]
        print('Lanczos vectors by the replica, three starts: %s' % counts)
        assert min(counts) > 24


# ---- conditions: MLE sums -----------------------------------------------------------------------------------
@pytest.mark.parametrize('key,directed,squared', MLE_RUNS, ids=lambda v: str(v))
def test_mle_case_points_are_what_the_table_says(key, directed, squared):
    T, N, d = key
    Y, X, radii = ir.mle_input(key, directed)
    start, near, extreme = ir.mle_points(key, directed, squared)

    def sums(p):
        if directed:
            return ir.mle_sums_directed(Y, X, radii, p[0], p[1], squared)
        return ir.mle_sums_undirected(Y, X, p[0], p[1], squared)
    ll = [sums(p)[0][0] for p in (start, near, extreme)]
    assert np.isfinite(ll).all() and ll[1] > ll[0] and ll[1] > ll[2]
    # |eta| at the extreme point: past the underflow of exp for part of the dyads, not for all
    dist = np.stack([ir._pairwise(X[t]) for t in range(T)]) ** (2 if squared else 1)
    if directed:
        eta = extreme[0] * (1 - dist / radii[None, None, :]) + extreme[1] * (1 - dist / radii[None, :, None])
    else:
        eta = extreme[1] - np.exp(extreme[0]) * dist
    frac = (np.abs(eta) > 745.2).mean()
    assert 0 < frac < 0.5 and np.abs(eta).max() < 1.01 * ir.ETA_EXTREME + 1
    c = (ir.MLE_DIRECTED if directed else ir.MLE_UNDIRECTED)[key]
    if 'empty' in c:
        assert Y[c['empty']].sum() == 0
    if 'complete' in c:
        assert Y[c['complete']].sum() == N * (N - 1)
    if 'isolated' in c:      # latent_space.py:140-153: the reg path
        raw = 0.5 * (Y.sum(axis=(0, 1)) + Y.sum(axis=(0, 2)))
        assert raw[c['isolated']] == 0 and (radii > 0).all()
        np.testing.assert_array_equal(radii, io.initialize_radii(Y))


def test_mle_case_shapes():
    assert -(-700 // 4) * 6 == 1050 and -(-900 // 4) * 5 == 1125       # records past the final sum's 1024 threads
    assert (6, 700, 2) in ir.MLE_UNDIRECTED and (5, 900, 5) in ir.MLE_DIRECTED
    # the recorded answer of init_oracle.scale_intercept_mle is a stationary point of the oracle's own sums
    Y, X, _ = ir.mle_input((6, 700, 2), False)
    p = ir.MLE_ORACLE_OPTIMUM_6_700_2
    s = io.mle_sums_undirected(Y, X, p[0], p[1])
    _, a = ir.mle_sums_undirected(Y, X, p[0], p[1])
    assert (np.abs(s[1:]) <= 1e-8 * a[1:]).all()


# ---- conditions: Lloyd iterations ---------------------------------------------------------------------------
@pytest.mark.parametrize('key', list(ir.KMEANS_CASES), ids=str)
@pytest.mark.parametrize('stop', ir.KMEANS_STOPS)
def test_kmeans_case_stops_as_the_table_says(key, stop):
    N, F, K = key
    X, seeds, max_iter, tol = ir.kmeans_input(key, stop)
    assert X.shape == (N, F) and seeds.shape == (K, F)
    assert all((X == s).all(axis=1).any() for s in seeds)               # the seeds are data rows
    r, rl = ir.kmeans_lloyd(X, seeds, max_iter, tol), ir.kmeans_lloyd(X, seeds, max_iter, tol, LD)
    assert not r.emptied and not rl.emptied
    assert r.ties == 0 and min(r.min_gap, rl.min_gap) >= 1e-9
    np.testing.assert_array_equal(r.labels, rl.labels)
    assert r.n_iter == rl.n_iter and r.strict == rl.strict
    assert np.abs(r.centers - rl.centers).max() < 1e-13 * np.abs(X).max()
    changed, shift = r.history[-1]
    if stop.startswith('max_iter'):
        assert r.n_iter == max_iter and not r.strict and changed > 0 and shift > tol
    elif stop == 'tol':
        assert not r.strict and 1 < r.n_iter < max_iter and changed > 0 and shift <= tol
        assert min(r.tol_margin, rl.tol_margin) >= 1e-6
    else:
        assert r.strict and changed == 0 and 2 < r.n_iter < max_iter


def test_kmeans_case_shapes_and_ties():
    assert (101 * 80 + 101) * 8 == 65448 <= 64 * 1024 < (102 * 80 + 102) * 8
    X, seeds = ir.kmeans_ties()
    assert (X == np.rint(X)).all()
    r = ir.kmeans_lloyd(X, seeds, 300, 0.0)
    t = ir.TIE_ROWS
    d2 = ((X[:, None, :] - seeds[None]) ** 2).sum(-1)
    assert d2[t['between_0_and_2'], 0] == d2[t['between_0_and_2'], 2] < d2[t['between_0_and_2'], 1]
    for row in t['duplicates_between_1_and_2']:
        assert d2[row, 1] == d2[row, 2] < d2[row, 0]
    assert r.labels[t['between_0_and_2']] == 0 and (r.labels[list(t['duplicates_between_1_and_2'])] == 1).all()
    assert r.ties == 6 and r.n_iter == 1 and not r.strict and not r.emptied
    np.testing.assert_array_equal(r.centers, seeds)


# ---- condition: the pipeline --------------------------------------------------------------------------------
@pytest.mark.parametrize('directed', [False, True])
def test_pipeline_case_has_one_best_start(directed):
    c = ir.PIPELINE_CASE
    Y = ir.pipeline_input(directed)
    rng = np.random.RandomState(c['rs'])
    delta = io.hop_matrix(Y[0])
    stress = sorted(ir.smacof_single(delta, rng.uniform(size=c['N'] * c['d']).reshape(c['N'], c['d']))[1]
                    for _ in range(4))
    assert (stress[1] - stress[0]) > 1e-6 * stress[0]
