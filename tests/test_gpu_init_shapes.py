"""The initialisation kernels (csrc/kernels_init.hpp) through ``Chain.init_*``, value for value against the
long-double replica tests/init_ref.py (pinned to the oracle and to the reference's outputs, and every case held
to its conditions, by tests/test_init_ref_cpu.py) at the smallest shapes that cross each of their boundaries:
a wavefront's second and third trip over a row, a last workgroup with two live rows, 64 concurrent SMACOF
runs that stop at different iterations, more than 256 workgroup records of a SMACOF pass, more than 16 Lanczos
vectors to orthogonalise against, more than 1024 records of the MLE sums, a second workgroup of samples and
the last cluster count that fits the assignment kernel's LDS.  Needs an MI355X: -m gpu.

Tolerances: iteration counts and labels are exact.  SMACOF holds to ic_ref.tolerance's rule, 16 eps + 4 ulp
with eps the reference's own error on the input, never looser than test_gpu_init.py's 1e-8 of the scale (X)
and 1e-9 (stress); the eigen step to test_gpu_init.py's 1e-10 (eigenvalues) and 1e-8 of the scale (X); the
MLE sums and the centres to bounds derived from the additions the kernels make (init_ref.mle_sum_bound,
init_ref.center_bound)."""
import time

import numpy as np
import pytest

import init_ref as ir
from oracle import init_oracle as io
from init_ref import GMDS_RUNS, MLE_RUNS, SMACOF_RUNS

pytestmark = pytest.mark.gpu
LD = ir.LD


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    from dynetlsm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, 'no HIP device: the engine has no CPU path'
    return dynetlsm_amd


def _chain(eng, Y, D, directed=False):
    T, N, _ = Y.shape
    c = eng.Chain(T, N, D, 'directed' if directed else 'undirected', seed=7)
    c.upload_network(Y)
    return c


# ---- SMACOF ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,eps', SMACOF_RUNS, ids=lambda v: str(v))
def test_smacof(eng, name, eps):
    c = ir.SMACOF_CASES[name]
    t0 = time.time()
    r = ir.smacof_reference(name, eps)
    t_ref = time.time() - t0
    delta, X0 = ir.smacof_delta(name), ir.smacof_starts(name)
    with _chain(eng, ir.smacof_network(name), c['d']) as ch:
        ch.init_shortest_paths()
        np.testing.assert_array_equal(ch.init_get_dissimilarity(0), delta)
        X, stress, n_iter = ch.init_smacof(0, X0, max_iter=c['max_iter'], eps=eps)
    tol_X, eps_X, tol_s, eps_s = ir.smacof_tolerances(r)
    err_X, err_s = np.abs(X - r.X64), np.abs(stress - r.s64)
    print('%s eps %g: n_iter %s want %s | X eps %.3e max err %.3e max err/tol %.3f | stress eps %.3e max err %.3e '
          'max err/tol %.3f | reference %.1f s' % (name, eps, n_iter[:6], r.n64[:6], eps_X, err_X.max(),
                                                   (err_X / tol_X).max(), eps_s, err_s.max(), (err_s / tol_s).max(), t_ref))
    np.testing.assert_array_equal(n_iter, r.n64)
    assert (err_X <= tol_X).all(), (name, eps_X, float(err_X.max()))
    assert (err_s <= tol_s).all(), (name, eps_s, float(err_s.max()))


def test_smacof_refuses_a_65th_start(eng):
    name = 'n65_64_starts'
    with _chain(eng, ir.smacof_network(name), 2) as ch:
        ch.init_shortest_paths()
        with pytest.raises(eng.EngineError):
            ch.init_smacof(0, np.zeros((65, 65, 2)), max_iter=1)


# ---- eigen step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,d,lmbda,variant', GMDS_RUNS)
def test_gmds_step(eng, N, d, lmbda, variant):
    Y, delta, X_prev = ir.gmds_input(N, d, variant)
    Xo, eo, _ = ir.gmds_reference(N, d, lmbda, variant)
    with _chain(eng, Y, d) as ch:
        ch.init_shortest_paths()
        np.testing.assert_array_equal(ch.init_get_dissimilarity(1), delta)
        X, evals, info = ch.init_gmds_step(1, X_prev, lmbda=lmbda)
    err_e, err_X = np.abs(evals / eo - 1).max(), np.abs(X - Xo).max() / np.abs(Xo).max()
    print('N %d d %d lambda %g %s: %d vectors, residual %.2e, evals rel err %.3e, X err / scale %.3e'
          % (N, d, lmbda, variant, info['n_lanczos'], info['residual'], err_e, err_X))
    assert info['residual'] <= 1e-12
    np.testing.assert_allclose(evals, eo, rtol=1e-10)
    assert err_X < 1e-8, info
    if lmbda == 0 and N >= 130:     # the coefficient loop's second round: columns 16 and up
        assert info['n_lanczos'] > 24, info
    if variant == 'edgeless':       # the Krylov space ends after about d + 1 vectors
        assert info['n_lanczos'] <= 16, info


def test_gmds_step_that_runs_out_of_vectors(eng):
    (N, d), lmbda, limits = ir.GMDS_UNCONVERGED
    from dynetlsm_amd import initialization as im
    Y, delta, X_prev = ir.gmds_input(N, d)
    w = ir.gmds_reference(N, d, lmbda)[2]
    with _chain(eng, Y, d) as ch:
        ch.init_shortest_paths()
        for m in limits:
            X, evals, info = ch.init_gmds_step(1, X_prev, lmbda=lmbda, max_lanczos=m)
            off = np.abs(evals[:, None] - w[None, :]).min(axis=1)
            print('max_lanczos %d: residual %.3e, Ritz values off by %s of max |theta|'
                  % (m, info['residual'], off / np.abs(evals).max()))
            assert info['residual'] > 1e-12 and info['n_lanczos'] == m
            assert np.isfinite(X).all()
            assert (off <= info['residual'] * np.abs(evals).max()).all()
        with pytest.raises(eng.EngineError, match='max_lanczos'):
            ch.init_gmds_step(1, X_prev, lmbda=lmbda, max_lanczos=d - 1)
        with pytest.warns(UserWarning, match='Lanczos residual'):
            im.generalized_mds(ch, lmbda=lmbda, random_state=np.random.RandomState(0), max_lanczos=limits[0])


# ---- MLE sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,directed,squared', MLE_RUNS, ids=lambda v: str(v))
def test_mle_sums(eng, key, directed, squared):
    T, N, d = key
    Y, X, radii = ir.mle_input(key, directed)
    worst = 0.0
    with _chain(eng, Y, d, directed) as ch:
        ch.set_positions(X)
        if directed:
            ch.set_radii(radii)
        ch.set_squared(int(squared))
        for what, p in zip(('start', 'near optimum', 'extreme'), ir.mle_points(key, directed, squared)):
            got = ch.init_mle_sums(p[0], p[1])
            if directed:
                ref, a = ir.mle_sums_directed(Y, X, radii, p[0], p[1], squared, LD)
            else:
                ref, a = ir.mle_sums_undirected(Y, X, p[0], p[1], squared, LD)
            bound = np.minimum(ir.mle_sum_bound(T, N, a), 1e-10 * np.abs(ref) + 1e-9)
            err = np.abs(got.astype(LD) - ref)
            print('%s %s squared %d, %s %s: err / bound %s' % ('directed' if directed else 'undirected', key, squared,
                                                              what, p, (err / bound).astype(np.float64)))
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(got).all()
            assert (err <= bound).all(), (what, got, ref.astype(np.float64))
    print('worst err / bound %.3f' % worst)


def test_conditional_mles_past_1024_records(eng):
    """the BFGS facades against init_oracle's: the undirected one at (6, 700, 2) against the oracle's recorded
    answer (its run takes a minute on the host; test_init_ref_cpu.py holds the record to be a stationary point
    of the oracle's sums), the directed one with the radii's reg path against the oracle run here"""
    from dynetlsm_amd import initialization as im
    key = (6, 700, 2)
    Y, X, _ = ir.mle_input(key, False)
    with _chain(eng, Y, 2) as ch:
        got = im.scale_intercept_mle(ch, X)
    np.testing.assert_allclose(got, ir.MLE_ORACLE_OPTIMUM_6_700_2, rtol=1e-5, atol=1e-6)
    key = (2, 130, 2)
    Y, X, radii = ir.mle_input(key, True)
    with _chain(eng, Y, 2, True) as ch:
        got = im.directed_intercept_mle(ch, X, radii)
    with np.errstate(over='ignore'):        # the oracle's 1 / (1 + exp(-eta)) on the isolated node's dyads
        want = io.directed_intercept_mle(Y, X, radii)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


# ---- Lloyd iterations --------------------------------------------------------------------------------------
def _assert_lloyd(eng, X, seeds, max_iter, tol, label):
    r = ir.kmeans_lloyd(X, seeds, max_iter, tol, LD)
    with eng.Chain(1, 8, 2, 'undirected') as ch:
        cen, lab, nit = ch.init_kmeans_lloyd(X, seeds, max_iter=max_iter, tol=tol)
    np.testing.assert_array_equal(lab, r.labels)
    assert nit == r.n_iter
    bound = ir.center_bound(X, r.members, r.centers)
    err = np.abs(cen.astype(LD) - r.centers)
    print('%s: n_iter %d, centres max err / bound %.3f' % (label, nit, float((err / bound).max())))
    assert (err <= bound).all()
    return r, cen, lab


@pytest.mark.parametrize('key', list(ir.KMEANS_CASES), ids=str)
@pytest.mark.parametrize('stop', ir.KMEANS_STOPS)
def test_kmeans_lloyd(eng, key, stop):
    X, seeds, max_iter, tol = ir.kmeans_input(key, stop)
    _assert_lloyd(eng, X, seeds, max_iter, tol, '%s %s' % (key, stop))


def test_kmeans_lloyd_refuses_centres_past_the_lds(eng):
    X, _, _, _ = ir.kmeans_input((300, 80, 101))
    with eng.Chain(1, 8, 2, 'undirected') as ch:
        with pytest.raises(eng.EngineError, match='centres'):
            ch.init_kmeans_lloyd(X, X[:102].copy(), max_iter=2, tol=0.0)


def test_kmeans_lloyd_exact_ties(eng):
    X, seeds = ir.kmeans_ties()
    r, cen, lab = _assert_lloyd(eng, X, seeds, 300, 0.0, 'ties')
    t = ir.TIE_ROWS
    assert lab[t['between_0_and_2']] == 0
    assert (lab[list(t['duplicates_between_1_and_2'])] == 1).all()
    np.testing.assert_array_equal(cen, seeds)


# ---- the pipeline at a middle size -------------------------------------------------------------------------
@pytest.mark.parametrize('directed', [False, True])
def test_generalized_mds_at_a_middle_size(eng, directed):
    from dynetlsm_amd import initialization as im
    c = ir.PIPELINE_CASE
    Y = ir.pipeline_input(directed)
    rs, rs_o = np.random.RandomState(c['rs']), np.random.RandomState(c['rs'])
    with _chain(eng, Y, c['d'], directed) as ch:
        X = im.generalized_mds(ch, is_directed=directed, random_state=rs)
    Xo = io.generalized_mds(Y, n_features=c['d'], is_directed=directed, rng=rs_o)
    err = np.abs(X - Xo).max() / np.abs(Xo).max()
    print('pipeline directed %d: err / scale %.3e' % (directed, err))
    assert err < 2e-6
    assert rs.rand() == rs_o.rand()
