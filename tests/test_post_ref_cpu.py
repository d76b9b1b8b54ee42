"""Pins tests/post_ref.py (the long-double replica that tests/test_gpu_post_shapes.py compares the post-loop
kernels with) to the reference's own outputs (tests/golden/post.npz) and to oracle/post_oracle.py at the
shapes of the GPU tests.  Counts are exact; VI values and the forward algorithm agree with the float64
oracle to 1e-13 relative (the replica is the more precise of the two), two orders under the device
tolerances.  No GPU."""
import numpy as np
import pytest

import post_ref as pr
from conftest import load_golden
from oracle import post_oracle as po


@pytest.fixture(scope='module')
def g():
    return load_golden('post.npz')


@pytest.mark.parametrize('tag', ['u', 'd'])
def test_replica_reproduces_the_reference_outputs(g, tag):
    from dynetlsm_amd import posterior as post
    zs, n_burn, K = g[tag + '_zs'], int(g[tag + '_n_burn']), int(g[tag + '_K'])
    kept = zs[n_burn:]
    S = kept.shape[0]
    counts = pr.cooccurrence_counts(kept, K)
    cooc = pr.cooccurrence_probas(counts, S)
    np.testing.assert_array_equal(cooc, g[tag + '_cooc'])
    sums = pr.vi_sums(kept, cooc)
    vis = post.expected_vi(kept, cooc.sum(axis=2), sums.astype(np.float64))
    np.testing.assert_allclose(vis, g[tag + '_vis'], rtol=1e-12)
    np.testing.assert_allclose(pr.assembled_vi(kept, counts).astype(np.float64), g[tag + '_vis'], rtol=1e-12)
    best = int(g[tag + '_best'])
    lm = pr.forward_loglik(g[tag + '_Xs'][best], g[tag + '_init_w'], g[tag + '_trans_w'], g[tag + '_mu_r'],
                           g[tag + '_sigma_r'], g[tag + '_lambdas'][best])
    np.testing.assert_allclose(float(lm), float(g[tag + '_latent_marginal']), rtol=1e-12)
    np.testing.assert_array_equal((pr.label_counts(kept, K) > 0).any(axis=1).sum(axis=1), g[tag + '_counts'])


@pytest.mark.parametrize('case', pr.LABEL_CASES, ids=str)
def test_label_counts_against_the_oracle(case):
    T, N, K, stored, first, count = case
    tr = pr.label_trace(*case)
    nk = pr.label_counts(tr.zs, K)
    assert nk.shape == (stored, T, K) and (nk.sum(axis=2) == N).all()
    np.testing.assert_array_equal((nk > 0).any(axis=1).sum(axis=1), po.cluster_counts(tr.zs, 0))
    np.testing.assert_array_equal((nk > 0).sum(axis=2).T, po.cluster_counts_t(tr.zs, 0))


@pytest.mark.parametrize('case', pr.COOC_CASES, ids=str)
def test_cooccurrence_and_vi_against_the_oracle(case):
    T, N, K, first, count = case
    tr = pr.cooc_trace(*case)
    kept = tr.zs[first:first + count]
    counts = pr.cooccurrence_counts(kept, K)
    ref = po.posterior_cooccurrence(tr.zs[:first + count], first, K)
    np.testing.assert_array_equal(pr.cooccurrence_probas(counts, count), ref)
    assert counts.max() == count and (np.diagonal(counts, axis1=1, axis2=2) == count).all()
    vis = pr.assembled_vi(kept, counts).astype(np.float64)
    want = np.array([po.time_averaged_expected_vi(z, ref) for z in kept])
    np.testing.assert_allclose(vis, want, rtol=1e-13)
    sums = pr.vi_sums(kept, ref)
    assert (sums[:, 0] == sums[:, count - 1]).all()             # the twins


def test_long_trace_counts_against_the_oracle():
    c = pr.LONG_CASE
    tr = pr.synthetic_trace(c['T'], c['N'], c['D'], c['K'], c['stored'], seed=5000)
    kept = tr.zs[c['first']:c['first'] + c['count']]
    counts = pr.cooccurrence_counts(kept, c['K'])
    ref = po.posterior_cooccurrence(tr.zs[:c['first'] + c['count']], c['first'], c['K'])
    np.testing.assert_array_equal(pr.cooccurrence_probas(counts, c['count']), ref)
    assert counts.max() == c['count']
    s = np.array(pr.LONG_VI_SAMPLES)
    vis = pr.vi_sums(kept, ref, samples=s)
    for q, sq in enumerate(s):
        for t in range(c['T']):
            z = kept[sq, t]
            want = sum(np.log2(np.sum((z == z[i]) * ref[t, i])) for i in range(c['N']))   # posterior_vi.py:10-20
            np.testing.assert_allclose(float(vis[t, q]), want, rtol=1e-13)


@pytest.mark.parametrize('case', pr.FORWARD_CASES, ids=str)
def test_forward_algorithm_against_the_oracle_and_finite(case):
    tr, row, init_w, trans_w, mu, sigma, lmbda = pr.forward_case(*case)
    got = pr.forward_loglik(tr.Xs[row], init_w, trans_w, mu, sigma, lmbda)
    assert np.isfinite(got)
    want = po.latent_marginal_loglikelihood(tr.Xs[row], init_w, trans_w, mu, sigma, float(lmbda[0]))
    assert np.isfinite(want)
    np.testing.assert_allclose(float(got), want, rtol=1e-13)
    K = case[3]
    if K == 64:      # the conditions of the component-removal check: finite, and the replica itself passes it
        for k in (K - 1, 0):
            full, less = pr.without_component(k, init_w, trans_w, mu, sigma)
            a = pr.forward_loglik(tr.Xs[row], *full, lmbda)
            b = pr.forward_loglik(tr.Xs[row], *less, lmbda)
            assert np.isfinite(a) and np.isfinite(b)
            np.testing.assert_allclose(float(a), float(b), rtol=1e-14)


def test_select_shape_against_the_oracle():
    c = pr.SELECT_CASE
    tr = pr.select_trace()
    kept = tr.zs[c['n_burn']:]
    counts = pr.cooccurrence_counts(kept, c['K'])
    ref = po.posterior_cooccurrence(tr.zs, c['n_burn'], c['K'])
    np.testing.assert_array_equal(pr.cooccurrence_probas(counts, c['kept']), ref)
    vis = pr.assembled_vi(kept, counts)
    best, want = po.minimize_expected_vi(tr.zs, c['n_burn'], ref, None)
    np.testing.assert_allclose(vis.astype(np.float64), want, rtol=1e-13)
    assert (vis == vis.min()).sum() == 1 and (want == want.min()).sum() == 1     # no tie: no tie-break
    assert best == c['n_burn'] + int(np.argmin(vis))
    assert sorted(np.unique(po.cluster_counts(tr.zs, c['n_burn']))) == list(range(3, 10))


def test_trace_mean_is_the_mean():
    rng = np.random.RandomState(3)
    Xs = rng.randn(200, 2, 5, 3)
    mean, sabs = pr.trace_mean(Xs)
    np.testing.assert_allclose(mean.astype(np.float64), Xs.mean(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(sabs.astype(np.float64), np.abs(Xs).sum(axis=0), rtol=1e-14)
