"""The post-loop kernels (csrc/kernels_post.hpp) over the device-resident trace, value for value against
the long-double replica tests/post_ref.py (pinned to the oracle and to the reference's outputs by
tests/test_post_ref_cpu.py) at the smallest shapes that cross each of their boundaries: more than one tile,
chunk, wavefront or workgroup, ragged last ones, n_features 1..8, 1..64 components, a trace longer than
a grid's y extent and host labels staged in two chunks.  Needs an MI355X: -m gpu.

Integers (label counts, co-occurrence counts and the probabilities count / n_samples) are exact; VI sums
hold to 1e-12 and the forward algorithm to 1e-11 relative (the tolerances of test_gpu_post.py); row sums
and posterior means are bounded by the roundings their kernels make."""
from types import SimpleNamespace

import numpy as np
import pytest

import post_ref as pr
from oracle import post_oracle as po

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    return dynetlsm_amd


def _trace_chain(eng, tr):
    """a chain whose device-resident trace holds the synthetic trace ``tr``"""
    from dynetlsm_amd import hdp_updates as hu
    c = eng.Chain(tr.T, tr.N, tr.D, 'undirected')
    c.upload_network(tr.Y); c.set_positions(tr.Xs[0]); c.set_intercepts([float(tr.intercepts[0, 0])])
    c.set_samplers(eng.SamplerGrid(tr.T, tr.N, 0.1, tune=None))
    c.set_prior_mixture(tr.mus[0], tr.sigmas[0], float(tr.lambdas[0, 0]), tr.zs[0])
    c.hdp_configure(hu.HDPHyper(tr.K), tr.betas[0], tr.weights[0], 0.5, 2.0)
    c.hdp_trace_alloc(tr.S, logp0=float(tr.logps[0]))
    c.hdp_trace_write(0, Xs=tr.Xs, intercepts=tr.intercepts, logps=tr.logps, mus=tr.mus, sigmas=tr.sigmas,
                      zs=tr.zs, betas=tr.betas, weights=tr.weights, lambdas=tr.lambdas)
    return c


def _bincounts(zs, K):
    return np.stack([[np.bincount(zs[s, t], minlength=K) for t in range(zs.shape[1])]
                     for s in range(zs.shape[0])])


def _assert_row_sums(rs, cooc, N):
    """|got - ref| <= (ceil(N / 64) + 6) 2^-53 sum_j C[i][j]: ceil(N / 64) sequential adds per lane, then the
    six levels of the wavefront's sum; never looser than the 1e-13 relative of test_gpu_post.py"""
    ref = cooc.astype(pr.LD).sum(axis=2)
    bound = np.minimum((-(-N // 64) + 6) * U, 1e-13) * ref
    err = np.abs(rs.astype(pr.LD) - ref)
    print('row sums: max err / bound', float((err / bound).max()))
    assert (err <= bound).all()


def _assert_mean(got, Xs_kept):
    """per element (ceil(count / 64) + 64) 2^-53 sum_s |x_s| / count - the strided partial sums of 64 chunks,
    then their sum - plus the rounding of the division"""
    count = Xs_kept.shape[0]
    ref, sabs = pr.trace_mean(Xs_kept)
    bound = (-(-count // 64) + 64) * U * sabs / count + U * np.abs(ref)
    err = np.abs(got.astype(pr.LD) - ref)
    print('mean: max err / bound', float((err / bound).max()))
    assert (err <= bound).all()


# ---- label counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pr.LABEL_CASES, ids=str)
def test_label_counts(eng, case):
    T, N, K, stored, first, count = case
    tr = pr.label_trace(*case)
    with _trace_chain(eng, tr) as c:
        nk = c.post_trace_label_counts(first, count)
    np.testing.assert_array_equal(nk, _bincounts(tr.zs[first:first + count], K))


@pytest.mark.parametrize('which', ['first', 'last'])
def test_label_counts_one_label_for_every_node(eng, which):
    T, N, K, stored, first, count = case = pr.LABEL_CASES[2]
    tr = pr.label_trace(*case)
    tr.zs[:] = 0 if which == 'first' else K - 1
    with _trace_chain(eng, tr) as c:
        nk = c.post_trace_label_counts(first, count)
    np.testing.assert_array_equal(nk, _bincounts(tr.zs[first:first + count], K))
    assert nk[:, :, 0 if which == 'first' else K - 1].min() == N


# ---- co-occurrence, row sums, VI sums ----------------------------------------------------------------------
@pytest.mark.parametrize('case', pr.COOC_CASES, ids=str)
def test_trace_cooccurrence_row_sums_and_vi(eng, case):
    T, N, K, first, count = case
    tr = pr.cooc_trace(*case)
    kept = tr.zs[first:first + count]
    want = pr.cooccurrence_probas(pr.cooccurrence_counts(kept, K), count)
    with _trace_chain(eng, tr) as c:
        cooc, rs = c.post_trace_cooccurrence(first, count, want_matrix=True)
        held = c.post_get_cooccurrence()
        sums = c.post_expected_vi_sums()
    np.testing.assert_array_equal(cooc, want)
    np.testing.assert_array_equal(held, want)
    _assert_row_sums(rs, want, N)
    assert sums.shape == (T, count)
    np.testing.assert_allclose(sums, pr.vi_sums(kept, want).astype(np.float64), rtol=1e-12)
    assert (sums[:, 0] == sums[:, count - 1]).all()             # identical samples: bitwise equal


# ---- a trace longer than a grid's y extent -----------------------------------------------------------------
def test_long_trace(eng):
    c_ = pr.LONG_CASE
    T, N, K, first, count = c_['T'], c_['N'], c_['K'], c_['first'], c_['count']
    tr = pr.synthetic_trace(T, N, c_['D'], K, c_['stored'], seed=5000)
    tr.Xs[:first] = 1e6
    kept = tr.zs[first:first + count]
    counts = pr.cooccurrence_counts(kept, K)
    want = pr.cooccurrence_probas(counts, count)
    assert counts.max() == count
    with _trace_chain(eng, tr) as c:
        nk = c.post_trace_label_counts(first, count)
        cooc, rs = c.post_trace_cooccurrence(first, count, want_matrix=True)
        sums = c.post_expected_vi_sums()
        mean = c.post_trace_mean(first, count)
    np.testing.assert_array_equal(nk, _bincounts(kept, K))
    np.testing.assert_array_equal(cooc, want)
    _assert_row_sums(rs, want, N)
    _assert_mean(mean, tr.Xs[first:first + count])
    s = np.array(pr.LONG_VI_SAMPLES)
    np.testing.assert_allclose(sums[:, s], pr.vi_sums(kept, want, samples=s).astype(np.float64), rtol=1e-12)


# ---- posterior mean of the trace ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mean_chain(eng):
    T, N, D = pr.MEAN_SHAPE
    tr = pr.synthetic_trace(T, N, D, 2, pr.MEAN_FIRST + max(pr.MEAN_COUNTS), seed=6000)
    tr.Xs[:pr.MEAN_FIRST] = 1e6                                  # an offset error shows
    with _trace_chain(eng, tr) as c:
        yield c, tr


@pytest.mark.parametrize('count', pr.MEAN_COUNTS)
def test_trace_mean(mean_chain, count):
    c, tr = mean_chain
    got = c.post_trace_mean(pr.MEAN_FIRST, count)
    _assert_mean(got, tr.Xs[pr.MEAN_FIRST:pr.MEAN_FIRST + count])


# ---- forward algorithm -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pr.FORWARD_CASES, ids=str)
def test_forward_algorithm(eng, case):
    T, N, D, K = case
    tr, row, init_w, trans_w, mu, sigma, lmbda = pr.forward_case(*case)
    want = float(pr.forward_loglik(tr.Xs[row], init_w, trans_w, mu, sigma, lmbda))
    p = np.random.RandomState(K).permutation(K)
    with _trace_chain(eng, tr) as c:
        got = c.post_latent_marginal_loglik(init_w, trans_w, mu, sigma, lmbda, row=row)
        perm = c.post_latent_marginal_loglik(init_w[p], trans_w[:, p][:, :, p], mu[p], sigma[p], lmbda, row=row)
        removed = []
        if K == 64:
            for k in (K - 1, 0):
                full, less = pr.without_component(k, init_w, trans_w, mu, sigma)
                removed.append((c.post_latent_marginal_loglik(*full, lmbda, row=row),
                                c.post_latent_marginal_loglik(*less, lmbda, row=row),
                                float(pr.forward_loglik(tr.Xs[row], *less, lmbda))))
        c.set_positions(tr.Xs[row])                              # row = -1: the chain's current positions
        current = c.post_latent_marginal_loglik(init_w, trans_w, mu, sigma, lmbda)
    print('forward: got %.17g want %.17g' % (got, want))
    np.testing.assert_allclose(got, want, rtol=1e-11)
    assert current == got
    # relabelling the components moves nothing but roundings
    np.testing.assert_allclose(perm, got, rtol=1e-12)
    # a component without mass is no component: the K - 1 value of the same parameters
    for full, less, ref in removed:
        np.testing.assert_allclose(full, ref, rtol=1e-12)
        np.testing.assert_allclose(full, less, rtol=1e-12)


# ---- host labels staged in two chunks ----------------------------------------------------------------------
def test_host_labels_over_two_staging_chunks(eng):
    c_ = pr.STAGED_CASE
    T, N, K, S = c_['T'], c_['N'], c_['K'], c_['S']
    assert (64 << 20) // (T * N * 8) == 131072 < S              # the second chunk lands at s0 = 131072
    zs = pr.synthetic_trace(T, N, 1, K, S, seed=7000).zs
    want = pr.cooccurrence_probas(pr.cooccurrence_counts(zs, K), S)
    with eng.Chain(T, N, 1, 'undirected') as c:
        cooc = c.post_cooccurrence(zs, K)
        sums = c.post_expected_vi_sums()
        c.post_release()
    np.testing.assert_array_equal(cooc, want)
    s = np.array(pr.STAGED_VI_SAMPLES)
    np.testing.assert_allclose(sums[:, s], pr.vi_sums(zs, want, samples=s).astype(np.float64), rtol=1e-12)


# ---- select_model_device at a shape that is not the golden one ---------------------------------------------
@pytest.fixture(scope='module')
def select_ref():
    c_ = pr.SELECT_CASE
    tr = pr.select_trace()
    n_burn = c_['n_burn']
    cooc = po.posterior_cooccurrence(tr.zs, n_burn, c_['K'])
    best, vis = po.minimize_expected_vi(tr.zs, n_burn, cooc, None)
    replica = pr.assembled_vi(tr.zs[n_burn:], pr.cooccurrence_counts(tr.zs[n_burn:], c_['K']))
    assert (replica == replica.min()).sum() == 1 and int(np.argmin(replica)) + n_burn == best   # no tie
    return SimpleNamespace(tr=tr, n_burn=n_burn, cooc=cooc, best=int(best), vis=vis,
                           counts=po.cluster_counts(tr.zs, n_burn), counts_t=po.cluster_counts_t(tr.zs, n_burn))


@pytest.mark.parametrize('selection_type', ['vi', 'bic', 'map'])
def test_select_model_device(eng, select_ref, selection_type):
    from dynetlsm_amd import posterior as post
    from oracle import oracle as orc
    r, tr, n_burn = select_ref, select_ref.tr, select_ref.n_burn
    T, N, D = tr.T, tr.N, tr.D
    m = SimpleNamespace(Y_fit_=tr.Y, logps_=tr.logps, n_components=tr.K, n_features=D, is_directed=False,
                        selection_type=selection_type)
    with _trace_chain(eng, tr) as c:
        post.select_model_device(m, c, n_burn)
        cooc = c.post_get_cooccurrence()
    np.testing.assert_array_equal(cooc, r.cooc)
    np.testing.assert_array_equal(m.counts_, r.counts)
    np.testing.assert_array_equal(m._counts_t, r.counts_t)
    # the BIC table (approx_bic.py:79-162): one row per model size in use, its MAP sample, and in it the
    # forward algorithm at that sample's renormalised parameters
    sizes = np.unique(r.counts)
    np.testing.assert_array_equal(m.bic_[:, 0], sizes)
    off = np.sum(tr.Y) - np.einsum('ikk', tr.Y).sum()
    want_bic = []
    for (k, bic_k, loglik_k, map_id), mod in zip(m.bic_, m.models_):
        want_id = n_burn + int(np.argmax(np.where(r.counts == k, tr.logps[n_burn:], -np.inf)))
        assert int(map_id) == want_id
        np.testing.assert_array_equal(mod.X, tr.Xs[want_id])
        n_params = (D + 1) * k + (k - 1) + (k - 1) + (T - 1) * k * (k - 1)
        lm = (-bic_k - 2 * loglik_k + np.log(0.5 * off) + n_params * np.log(N * T)) / 2
        ref = float(pr.forward_loglik(mod.X, mod.init_weights, mod.trans_weights, mod.mu, mod.sigma, mod.lmbda))
        np.testing.assert_allclose(lm, ref, rtol=1e-11)
        ll = orc.dynamic_network_loglikelihood_undirected(tr.Y, tr.Xs[want_id], tr.intercepts[want_id, 0])
        np.testing.assert_allclose(loglik_k, ll, rtol=1e-9)
        want_bic.append(-2 * ll + np.log(0.5 * off) - 2 * ref + n_params * np.log(N * T))
    np.testing.assert_allclose(m.bic_[:, 1], want_bic, rtol=1e-9)
    if selection_type == 'vi':
        np.testing.assert_allclose(m.expected_vis_, r.vis, rtol=1e-12)
        assert m.selected_id_ == r.best
        np.testing.assert_array_equal(m.X_, tr.Xs[r.best])
    elif selection_type == 'bic':
        assert m.selected_id_ == int(m.bic_[int(np.argmin(want_bic)), 3])
    else:
        best_k = int(np.argmax(np.bincount(r.counts)))
        assert m.best_k_ == best_k
        assert m.selected_id_ == int(m.bic_[list(sizes).index(best_k), 3])
