"""The row words of the undirected log-likelihood pass (csrc/kernels_loglik.hpp: k_loglik_undirected reads the four
64-bit words of a trip of rows with one scalar load, a trip ahead of their use, the diagonal tiles' second triangle
in descending order): ``Chain.loglik_full`` with two intercept candidates against a float64 numpy restatement, at
the smallest shapes where a wrong word, a wrong bit order or a read past a tile can show, and the device loop with
the missing dyads' sampler rewriting the words between the launches.  Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_stats  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-12            # the project's tolerance for the log-likelihood seam


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _symmetric(U):
    U = np.triu(U, 1)
    return (U + U.swapaxes(-1, -2)).astype(np.float64)


def _networks(rng, T, N):
    """name -> (T, N, N) symmetric 0 / 1 network with a zero diagonal"""
    i, j = np.triu_indices(N, 1)
    nets = {'empty': np.zeros((T, N, N)), 'dense': _symmetric(np.ones((T, N, N)))}
    # exactly one edge in every 64-column word of the rows above the diagonal: at its bit 0, at its bit 63
    for name, bit in (('bit0', 0), ('bit63', 63)):
        U = np.zeros((T, N, N))
        cols = np.arange(bit, N, 64)
        for c in cols:
            U[:, :c, c] = 1.0                       # rows i < c pair with column c (the pass reads i < j)
        nets[name] = _symmetric(U)
    nets['random'] = _symmetric(rng.rand(T, N, N) < 0.3)
    return nets


def _distances(X, squared):
    d2 = ((X[:, :, None, :] - X[:, None, :, :]) ** 2).sum(-1)
    return d2 if squared else np.sqrt(d2)


def _loglik_numpy(Y, X, b, squared):
    """sum over t and i < j of y (b - d) - log(1 + exp(b - d)), float64"""
    d = _distances(X, squared)
    N = Y.shape[1]
    iu = np.triu_indices(N, 1)
    eta = b - d[:, iu[0], iu[1]]
    y = Y[:, iu[0], iu[1]]
    return float(np.sum(y * eta) - np.sum(np.logaddexp(0.0, eta)))


CASES = [(D, N, T) for D in (2, 3) for N in (65, 129, 200, 257) for T in (1, 3)]


@pytest.mark.parametrize('D,N,T', CASES)
def test_two_candidates_against_numpy(da, D, N, T):
    """N = 65, 129, 257: the last column block holds one column, one or two diagonal tiles + a partial third;
    N = 200: the second tile row's rows run past N.  Every network at plain and at squared distances."""
    rng = np.random.RandomState(1000 * D + 10 * N + T)
    X = rng.randn(T, N, D) * (1.5 / np.sqrt(D))
    cands = np.array([[0.7], [-0.4]])
    # exp(b) underflows to zero below -745: the candidates' sums of log(1 + exp(b - d)) vanish and
    # ll(b) = b sum(Y) - sum(Y d), so ll(-800) - ll(-801) is the edge count the pass took from the words
    far = np.array([[-800.0], [-801.0]])
    with da.Chain(T, N, D, 'undirected') as c:
        c.set_positions(X)
        c.set_intercepts(np.array([0.1]))
        for name, Y in sorted(_networks(rng, T, N).items()):
            c.upload_network(Y)
            n_edges = int(Y.sum()) // 2
            for squared in (False, True):
                c.set_squared(squared)
                got = c.loglik_full(cands)
                want = np.array([_loglik_numpy(Y, X, b, squared) for b in cands[:, 0]])
                lf = c.loglik_full(far)
                print('%-6s squared=%d edges %d  ll %r  numpy %r  count %r'
                      % (name, squared, n_edges, got.tolist(), want.tolist(), lf[0] - lf[1]))
                # (each value carries the rounding of a number of size 801 sum(Y) + sum(Y d) < 2^28: 3e-8 at most)
                assert abs((lf[0] - lf[1]) - n_edges) < 1e-6 and int(np.rint(lf[0] - lf[1])) == n_edges, (name, squared)
                np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg='%s squared=%d' % (name, squared))
                if name == 'empty':
                    assert lf[0] == 0.0 and lf[1] == 0.0
        c.set_squared(False)


def _read_packed(c):
    n = c.network_packed_words()
    buf = np.zeros(n, dtype=np.uint32)
    c.get_network_packed(buf.ctypes.data, n)
    return buf


def _loop_chain(da, Y, X, ic, index, n_total):
    T, N, D = X.shape
    c = da.Chain(T, N, D, 'undirected', seed=20260, chain_id=2)
    c.upload_network(Y)
    c.set_positions(X)
    c.set_intercepts(ic)
    c.set_prior_random_walk(TAU_SQ, SIGMA_SQ)
    c.set_samplers(da.SamplerGrid(T, N, 0.05, tune=4, tune_interval=2))
    c.lsm_configure(ic, IC_VAR, step_size_intercept=0.1, tune=4, tune_interval=2, n_iter_procrustes=0, sweep_algo=4)
    c.trace_alloc(n_total, logp0=0.0)
    c.set_missing(index)
    c.missing_sampling(True, accumulate_after=0)
    return c


TAU_SQ, SIGMA_SQ, IC_VAR = 2.0, 0.1, 2.0


def test_loop_reads_the_words_the_sampler_left(da, monkeypatch):
    """T = 2, N = 520, d = 2, three iterations of the device loop with the missing dyads re-drawn at the end of
    every iteration: the pass of iteration it must see the words as iteration it - 1 left them (a kernel boundary
    lies between the writer and the scalar loads).  The stored log-posterior of every iteration against the
    log-likelihood of the stored positions on the words read back BEFORE that iteration - by ``loglik_full`` on a
    fresh chain and by numpy - plus the priors restated on the host; and the three iterations in one ``lsm_run``
    give the same trace bit for bit."""
    from dynetlsm_amd.lsm import latent_prior_terms
    from dynetlsm_amd.model_selection import train_test_split
    monkeypatch.delenv('DLSM_GRAPH', raising=False)
    T, N, D, n_total = 2, 520, 2, 4
    rng = np.random.RandomState(520)
    Y = _symmetric(rng.rand(T, N, N) < 0.1)
    X = rng.randn(T, N, D) * (1.5 / np.sqrt(D))
    ic = np.array([0.4])
    _, index = train_test_split(np.zeros((T, N, N)), 0.1, random_state=rng, is_directed=False)
    W = gof_stats.row_words(N)
    before, rows = [], []
    with _loop_chain(da, Y, X, ic, index, n_total) as c:
        for it in range(1, n_total):
            before.append(_read_packed(c))
            c.lsm_run(it, 1)
            rows.append(c.trace_read(it, 1))
        single = c.trace_read(0, n_total)
    with _loop_chain(da, Y, X, ic, index, n_total) as c:
        c.lsm_run(1, n_total - 1)
        ranged = c.trace_read(0, n_total)
    for name, a, b in zip(('positions', 'intercepts', 'log-posteriors'), single, ranged):
        assert np.array_equal(a, b), name
    assert not np.array_equal(before[0], before[1]) and not np.array_equal(before[1], before[2]), \
        'the sampler never changed the network'
    with da.Chain(T, N, D, 'undirected') as f:
        for k, (buf, (Xs, ics, lps)) in enumerate(zip(before, rows)):
            b = float(ics[0, 0])
            f.set_network_packed(buf.ctypes.data, buf.shape[0])
            f.set_positions(Xs[0])
            ll = f.loglik_full(np.array([[b], [b + 0.25]]))[0]
            Yk = gof_stats.unpack(buf.reshape(T, N, W), N).astype(np.float64)
            ll_np = _loglik_numpy(Yk, Xs[0], b, False)
            prior = latent_prior_terms(Xs[0], TAU_SQ, SIGMA_SQ) - 0.5 * (b - ic[0]) ** 2 / IC_VAR
            print('iteration %d: stored %r  loglik_full + priors %r  numpy + priors %r'
                  % (k + 1, float(lps[0]), ll + prior, ll_np + prior))
            np.testing.assert_allclose(ll, ll_np, rtol=RTOL, atol=0)
            np.testing.assert_allclose(lps[0], ll + prior, rtol=RTOL, atol=0)
            np.testing.assert_allclose(lps[0], ll_np + prior, rtol=RTOL, atol=0)
            if k > 0:       # on the words of one iteration earlier the value is another one
                f.set_network_packed(before[k - 1].ctypes.data, before[k - 1].shape[0])
                stale = f.loglik_full(np.array([[b], [b + 0.25]]))[0]
                assert abs(stale - ll) > 1e-9 * abs(ll)
