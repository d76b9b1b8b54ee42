"""Information criteria on the device (csrc/kernels_ic.hpp, dynetlsm_amd/ic.py) against the host
restatement tests/ic_ref.py.  Needs an MI355X: -m gpu.

The tolerance of a comparison with ic_ref is not a constant: ic_ref is evaluated in float64 and in
np.longdouble, eps = max |float64 - longdouble| over the output array is the reference's own rounding
error on that input, and the device gets 16 eps + 4 ulp of the value (a different but fixed summation
order and the device's exp / log, each within a few ulp: one order of magnitude, no more)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ic_ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_gof import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _case(rng, S, T, N, D, directed, density=0.2, scale=1.5):
    Xs = rng.randn(S, T, N, D) * (scale / np.sqrt(D))
    ic = np.stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    idx = np.arange(N)
    Y[:, idx, idx] = 0
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.transpose(0, 2, 1)
    return Y, Xs, ic, radii


def _reference(Y, Xs, ic, radii, directed, want_pointwise=True):
    r64 = ic_ref.accumulate(Y, Xs, ic, radii, directed, np.float64, want_pointwise)
    rld = ic_ref.accumulate(Y, Xs, ic, radii, directed, np.longdouble, want_pointwise)
    return r64, rld


def _check(got, ref, label=''):
    """device outputs (totals, sample_loglik[, pointwise]) within 16 eps + 4 ulp of ic_ref; returns the eps"""
    r64, rld = ref
    eps_all = []
    for name, g, a, b in zip(('totals', 'sample_loglik', 'pointwise'), got, r64, rld):
        if a is None:
            continue
        assert np.isfinite(g).all(), (label, name)
        tol, eps = ic_ref.tolerance(a, b)
        err = np.abs(g - a)
        worst = float((err / tol).max())
        print('%s %-13s eps %.3e  max err %.3e  max err/tol %.3f' % (label, name, eps, err.max(), worst))
        assert (err <= tol).all(), (label, name, eps, float(err.max()), worst)
        eps_all.append(eps)
    return eps_all


def _loglik_full(c, Y, Xs, ic, radii, s):
    c.set_positions(Xs[s])
    c.set_intercepts(ic[s] if radii is not None else ic[s, :1])
    if radii is not None:
        c.set_radii(radii[s])
    return c.loglik_full()


@pytest.mark.parametrize('T,N,D,directed', CASES)
def test_outputs_against_the_reference_on_the_shape_grid(da, T, N, D, directed):
    rng = np.random.RandomState(N * 16 + D + 8 * directed)
    Y, Xs, ic, radii = _case(rng, 17, T, N, D, directed, density=0.2 if N < 1000 else 0.03)
    bits = da.engine.pack_network(Y)
    rtol_full = 1e-12 if N < 2000 else 1e-10
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        c.upload_network(Y)
        for S in (1, 2, 17):
            r = radii[:S] if directed else None
            got = c.ic_accumulate(bits, Xs[:S], ic[:S], r, want_pointwise=True)
            _check(got, _reference(Y, Xs[:S], ic[:S], r, directed), 'N=%d D=%d dir=%d S=%d' % (N, D, directed, S))
            totals, sl, pw = got
            n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
            assert (totals[:, 4] == n_dyads).all()
            if not directed:
                assert not pw[:, np.tril_indices(N)[0], np.tril_indices(N)[1]].any()
            # the per-sample network log-likelihood is the chain's own full pass
            for s in sorted({0, S - 1}):
                want = _loglik_full(c, Y, Xs, ic, r, s)
                assert abs(sl[s].sum() - want) <= rtol_full * abs(want), (S, s, sl[s].sum(), want)


@pytest.mark.parametrize('directed', [False, True])
def test_one_sample_repeated_samples_and_permutations(da, directed):
    rng = np.random.RandomState(3 + directed)
    T, N, D, S = 3, 65, 2, 17
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    bits = da.engine.pack_network(Y)
    sub = (lambda idx: radii[idx]) if directed else (lambda idx: None)
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        # S = 1: no variance, and lppd is the log-likelihood
        t1, s1, p1 = c.ic_accumulate(bits, Xs[:1], ic[:1], sub(slice(0, 1)), want_pointwise=True)
        assert (p1[..., 1] == 0).all() and (t1[:, 1] == 0).all()
        np.testing.assert_allclose(t1[:, 0], s1[0], rtol=1e-13)
        np.testing.assert_array_equal(t1[:, 0], t1[:, 2])
        # S copies of one sample: var within the reference's error, lppd unchanged
        rep = np.zeros(S, dtype=int)
        got = c.ic_accumulate(bits, Xs[rep], ic[rep], sub(rep), want_pointwise=True)
        ref = _reference(Y, Xs[rep], ic[rep], sub(rep), directed)
        eps = _check(got, ref, 'repeated dir=%d' % directed)
        assert got[2][..., 1].max() <= eps[2]
        tol, _ = ic_ref.tolerance(ref[0][2][..., 0], ref[1][2][..., 0])
        assert (np.abs(got[2][..., 0] - p1[..., 0]) <= tol).all()
        # a permutation of the samples: every output within the same tolerance
        perm = rng.permutation(S)
        a = c.ic_accumulate(bits, Xs, ic, radii, want_pointwise=True)
        b = c.ic_accumulate(bits, Xs[perm], ic[perm], sub(perm), want_pointwise=True)
        ref = _reference(Y, Xs, ic, radii, directed)
        _check(a, ref, 'order dir=%d' % directed)
        _check((b[0], b[1][np.argsort(perm)], b[2]), ref, 'permuted dir=%d' % directed)


@pytest.mark.parametrize('directed', [False, True])
def test_large_exponents_stay_finite(da, directed):
    """positions scaled until |eta| reaches about 800 on dyads with y = 1 and with y = 0"""
    rng = np.random.RandomState(21 + directed)
    T, N, D, S = 2, 40, 2, 5
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed, density=0.5)
    Xs *= 800.0 / np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1)).max()
    if directed:
        radii[:] = rng.uniform(0.8, 1.25, radii.shape)
        ic[:] = rng.uniform(0.4, 0.6, ic.shape)
    r64, rld = _reference(Y, Xs, ic, radii, directed)
    l = ic_ref.loglik_rows(Y, Xs, ic, radii, directed, 0, N)
    mask = ic_ref.dyad_mask(N, directed)
    assert l[..., mask].min() < -700 and np.isfinite(r64[2]).all()
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        got = c.ic_accumulate(da.engine.pack_network(Y), Xs, ic, radii, want_pointwise=True)
    _check(got, (r64, rld), 'large dir=%d' % directed)


def test_calls_are_reproducible_and_pointwise_does_not_change_the_sums(da):
    rng = np.random.RandomState(8)
    for directed in (False, True):
        T, N, D, S = 3, 200, 5, 17
        Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
        bits = da.engine.pack_network(Y)
        with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
            a = c.ic_accumulate(bits, Xs, ic, radii, want_pointwise=True)
            b = c.ic_accumulate(bits, Xs, ic, radii, want_pointwise=True)
            n = c.ic_accumulate(bits, Xs, ic, radii)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        assert len(n) == 2 and n[0].tobytes() == a[0].tobytes() and n[1].tobytes() == a[1].tobytes()


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 2, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.ic_accumulate(bits, Xs, ic, None)
        with pytest.raises(ValueError):
            c.ic_accumulate(bits[:1], Xs, ic, radii)
        with pytest.raises(ValueError):
            c.ic_accumulate(bits, Xs[:, :, :, :1], ic, radii)
        Yb = Y.copy()
        Yb[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.ic_accumulate(da.engine.pack_network(Yb), Xs, ic, radii)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.ic_accumulate(bits, Xs, ic, radii * 0)
        assert e.value.code == -4


def _host_result(model, res):
    """the quantities of ``res`` computed by ic_ref from the model's trace"""
    ids = res.sample_ids
    directed = bool(model.is_directed)
    ic = np.asarray(model.intercepts_)[ids].reshape(len(ids), -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_)[ids] if directed else None
    Y = np.asarray(model.Y_fit_)
    ref = _reference(Y, model.Xs_[ids], ic, radii, directed)
    ich = np.ravel(model.intercept_)
    ich = np.array([[ich[0], ich[1] if ich.size > 1 else 0.0]])
    hat = ic_ref.accumulate(Y, np.asarray(model.X_)[None], ich, np.asarray(model.radii_)[None] if directed else None,
                            directed)[1][0]
    return ref, ic_ref.criteria(ref[0][2], ref[0][1], hat, directed)


def _check_result(model, res, label):
    ref, want = _host_result(model, res)
    pw = np.stack([res.pointwise_lppd, res.pointwise_p_waic], axis=-1)
    totals = np.stack([res.lppd_t, res.p_waic_t, res.mean_loglik_t, ref[0][0][:, 3], res.n_dyads_t], axis=1)
    _check((totals, res.sample_loglik, pw), ref, label)
    for name in ('lppd', 'p_waic', 'elpd_waic', 'waic', 'se_elpd', 'd_bar', 'd_hat', 'p_d', 'dic', 'p_v', 'dic_v'):
        np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-9, atol=1e-9, err_msg=label + name)
    assert res.n_dyads == want['n_dyads']
    assert res.p_waic > 0 and res.se_elpd > 0
    for name in ('lppd', 'p_waic', 'elpd_waic', 'waic', 'd_bar', 'd_hat', 'dic'):
        np.testing.assert_allclose(getattr(res, name + '_t').sum(), getattr(res, name), rtol=1e-12)


@pytest.mark.parametrize('directed', [False, True])
def test_end_to_end_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.information_criteria(m, pointwise=True)
    assert res.n_samples == m.Xs_.shape[0] - m.n_burn_ and res.sample_ids[0] == m.n_burn_
    _check_result(m, res, 'monks dir=%d ' % directed)
    few = da.information_criteria(m, n_samples=10)
    assert few.n_samples == 10 and few.pointwise_lppd is None and few.sample_ids[-1] == m.Xs_.shape[0] - 1
    assert 'waic' in res.summary()
    print(res.summary())


def test_end_to_end_on_a_small_hdp_lpcm(da):
    from test_gpu_gof import _splitting
    Y = _splitting(30, 2, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=60, burn=20, tune=20, n_components=4, random_state=1).fit(Y)
    res = da.information_criteria(hdp, pointwise=True)
    _check_result(hdp, res, 'hdp ')
    hdp.release_device_trace()                        # the call then makes a chain of its own
    again = da.information_criteria(hdp, pointwise=True)
    assert again.waic == res.waic and again.dic == res.dic


def test_the_criteria_rank_the_latent_dimension(da):
    """a network drawn with two latent dimensions, fitted with one and with two"""
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=4, N=150, density=0.1, seed=6)['Y']
    fits = {}
    for d in (1, 2):
        m = da.DynamicNetworkLSM(n_features=d, n_iter=600, burn=300, tune=300, random_state=2).fit(Y)
        fits[d] = da.information_criteria(m, n_samples=100, pointwise=True)
    diff, se = da.compare_information_criteria(fits[2], fits[1])
    print('elpd(d=2) - elpd(d=1) = %.1f, se %.1f (%.1f se); dic %.1f against %.1f'
          % (diff, se, diff / se, fits[2].dic, fits[1].dic))
    assert diff > 4 * se, (diff, se)
    assert fits[2].dic < fits[1].dic and fits[2].waic < fits[1].waic


def test_full_size(da):
    """T=10, N=2000, d=2, S=100 on the headline network, the samples jittered around the truth"""
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N, D, S = 10, 2000, 2, 100
    net = synthetic_lsm_network(T=T, N=N, density=0.03, seed=3)
    Y = net['Y']
    rng = np.random.RandomState(5)
    Xs = net['X_true'][None] + 0.05 * rng.randn(S, T, N, D)
    b = float(np.ravel(net['intercept'])[0])
    ic = np.stack([b + 0.02 * rng.randn(S), np.zeros(S)], axis=1)
    with da.Chain(T, N, D, 'undirected') as c:
        totals, sl = c.ic_accumulate(da.engine.pack_network(Y), Xs, ic)
        c.upload_network(Y)
        for s in (0, 49, 99):
            want = _loglik_full(c, Y, Xs, ic, None, s)
            assert abs(sl[s].sum() - want) <= 1e-10 * abs(want), (s, sl[s].sum(), want)
    ref = _reference(Y, Xs, ic, None, False, want_pointwise=False)
    _check((totals, sl), ref, 'full size')
