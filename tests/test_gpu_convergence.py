"""Per-dyad convergence diagnostics on the device (csrc/kernels_conv.hpp, dynetlsm_amd/convergence.py)
against the host restatement tests/convergence_ref.py.  Needs an MI355X: -m gpu.

The tolerance of a real value is not a constant (the rule of test_gpu_ic.py): convergence_ref is evaluated in
float64 and in np.longdouble, eps = max |float64 - longdouble| over the finite values of the output array is the
reference's own rounding error on that input, and the device gets 16 eps + 4 ulp of the value (its Welford
steps multiply by a rounded reciprocal and fuse the multiply-adds: one order of magnitude, no more).  An
infinite value must be met exactly.  The histograms are compared exactly, under the precondition - asserted
first - that no float64 reference value lies within its tolerance of an edge."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import convergence_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

# 16 edges (the most the device holds) around 1, and 9 that spread the ESS of series of 4 to 96 samples
RHAT_EDGES = (0.75, 0.85, 0.95, 1.0, 1.01, 1.02, 1.05, 1.1, 1.15, 1.2, 1.3, 1.5, 1.75, 2.0, 2.5, 3.0)
ESS_EDGES = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 1000.0)

SPLITS = [(1, 2, 1), (1, 7, 2), (3, 16, 4)]          # (chains, seg_len, batch_len)
GRID = [(T, N, D, directed, split)
        for D in (1, 2, 5, 8) for N in (5, 33, 65, 130) + ((17,) if D >= 5 else ())
        for T in (1, 3) for directed in (False, True) for split in SPLITS]


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _case(seed, C, h, T, N, D, directed):
    """C chains of 2 h samples, chain after chain: an AR(1) path around a centre of the chain's own"""
    rng = np.random.RandomState(seed)
    n = 2 * h

    def path(shape, scale, rho=0.7):
        out = np.zeros((C, n) + shape)
        x = scale * rng.randn(C, *shape)
        for s in range(n):
            x = rho * x + np.sqrt(1 - rho * rho) * scale * rng.randn(C, *shape)
            out[:, s] = x
        return out

    Xs = (1.0 / np.sqrt(D)) * (rng.randn(1, 1, T, N, D) + 0.3 * rng.randn(C, 1, T, N, D) + path((T, N, D), 0.4))
    ic = 0.5 + 0.2 * rng.randn(C, 1, 2) + path((2,), 0.3)
    radii = np.exp(0.3 * rng.randn(1, 1, N) + path((N,), 0.1)) if directed else None
    S = C * n
    return (Xs.reshape(S, T, N, D), ic.reshape(S, 2), radii.reshape(S, N) if directed else None)


def _reference(Xs, ic, radii, directed, split, rhat_edges=RHAT_EDGES, ess_edges=ESS_EDGES):
    """the float64 and the longdouble reference, the tolerances of the three real outputs, and the
    precondition of the exact comparison of the histograms"""
    C, h, b = split
    args = (Xs, ic, radii, directed, 2 * C, h, b, rhat_edges, ess_edges)
    r64, rld = cr.accumulate(*args, dtype=np.float64), cr.accumulate(*args, dtype=np.longdouble)
    tols = [cr.tolerance(a, l) for a, l in zip(r64[2:], rld[2:])]
    mask = cr.dyad_mask(Xs.shape[2], directed)
    for k, edges in ((0, rhat_edges), (1, ess_edges)):
        v, tol = r64[4][..., k][:, mask], tols[2][0][..., k][:, mask]
        for e in edges:
            near = np.abs(v - e) <= tol
            assert not near.any(), 'a reference value lies within its tolerance of the edge %r' % (e,)
    return r64, rld, tols


def _check(got, ref, label=''):
    """device outputs (hist_rhat, hist_ess, node_rhat, node_ess, pointwise) against the reference: the real
    arrays within 16 eps + 4 ulp, the histograms exactly"""
    r64, rld, tols = ref
    for name, g, a, (tol, eps) in zip(('node_rhat', 'node_ess', 'pointwise'), got[2:], r64[2:], tols):
        assert not np.isnan(g).any(), (label, name)
        err = cr.error(g, a)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(err == 0, 0.0, err / tol)
        worst = float(ratio.max()) if ratio.size else 0.0
        fin = np.isfinite(err)
        print('%s %-10s eps %.3e  max err %.3e  max err/tol %.3f'
              % (label, name, eps, err[fin].max() if fin.any() else 0.0, worst))
        assert (err <= tol).all(), (label, name, eps, worst)
    for name, g, a in zip(('hist_rhat', 'hist_ess'), got[:2], r64[:2]):
        assert g.dtype == np.uint64
        np.testing.assert_array_equal(g.astype(np.int64), a, err_msg=label + name)


def _check_consistency(got, N, directed):
    """exact relations among the device's own outputs"""
    hr, he, nr, ne, pw = got
    mask = cr.dyad_mask(N, directed)
    n_dyads = int(mask.sum())
    assert (hr.sum(axis=1) == n_dyads).all() and (he.sum(axis=1) == n_dyads).all()
    assert not pw[:, ~mask].any()                    # the diagonal; undirected: the lower triangle as well
    R = np.where(mask, pw[..., 0], 0.0)
    E = np.where(mask, pw[..., 1], np.inf)
    np.testing.assert_array_equal(nr, np.maximum(R.max(axis=2), R.max(axis=1)))
    np.testing.assert_array_equal(ne, np.minimum(E.min(axis=2), E.min(axis=1)))


def _run(da, Xs, ic, radii, directed, split, pointwise=True, rhat_edges=RHAT_EDGES, ess_edges=ESS_EDGES):
    C, h, b = split
    S, T, N, D = Xs.shape
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        return c.convergence_accumulate(Xs, ic, radii, n_segments=2 * C, seg_len=h, batch_len=b,
                                        rhat_edges=rhat_edges, ess_edges=ess_edges, want_pointwise=pointwise)


@pytest.mark.parametrize('T,N,D,directed,split', GRID)
def test_outputs_against_the_reference_on_the_shape_grid(da, T, N, D, directed, split):
    C, h, b = split
    Xs, ic, radii = _case(1000 * N + 16 * D + 4 * T + 2 * directed + C, C, h, T, N, D, directed)
    ref = _reference(Xs, ic, radii, directed, split)
    got = _run(da, Xs, ic, radii, directed, split)
    _check(got, ref, 'T=%d N=%d D=%d dir=%d C=%d h=%d b=%d' % (T, N, D, directed, C, h, b))
    _check_consistency(got, N, directed)


def test_calls_are_reproducible_and_pointwise_does_not_change_the_rest(da):
    for D, directed in ((2, False), (5, True)):
        split = (3, 16, 4)
        Xs, ic, radii = _case(77 + D, 3, 16, 3, 130, D, directed)
        a = _run(da, Xs, ic, radii, directed, split)
        b = _run(da, Xs, ic, radii, directed, split)
        n = _run(da, Xs, ic, radii, directed, split, pointwise=False)
        assert len(a) == 5 and len(n) == 4
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(a, n):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('directed', [False, True])
def test_series_with_defined_values(da, directed):
    T, N, D = 2, 33, 2
    split = (2, 6, 2)
    S = 24
    Xs, ic, radii = _case(5 + directed, 2, 6, T, N, D, directed)
    mask = cr.dyad_mask(N, directed)
    n_dyads = int(mask.sum())
    # identical samples: every dyad has rhat = 1 and ess = S
    rep = np.zeros(S, dtype=int)
    hr, he, nr, ne, pw = _run(da, Xs[rep], ic[rep], radii[rep] if directed else None, directed, split)
    assert (pw[..., 0][:, mask] == 1.0).all() and (pw[..., 1][:, mask] == S).all()
    assert (nr == 1.0).all() and (ne == S).all()
    assert (hr[:, cr.bins(1.0, RHAT_EDGES)] == n_dyads).all() and (he[:, cr.bins(S, ESS_EDGES)] == n_dyads).all()
    # fixed positions, an intercept of each chain's own: rhat = +inf in the last bin, the nodes' maximum +inf
    ic2 = np.repeat(np.array([[0.25, 0.5], [0.75, 0.125]]), 12, axis=0)
    got = _run(da, Xs[rep], ic2, radii[rep] if directed else None, directed, split)
    hr, he, nr, ne, pw = got
    assert (pw[..., 0][:, mask] == np.inf).all() and (nr == np.inf).all()
    assert (hr[:, -1] == n_dyads).all() and (hr[:, :-1] == 0).all()
    assert np.isfinite(pw[..., 1][:, mask]).all() and (pw[..., 1][:, mask] > 0).all()
    _check(got, _reference(Xs[rep], ic2, radii[rep] if directed else None, directed, split), 'apart dir=%d' % directed)
    _check_consistency(got, N, directed)
    # an intercept of period b on fixed positions: every batch mean is the same, ess = +inf
    if not directed:
        ic3 = np.stack([np.tile([0.5, -1.0], 12), np.zeros(S)], axis=1)
        hr, he, nr, ne, pw = _run(da, Xs[rep], ic3, None, directed, split)
        assert (pw[..., 1][:, mask] == np.inf).all() and (ne == np.inf).all() and (he[:, -1] == n_dyads).all()
        assert np.isfinite(pw[..., 0][:, mask]).all()


@pytest.mark.parametrize('directed', [False, True])
def test_large_predictors(da, directed):
    """positions scaled until |eta| reaches about 800"""
    T, N, D = 2, 40, 2
    split = (2, 8, 2)
    Xs, ic, radii = _case(21 + directed, 2, 8, T, N, D, directed)
    Xs *= 800.0 / np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1)).max()
    if directed:
        radii = np.clip(radii, 0.8, 1.25)
    eta = cr.eta_series(Xs, ic, radii, directed)
    assert 700 < np.abs(eta).max() < (2200 if directed else 900)
    got = _run(da, Xs, ic, radii, directed, split)
    _check(got, _reference(Xs, ic, radii, directed, split), 'large dir=%d' % directed)
    _check_consistency(got, N, directed)


def test_bad_arguments_are_rejected(da):
    Xs, ic, radii = _case(0, 1, 4, 2, 9, 2, True)
    with da.Chain(2, 9, 2, 'directed') as c:
        kw = dict(n_segments=2, seg_len=4, batch_len=2, rhat_edges=(1.1, 1.2), ess_edges=(10.0,))
        assert len(c.convergence_accumulate(Xs, ic, radii, **kw)) == 4
        with pytest.raises(ValueError):
            c.convergence_accumulate(Xs, ic, None, **kw)
        with pytest.raises(ValueError):
            c.convergence_accumulate(Xs[:, :, :, :1], ic, radii, **kw)
        for bad in (dict(n_segments=3), dict(seg_len=3), dict(batch_len=3), dict(batch_len=0), dict(n_segments=8, seg_len=1)):
            with pytest.raises(ValueError):
                c.convergence_accumulate(Xs, ic, radii, **dict(kw, **bad))
        with pytest.raises(da.EngineError) as e:
            c.convergence_accumulate(Xs, ic, radii * 0, **kw)
        assert e.value.code == -4
        for edges in (dict(rhat_edges=(1.2, 1.1)), dict(ess_edges=(5.0, 5.0)), dict(ess_edges=(1.0, np.inf))):
            with pytest.raises(da.EngineError) as e:
                c.convergence_accumulate(Xs, ic, radii, **dict(kw, **edges))
            assert e.value.code == -4
        # the checks of the C entry point itself
        from dynetlsm_amd import _lib
        from dynetlsm_amd.engine import _p
        out = c.convergence_accumulate(Xs, ic, radii, **kw)
        hr, he = np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64)
        nr, ne = np.zeros((2, 9)), np.zeros((2, 9))
        e1, e2 = np.array([1.1, 1.2]), np.array([10.0])

        def call(M, h, b):
            return c._L.dlsm_convergence_accumulate(
                c._h, _p(Xs), _p(ic), _p(radii), M, h, b, _p(e1), 2, _p(e2), 1, hr.ctypes.data_as(_lib.c_u64_p),
                he.ctypes.data_as(_lib.c_u64_p), _p(nr), _p(ne), None)
        assert call(2, 4, 2) == 0
        np.testing.assert_array_equal(hr, out[0])
        np.testing.assert_array_equal(ne, out[3])
        for M, h, b in ((1, 8, 2), (3, 2, 1), (0, 4, 2), (8, 1, 1), (2, 4, 3), (2, 4, 0)):
            assert call(M, h, b) == -1, (M, h, b)


def _model_reference(models, res):
    ids = res.sample_ids if isinstance(res.sample_ids, list) else [res.sample_ids]
    h = res.seg_len
    directed = bool(models[0].is_directed)
    Xs = np.concatenate([np.asarray(m.Xs_)[i[:2 * h]] for m, i in zip(models, ids)])
    ic = np.concatenate([np.asarray(m.intercepts_)[i[:2 * h]].reshape(2 * h, -1) for m, i in zip(models, ids)])
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.concatenate([np.asarray(m.radiis_)[i[:2 * h]] for m, i in zip(models, ids)]) if directed else None
    return _reference(Xs, ic, radii, directed, (res.n_chains, h, res.batch_len), res.rhat_edges, res.ess_edges)


def _check_model(da, models, res, label):
    from dynetlsm_amd.multichain import split_rhat
    ref = _model_reference(models, res)
    pw = np.stack([res.pointwise_rhat, res.pointwise_ess], axis=-1)
    got = (res.rhat_hist_t.astype(np.uint64), res.ess_hist_t.astype(np.uint64), res.node_rhat_, res.node_ess_, pw)
    _check(got, ref, label)
    _check_consistency(got, res.n_nodes, res.is_directed)
    ids = res.sample_ids if isinstance(res.sample_ids, list) else [res.sample_ids]
    n = 2 * res.seg_len
    want = split_rhat(np.stack([np.asarray(m.intercepts_)[i[:n], 0] for m, i in zip(models, ids)]))
    assert abs(res.scalars['intercepts[0]'][0] - want) <= 1e-12 * want
    assert 'logps' in res.scalars and res.scalars['logps'][1] > 0
    assert res.max_rhat == res.node_rhat_.max() and res.min_ess == res.node_ess_.min()
    assert res.rhat_hist.sum() == res.n_dyads and 'max rhat' in res.summary()
    print(res.summary())


def test_end_to_end_on_two_chains_of_a_small_lsm(da):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=3, N=30, density=0.15, seed=1)['Y']
    fits = [da.DynamicNetworkLSM(n_iter=80, burn=40, tune=40, random_state=rs).fit(Y) for rs in (0, 1)]
    res = da.convergence_diagnostics(fits, pointwise=True)
    n_kept = fits[0].Xs_.shape[0] - fits[0].n_burn_
    assert res.n_chains == 2 and res.n_segments == 4 and res.seg_len == n_kept // 2
    assert res.batch_len == int(np.floor(np.sqrt(res.seg_len))) and res.n_samples == 4 * res.seg_len
    assert res.sample_ids[0][0] == fits[0].n_burn_
    _check_model(da, fits, res, 'two chains ')
    few = da.convergence_diagnostics(fits, n_samples=10)
    assert few.seg_len == 5 and few.pointwise_rhat is None and few.sample_ids[1][-1] == fits[1].Xs_.shape[0] - 1


@pytest.mark.parametrize('directed', [False, True])
def test_end_to_end_on_a_single_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=3, N=30, density=0.15, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=80, burn=40, tune=40, is_directed=directed, random_state=3).fit(Y)
    res = da.convergence_diagnostics(m, pointwise=True)
    assert res.n_chains == 1 and res.n_segments == 2 and res.is_directed == directed
    _check_model(da, [m], res, 'single dir=%d ' % directed)
