"""PSIS-LOO on the device (csrc/kernels_loo.hpp, csrc/psis_tail.hpp, dynetlsm_amd/loo.py) against the host
restatement tests/loo_ref.py.  Needs an MI355X: -m gpu.

Tolerance: the project's rule of ic_ref.tolerance, 16 eps + 4 ulp of the value, with eps the reference's own error
on that input: the larger of max |float64 - longdouble| and max |ref(l) - ref(l')|, where l' is every l_s moved by
+-4 ulp with random signs - the device's exp / log1p allowance; the fit amplifies input rounding, so the
reference's sensitivity to it enters the tolerance.  Nothing enters it from the code under test.

A dyad may be left out of the value comparison only if the three reference evaluations (float64, longdouble,
perturbed) disagree among themselves on fitted / unfitted, and at most 1 % of a case's dyads.  Sums are then
compared with the left-out dyads' own device values in place of the reference's.  The histogram must equal the
reference's counts except for dyads whose reference k lies within the tolerance of an edge."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ic_ref  # noqa: E402
import loo_ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_gof import CASES  # noqa: E402
from test_gpu_ic import _case  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = [c for c in CASES if c[1] != 2000]
EDGES = np.array([0.5, 0.7, 1.0])


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _edges(S):
    return importlib.import_module('dynetlsm_amd.loo').k_edges(S) if S > 1 else EDGES


def _reference(Y, Xs, ic, radii, directed, edges):
    """loo_ref.accumulate in float64, in longdouble and on the perturbed l"""
    return tuple(loo_ref.accumulate(Y, Xs, ic, radii, directed, edges, dtype, perturb_seed=seed)
                 for dtype, seed in ((np.float64, None), (np.longdouble, None), (np.float64, 77)))


def _tol(a64, ald, apt, where=None):
    """16 eps + 4 ulp of the values a64; eps over the entries ``where`` (all), infinities aside"""
    a64 = np.asarray(a64, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        d = np.maximum(np.abs(a64.astype(np.longdouble) - ald).astype(np.float64), np.abs(a64 - apt))
    if where is not None:
        d = d[where]
    d = d[np.isfinite(d)]
    eps = float(d.max()) if d.size else 0.0
    with np.errstate(invalid='ignore'):
        return 16.0 * eps + 4.0 * np.spacing(np.abs(np.where(np.isfinite(a64), a64, 0.0))), eps


def _check(got, ref, edges, directed, label='', pointwise_at=None):
    """device outputs (totals, hist_k, node_k_max[, pointwise]) against the three reference evaluations.
    ``pointwise_at``: a boolean (T, N, N) choice of the dyads whose pointwise values are compared (all)."""
    r64, rld, rpt = ref
    totals, hist, node = got[:3]
    pw = got[3] if len(got) > 3 else None
    T, N = node.shape
    mask = np.broadcast_to(ic_ref.dyad_mask(N, directed), (T, N, N))
    n_dyads = int(mask[0].sum())
    assert np.isfinite(totals).all(), label
    assert (totals[:, 3] == n_dyads).all() and (hist.sum(axis=1) == n_dyads).all(), label
    f64, fld, fpt = r64[4], rld[4], rpt[4]
    agree = mask & (f64 == fld) & (f64 == fpt)
    left = mask & ~agree
    print('%s left out %d of %d dyads' % (label, left.sum(), mask.sum()))
    assert left.sum() <= 0.01 * mask.sum(), (label, int(left.sum()))
    k64 = r64[3][..., 1]
    tol_k, eps_k = _tol(k64, rld[3][..., 1], rpt[3][..., 1], agree & f64)
    tol_e, eps_e = _tol(r64[3][..., 0], rld[3][..., 0], rpt[3][..., 0], agree)
    if pw is not None:
        at = agree if pointwise_at is None else agree & pointwise_at
        assert np.isfinite(pw[..., 0]).all(), label
        assert not pw[~mask].any(), label                           # undirected: the lower triangle is zero
        err_e = np.abs(pw[..., 0] - r64[3][..., 0])
        fit = at & f64
        for t, i, j in np.argwhere(at & (np.isinf(pw[..., 1]) == f64))[:20]:
            print('%s dyad (%d, %d, %d): device k %r, reference k %r (float64) %r (longdouble) %r (perturbed)'
                  % (label, t, i, j, pw[t, i, j, 1], k64[t, i, j], float(rld[3][t, i, j, 1]), rpt[3][t, i, j, 1]))
        np.testing.assert_array_equal(np.isinf(pw[..., 1])[at], ~f64[at], err_msg=label + ' fitted / unfitted')
        assert (pw[..., 1][at & ~f64] > 0).all(), label
        with np.errstate(invalid='ignore'):
            err_k = np.abs(pw[..., 1] - k64)                        # (inf - inf where both are unfitted)
        print('%s elpd_loo eps %.3e  max err %.3e  max err/tol %.3f | k eps %.3e  max err %.3e  max err/tol %.3f'
              % (label, eps_e, err_e[at].max(), (err_e / tol_e)[at].max(), eps_k,
                 err_k[fit].max() if fit.any() else 0.0, (err_k / tol_k)[fit].max() if fit.any() else 0.0))
        assert (err_e <= tol_e)[at].all(), (label, 'elpd_loo', eps_e, float(err_e[at].max()))
        assert (err_k <= tol_k)[fit].all(), (label, 'k', eps_k, float(err_k[fit].max()))
        # the nodes' largest k is exactly the maximum of the device's own pointwise k
        kf = np.where(mask, pw[..., 1], -np.inf)
        np.testing.assert_array_equal(node, np.maximum(kf.max(axis=2), kf.max(axis=1)), err_msg=label)
    # sums: the left-out dyads enter with the device's own values
    want = [np.array(r[0], dtype=np.longdouble) for r in ref]
    if left.any():
        assert pw is not None, 'dyads were left out: the sums need the pointwise values'
        for w, r in zip(want, ref):
            for t in range(T):
                ge, re_ = pw[t, ..., 0][left[t]], r[3][t, ..., 0][left[t]]
                w[t, 0] += (ge - re_).sum()
                w[t, 1] += (ge * ge - re_ * re_).sum()
                w[t, 4] += np.isinf(pw[t, ..., 1][left[t]]).sum() - (~r[4][t][left[t]]).sum()
    for c, name in ((0, 'sum elpd_loo'), (1, 'sum elpd_loo^2'), (2, 'sum lppd')):
        tol, eps = _tol(want[0][:, c].astype(np.float64), want[1][:, c], want[2][:, c].astype(np.float64))
        err = np.abs(totals[:, c] - want[0][:, c].astype(np.float64))
        print('%s %-15s eps %.3e  max err %.3e  max err/tol %.3f' % (label, name, eps, err.max(), (err / tol).max()))
        assert (err <= tol).all(), (label, name, eps, float(err.max()))
    np.testing.assert_array_equal(totals[:, 4], want[0][:, 4].astype(np.float64), err_msg=label + ' unfitted')
    # histogram: exact, except for dyads within the tolerance of an edge (and the left-out ones)
    nb = len(edges) + 1
    for t in range(T):
        kt, tt = k64[t][mask[t]], tol_k[t][mask[t]]
        lo = np.searchsorted(edges, kt - tt, side='right')
        hi = np.searchsorted(edges, kt + tt, side='right')
        lo[left[t][mask[t]]], hi[left[t][mask[t]]] = 0, nb - 1
        sure = np.bincount(lo[lo == hi], minlength=nb)
        maybe = np.array([((lo != hi) & (lo <= b) & (b <= hi)).sum() for b in range(nb)])
        assert (hist[t] >= sure).all() and (hist[t] <= sure + maybe).all(), (label, t, hist[t], sure, maybe)
        if not maybe.any():
            np.testing.assert_array_equal(hist[t], r64[1][t], err_msg=label)
    # the nodes' largest k against the reference
    if not left.any():
        nk = r64[2]
        tol_n = 16.0 * eps_k + 4.0 * np.spacing(np.abs(np.where(np.isfinite(nk), nk, 0.0)))
        both = np.isfinite(nk)
        np.testing.assert_array_equal(np.isinf(node), ~both, err_msg=label)
        assert (np.abs(node[both] - nk[both]) <= tol_n[both]).all(), (label, 'node_k_max')
    return eps_e, eps_k


def _model(directed):
    return 'directed' if directed else 'undirected'


@pytest.mark.parametrize('T,N,D,directed', GRID)
def test_outputs_against_the_reference_on_the_shape_grid(da, T, N, D, directed):
    """S = 1: nothing to sort; 24: the last unsmoothed S; 25: the first smoothed one, M = 5; 100: M = 20"""
    rng = np.random.RandomState(N * 16 + D + 8 * directed)
    Y, Xs, ic, radii = _case(rng, 100, T, N, D, directed)
    bits = da.engine.pack_network(Y)
    n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
    with da.Chain(T, N, D, _model(directed)) as c:
        for S in (1, 24, 25, 100):
            r = radii[:S] if directed else None
            edges = _edges(S)
            got = c.loo_accumulate(bits, Xs[:S], ic[:S], r, k_edges=edges, want_pointwise=True)
            label = 'N=%d D=%d dir=%d S=%d' % (N, D, directed, S)
            ref = _reference(Y, Xs[:S], ic[:S], r, directed, edges)
            _check(got, ref, edges, directed, label)
            totals, hist, node, pw = got
            assert (totals[:, 3] == n_dyads).all()
            if S < 25:
                assert (totals[:, 4] == n_dyads).all() and np.isinf(node).all()
            if not directed:
                assert not pw[:, np.tril_indices(N)[0], np.tril_indices(N)[1]].any()
            # lppd is the information criteria's
            ic_tot = c.ic_accumulate(bits, Xs[:S], ic[:S], r)[0]
            tol, _ = _tol(*[np.asarray(x[0][:, 2]) for x in ref])
            assert (np.abs(totals[:, 2] - ic_tot[:, 0]) <= tol).all(), (label, totals[:, 2], ic_tot[:, 0], tol)


@pytest.mark.parametrize('directed', [False, True])
def test_the_narrow_form_at_a_long_tail(da, directed):
    """S = 2000: M = 135, one row of 64 dyads per workgroup"""
    rng = np.random.RandomState(40 + directed)
    T, N, D, S = 1, 33, 2, 2000
    assert loo_ref.tail_length(S) == 135
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    edges = _edges(S)
    with da.Chain(T, N, D, _model(directed)) as c:
        got = c.loo_accumulate(da.engine.pack_network(Y), Xs, ic, radii, k_edges=edges, want_pointwise=True)
    _check(got, _reference(Y, Xs, ic, radii, directed, edges), edges, directed, 'narrow dir=%d' % directed)


def test_a_tail_beyond_the_lds_is_refused_with_the_largest_s_that_fits(da):
    rng = np.random.RandomState(9)
    T, N, D = 1, 3, 1
    Y, Xs, ic, _ = _case(rng, 12000, T, N, D, False)
    bits = da.engine.pack_network(Y)
    with da.Chain(T, N, D, 'undirected') as c:
        with pytest.raises(da.EngineError) as e:
            c.loo_accumulate(bits, Xs, ic)
        assert e.value.code == -5
        m = re.search(r'largest S that fits is (\d+)', str(e.value))
        assert m, str(e.value)
        fit = int(m.group(1))
        assert 2000 < fit < 12000
        # the limit the code declares: 144 KB of sorted buffers, one row of 64 dyads, M + 1 doubles each
        assert (loo_ref.tail_length(fit) + 1) * 64 * 8 <= 144 << 10 < (loo_ref.tail_length(fit + 1) + 1) * 64 * 8
        with pytest.raises(da.EngineError) as e:
            c.loo_accumulate(bits, Xs[:fit + 1], ic[:fit + 1])
        assert e.value.code == -5
        got = c.loo_accumulate(bits, Xs[:fit], ic[:fit], k_edges=EDGES, want_pointwise=True)
    _check(got, _reference(Y, Xs[:fit], ic[:fit], None, False, EDGES), EDGES, False, 'S=%d' % fit)


@pytest.mark.parametrize('directed', [False, True])
def test_ties_and_degenerate_tails(da, directed):
    rng = np.random.RandomState(13 + directed)
    T, N, D = 2, 65, 2
    Y, Xs, ic, radii = _case(rng, 50, T, N, D, directed)
    bits = da.engine.pack_network(Y)
    sub = (lambda idx: radii[idx]) if directed else (lambda idx: None)
    n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
    with da.Chain(T, N, D, _model(directed)) as c:
        # S copies of one sample: every dyad unfitted, elpd_loo = l
        rep = np.zeros(30, dtype=int)
        one = c.loo_accumulate(bits, Xs[:1], ic[:1], sub(slice(0, 1)), k_edges=EDGES, want_pointwise=True)
        got = c.loo_accumulate(bits, Xs[rep], ic[rep], sub(rep), k_edges=EDGES, want_pointwise=True)
        ref = _reference(Y, Xs[rep], ic[rep], sub(rep), directed, EDGES)
        # (the perturbed evaluation breaks the ties, so its dyads are fitted: the float64 and longdouble
        # evaluations carry the class here, and the cap of 1 % does not apply to this input)
        assert not ref[0][4].any() and not ref[1][4].any()
        assert (got[0][:, 4] == n_dyads).all() and (got[0][:, 3] == n_dyads).all()
        assert np.isinf(got[3][..., 1][:, ic_ref.dyad_mask(N, directed)]).all()
        assert (got[1][:, -1] == n_dyads).all() and np.isinf(got[2]).all()
        tol = 16.0 * np.max(np.abs(ref[0][3][..., 0].astype(np.longdouble) - ref[1][3][..., 0])).astype(np.float64) \
            + 4.0 * np.spacing(np.abs(ref[0][3][..., 0]))
        assert (np.abs(got[3][..., 0] - ref[0][3][..., 0]) <= tol).all()
        assert (np.abs(got[3][..., 0] - one[3][..., 0]) <= tol).all()
        # 25 distinct samples, each given twice: S = 50, M = 10, the cutoff is one of a tied pair
        twice = np.repeat(np.arange(25), 2)[rng.permutation(50)]
        got = c.loo_accumulate(bits, Xs[twice], ic[twice], sub(twice), k_edges=_edges(50), want_pointwise=True)
        _check(got, _reference(Y, Xs[twice], ic[twice], sub(twice), directed, _edges(50)), _edges(50), directed,
               'twice dir=%d' % directed)
        # a permutation of the samples: every output within the same tolerance
        perm = rng.permutation(50)
        ref = _reference(Y, Xs, ic, radii, directed, _edges(50))
        a = c.loo_accumulate(bits, Xs, ic, radii, k_edges=_edges(50), want_pointwise=True)
        b = c.loo_accumulate(bits, Xs[perm], ic[perm], sub(perm), k_edges=_edges(50), want_pointwise=True)
        _check(a, ref, _edges(50), directed, 'order dir=%d' % directed)
        _check(b, ref, _edges(50), directed, 'permuted dir=%d' % directed)


@pytest.mark.parametrize('directed', [False, True])
def test_large_exponents_stay_finite(da, directed):
    """positions scaled until |eta| reaches about 800: exp(lr_cut) and part of x underflow.

    Saturated dyads have tail values within an ulp of the cutoff, where xstar = exp(lr_(q)) - exp(lr_cut) > 0 -
    fitted or not - hinges on the last bit of the two exponentials.  Dyad (0, 7, 9) of the undirected case is one:
    the arguments differ by 8.15e-17, 0.73 ulp of the results, which both round to the same float64 (correctly
    rounded: 0.28 ulp above and 0.46 ulp below it).  The device's exp and glibc's give that, xstar = 0, unfitted;
    numpy's SIMD exp is one ulp off on one of them and gave a fitted dyad with k = 3.55 (3.64 in longdouble), which
    is why loo_ref takes these two exponentials correctly rounded (loo_ref._exp).  The float64 and the longdouble
    evaluation then disagree on this dyad, and it is one of the few left out under the cap."""
    rng = np.random.RandomState(21 + directed)
    T, N, D, S = 2, 40, 2, 25
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed, density=0.5)
    Xs *= 800.0 / np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1)).max()
    if directed:
        radii[:] = rng.uniform(0.8, 1.25, radii.shape)
        ic[:] = rng.uniform(0.4, 0.6, ic.shape)
    l = ic_ref.loglik_rows(Y, Xs, ic, radii, directed, 0, N)
    assert l[..., ic_ref.dyad_mask(N, directed)].min() < -700
    edges = _edges(S)
    with da.Chain(T, N, D, _model(directed)) as c:
        got = c.loo_accumulate(da.engine.pack_network(Y), Xs, ic, radii, k_edges=edges, want_pointwise=True)
    assert np.isfinite(got[3][..., 0]).all() and np.isfinite(got[0]).all()
    _check(got, _reference(Y, Xs, ic, radii, directed, edges), edges, directed, 'large dir=%d' % directed)


def test_calls_are_reproducible_and_pointwise_does_not_change_the_sums(da):
    rng = np.random.RandomState(8)
    for directed in (False, True):
        T, N, D, S = 3, 200, 5, 40
        Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
        bits = da.engine.pack_network(Y)
        with da.Chain(T, N, D, _model(directed)) as c:
            a = c.loo_accumulate(bits, Xs, ic, radii, k_edges=_edges(S), want_pointwise=True)
            b = c.loo_accumulate(bits, Xs, ic, radii, k_edges=_edges(S), want_pointwise=True)
            n = c.loo_accumulate(bits, Xs, ic, radii, k_edges=_edges(S))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        assert len(n) == 3
        for x, y in zip(n, a):
            assert x.tobytes() == y.tobytes()


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 2, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.loo_accumulate(bits, Xs, ic, None)
        with pytest.raises(ValueError):
            c.loo_accumulate(bits[:1], Xs, ic, radii)
        with pytest.raises(ValueError):
            c.loo_accumulate(bits, Xs[:, :, :, :1], ic, radii)
        with pytest.raises(ValueError):
            c.loo_accumulate(bits, Xs, ic, radii, k_edges=np.linspace(0, 1, 17))
        Yb = Y.copy()
        Yb[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.loo_accumulate(da.engine.pack_network(Yb), Xs, ic, radii)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.loo_accumulate(bits, Xs, ic, radii * 0)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.loo_accumulate(bits, Xs, ic, radii, k_edges=(0.7, 0.5))
        assert e.value.code == -4
        # the library itself holds at most 16 edges
        from dynetlsm_amd import _lib
        import ctypes
        edges = np.linspace(0.0, 1.0, 17)
        tot, hist, node = np.zeros((2, 5)), np.zeros((2, 18), dtype=np.uint64), np.zeros((2, 9))
        dp = ctypes.POINTER(ctypes.c_double)
        rc = c._L.dlsm_loo_accumulate(
            c._h, bits.ctypes.data_as(_lib.c_u32_p), np.ascontiguousarray(Xs).ctypes.data_as(dp),
            np.ascontiguousarray(ic).ctypes.data_as(dp), np.ascontiguousarray(radii).ctypes.data_as(dp), 2,
            edges.ctypes.data_as(dp), 17, tot.ctypes.data_as(dp), hist.ctypes.data_as(_lib.c_u64_p),
            node.ctypes.data_as(dp), None)
        assert rc == -1


def _check_result(model, res, label):
    """``res`` against loo_ref on the model's trace"""
    ids = res.sample_ids
    directed = bool(model.is_directed)
    ic = np.asarray(model.intercepts_)[ids].reshape(len(ids), -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_)[ids] if directed else None
    Y = np.asarray(model.Y_fit_)
    edges = _edges(len(ids))
    np.testing.assert_array_equal(res.k_edges, edges)
    ref = _reference(Y, model.Xs_[ids], ic, radii, directed, edges)
    pw = np.stack([res.pointwise_elpd_loo, res.pointwise_k], axis=-1)
    totals = np.stack([res.elpd_loo_t, ref[0][0][:, 1], res.lppd_t, res.n_dyads_t, res.n_unfitted_t], axis=1)
    _check((totals, res.k_hist_t, res.node_k_, pw), ref, edges, directed, label)
    want = loo_ref.result(ref[0][3], ref[0][0][:, 2], directed)
    for name in ('elpd_loo', 'p_loo', 'looic', 'se_elpd_loo', 'lppd'):
        np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-9, atol=1e-9, err_msg=label + name)
    assert res.n_dyads == want['n_dyads'] and res.n_unfitted == want['n_unfitted']
    assert res.max_k == res.pointwise_k[:, res.dyad_mask()].max()
    assert res.n_bad == int((res.pointwise_k[:, res.dyad_mask()] > res.k_threshold).sum())
    assert res.p_loo > 0 and res.se_elpd_loo > 0
    for name in ('elpd_loo', 'p_loo', 'looic', 'lppd'):
        np.testing.assert_allclose(getattr(res, name + '_t').sum(), getattr(res, name), rtol=1e-12)
    assert 'n_bad' in res.summary()


@pytest.mark.parametrize('directed', [False, True])
def test_end_to_end_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.loo(m, pointwise=True)
    assert res.n_samples == m.Xs_.shape[0] - m.n_burn_ and res.sample_ids[0] == m.n_burn_
    _check_result(m, res, 'monks dir=%d ' % directed)
    same = da.information_criteria(m)
    np.testing.assert_array_equal(same.sample_ids, res.sample_ids)
    np.testing.assert_allclose(res.lppd, same.lppd, rtol=1e-12)
    few = da.loo(m, n_samples=30)
    assert few.n_samples == 30 and few.pointwise_k is None and few.sample_ids[-1] == m.Xs_.shape[0] - 1
    print(res.summary())


def test_end_to_end_on_a_small_hdp_lpcm(da):
    from test_gpu_gof import _splitting
    Y = _splitting(30, 2, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=60, burn=20, tune=20, n_components=4, random_state=1).fit(Y)
    res = da.loo(hdp, pointwise=True)
    _check_result(hdp, res, 'hdp ')
    hdp.release_device_trace()                        # the call then makes a chain of its own
    again = da.loo(hdp, pointwise=True)
    assert again.elpd_loo == res.elpd_loo and again.max_k == res.max_k


def test_loo_ranks_the_latent_dimension_as_the_information_criteria_do(da):
    """a network drawn with two latent dimensions, fitted with one and with two"""
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=4, N=150, density=0.1, seed=6)['Y']
    fits, waic = {}, {}
    for d in (1, 2):
        m = da.DynamicNetworkLSM(n_features=d, n_iter=600, burn=300, tune=300, random_state=2).fit(Y)
        fits[d] = da.loo(m, n_samples=100, pointwise=True)
        waic[d] = da.information_criteria(m, n_samples=100, pointwise=True)
        print('d=%d  elpd_loo %.2f  elpd_waic %.2f  |elpd_loo - elpd_waic| %.3f  n_bad %d  max_k %.3f'
              % (d, fits[d].elpd_loo, waic[d].elpd_waic, abs(fits[d].elpd_loo - waic[d].elpd_waic), fits[d].n_bad,
                 fits[d].max_k))
        assert 'n_bad' in fits[d].summary()
    diff, se = da.compare_loo(fits[2], fits[1])
    diff_w, _ = da.compare_information_criteria(waic[2], waic[1])
    print('elpd_loo(d=2) - elpd_loo(d=1) = %.1f, se %.1f; by WAIC %.1f' % (diff, se, diff_w))
    assert np.sign(diff) == np.sign(diff_w) and se > 0
    np.testing.assert_allclose(diff, fits[2].elpd_loo - fits[1].elpd_loo, rtol=1e-9)


def test_full_size(da):
    """T=1, N=2000, d=2, S=25 on the headline network, the samples jittered around the truth"""
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N, D, S = 1, 2000, 2, 25
    net = synthetic_lsm_network(T=T, N=N, density=0.03, seed=3)
    Y = net['Y']
    rng = np.random.RandomState(5)
    Xs = net['X_true'][None] + 0.05 * rng.randn(S, T, N, D)
    b = float(np.ravel(net['intercept'])[0])
    ic = np.stack([b + 0.02 * rng.randn(S), np.zeros(S)], axis=1)
    edges = _edges(S)
    bits = da.engine.pack_network(Y)
    with da.Chain(T, N, D, 'undirected') as c:
        got = c.loo_accumulate(bits, Xs, ic, k_edges=edges, want_pointwise=True)
        sums = c.loo_accumulate(bits, Xs, ic, k_edges=edges)
        ic_tot = c.ic_accumulate(bits, Xs, ic)[0]
    for x, y in zip(sums, got):
        assert x.tobytes() == y.tobytes()
    ref = _reference(Y, Xs, ic, None, False, edges)
    # pointwise on 20 000 randomly chosen dyads; totals, histogram and the nodes over all of them
    iu = np.triu_indices(N, 1)
    pick = rng.choice(iu[0].size, 20000, replace=False)
    at = np.zeros((T, N, N), dtype=bool)
    at[0, iu[0][pick], iu[1][pick]] = True
    _check(got, ref, edges, False, 'full size', pointwise_at=at)
    lp = [np.asarray(r[0][:, 2]) for r in ref]
    tol, _ = _tol(lp[0], lp[1], lp[2])
    assert (np.abs(got[0][:, 2] - ic_tot[:, 0]) <= tol).all(), (got[0][:, 2], ic_tot[:, 0], tol)
