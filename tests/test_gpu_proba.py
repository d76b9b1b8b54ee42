"""Posterior edge probabilities on the device (csrc/kernels_proba.hpp, dynetlsm_amd/probabilities.py) against the
host restatement tests/proba_ref.py.  Needs an MI355X: -m gpu.

Tolerance of mean, sd, lower and upper: the project's rule of ic_ref.tolerance, 16 eps + 4 ulp of the value, with
eps the reference's own error on that input: the larger of max |float64 - longdouble| and the largest change when
every p_s is moved by +-4 ulp with random signs - the device's exp and division allowance; sd cancels, so its eps
is that sensitivity and no fixed number.  Nothing enters it from the code under test.

The fixed-point sums are compared with a derived bound: the number of dyads in the sum times one unit of 2^-32 -
the q of a dyad moves by at most one unit when pbar is off by a few ulp.  The counts (bins of the mean, ties, bins of
the width) must be the reference's exactly; every case first asserts on its own inputs that each reference bin is the
same at pbar (1 +- 1e-12) and at width +- 1e-12 (proba_ref.bins_are_stable).  No dyad is left out."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proba_ref  # noqa: E402
from test_gpu_ic import _case  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
NAMES = ('mean', 'sd', 'lower', 'upper')


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _model(directed):
    return 'directed' if directed else 'undirected'


def _ints(a):
    return np.asarray(a).astype(object)


def _check(got, ref, label, n_bins=20, edges=EDGES):
    """device outputs (calib, brier, node_sums, hist_width, pointwise) against the reference"""
    calib, brier, node, hist, pw = got
    exists, scored = ref['exists'], ref['scored']
    assert proba_ref.bins_are_stable(ref['pw'], scored, n_bins, edges), label + ': pick another seed'
    assert np.isfinite(pw).all(), label
    assert not pw[~exists].any(), label                             # undirected: only i < j is filled
    for c, name in enumerate(NAMES):
        tol, eps = proba_ref.tolerance(ref, c)
        err = np.abs(pw[..., c] - ref['pw'][..., c])
        print('%s %-5s eps %.3e  max err %.3e  max err/tol %.3f' % (label, name, eps, err.max(), (err / tol).max()))
        assert (err <= tol).all(), (label, name, eps, float(err.max()), float((err / tol).max()))
    assert (pw[..., 2] <= pw[..., 3]).all() and (pw[..., 1] >= 0).all(), label
    # the counts are exact, the fixed-point sums within one unit per dyad
    want = _ints(ref['calib'])
    cal = _ints(calib)
    np.testing.assert_array_equal(cal[..., 0], want[..., 0], err_msg=label + ' bin counts')
    np.testing.assert_array_equal(cal[..., 1], want[..., 1], err_msg=label + ' ties')
    assert (np.abs(cal[..., 2] - want[..., 2]) <= want[..., 0]).all(), (label, 'sum of the mean per bin')
    n_t = _ints(scored.sum(axis=(1, 2)))
    assert (np.abs(_ints(brier) - _ints(ref['brier'])) <= n_t).all(), (label, 'brier')
    per_node = np.stack([scored.sum(axis=2), scored.sum(axis=1)], axis=-1).astype(object)
    assert (np.abs(_ints(node) - _ints(ref['node_sums'])) <= per_node).all(), (label, 'node sums')
    np.testing.assert_array_equal(_ints(hist), _ints(ref['hist']), err_msg=label + ' widths')
    assert (_ints(hist).sum(axis=1) == n_t).all() and (cal[..., 0].sum(axis=1) == n_t).all(), label
    # the three sums of fix(pbar) are of the same integers
    assert (cal[..., 2].sum(axis=1) == _ints(node)[..., 0].sum(axis=1)).all(), label
    assert (_ints(node)[..., 0].sum(axis=1) == _ints(node)[..., 1].sum(axis=1)).all(), label


def _mask(rng, T, N):
    """10 % of the entries at random and one whole row"""
    mask = rng.rand(T, N, N) < 0.1
    mask[rng.randint(T), rng.randint(N), :] = True
    return mask


@functools.lru_cache(maxsize=None)
def _inputs(N, T, D, S, directed, masked=False, seed=0):
    rng = np.random.RandomState(1000 * seed + 16 * N + D + 8 * directed + S)
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    return Y, Xs, ic, radii, (_mask(rng, T, N) if masked else None)


def _run(da, inputs, directed, level=0.9, n_bins=20, edges=EDGES, label='', chain=None):
    Y, Xs, ic, radii, mask = inputs
    S, T, N, D = Xs.shape
    bits = da.engine.pack_network(Y)
    pm = da.engine.pack_network(mask) if mask is not None else None
    ref = proba_ref.reference(Y, Xs, ic, radii, directed, level, n_bins, edges, mask)
    if chain is None:
        with da.Chain(T, N, D, _model(directed)) as c:
            got = c.proba_accumulate(bits, Xs, ic, radii, level, mask=pm, n_bins=n_bins, width_edges=edges,
                                     pointwise=True)
    else:
        got = chain.proba_accumulate(bits, Xs, ic, radii, level, mask=pm, n_bins=n_bins, width_edges=edges,
                                     pointwise=True)
    _check(got, ref, label, n_bins, edges)
    return got, ref


@pytest.mark.parametrize('N,T,D,S,directed', [(70, 2, 2, 20, False), (37, 3, 3, 25, True)])
def test_parity_on_two_tiles_and_a_ragged_edge(da, N, T, D, S, directed):
    _run(da, _inputs(N, T, D, S, directed, True), directed, label='N=%d dir=%d' % (N, directed))


@pytest.mark.parametrize('directed', [False, True])
def test_past_one_tile_chunk_and_wavefront(da, directed):
    """N = 200: four column tiles, fifty row blocks of four rows"""
    _run(da, _inputs(200, 2, 2, 8, directed, True), directed, label='N=200 dir=%d' % directed)


@pytest.mark.parametrize('S,K', [(40, 3), (1000, 51), (2000, 101)])
def test_every_form(da, S, K):
    """rows = 4, 2 and 1: K rows <= 144"""
    assert min(int(np.floor(0.05 * (S - 1))) + 2, S) == K
    _run(da, _inputs(40, 1, 2, S, False), False, label='S=%d K=%d' % (S, K))


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('D', range(1, 9))
def test_every_instantiation(da, D, directed):
    _run(da, _inputs(20, 1, D, 12, directed, True), directed, label='D=%d dir=%d' % (D, directed))


@pytest.mark.parametrize('S,level', [(5, 0.2), (2, 0.9), (10, 0.999), (3, 0.5), (21, 0.9), (41, 0.9)])
def test_overlapping_and_degenerate_columns(da, S, level):
    """K = 3 > S / 2; K = S = 2; k0 = 0; the median twice; S = 21 and 41 at level 0.9: the upper position is an
    integer (19.0, 38.0: the weight is 0) while the lower one falls an ulp short of 1 and 2 (a weight of nearly 1)"""
    for directed in (False, True):
        _run(da, _inputs(33, 2, 2, S, directed), directed, level=level, label='S=%d level=%g dir=%d'
             % (S, level, directed))


@pytest.mark.parametrize('directed', [False, True])
def test_ties(da, directed):
    Y, Xs, ic, radii, _ = _inputs(40, 2, 2, 7, directed)
    sub = (lambda idx: radii[idx]) if directed else (lambda idx: None)
    rng = np.random.RandomState(3)
    # every row three times, shuffled
    rep = np.repeat(np.arange(7), 3)[rng.permutation(21)]
    _run(da, (Y, Xs[rep], ic[rep], sub(rep), None), directed, label='thrice dir=%d' % directed)
    # a constant trace: sd = 0 exactly, lower = upper = mean
    rep = np.zeros(9, dtype=int)
    got, ref = _run(da, (Y, Xs[rep], ic[rep], sub(rep), None), directed, label='constant dir=%d' % directed)
    pw = got[4]
    assert not pw[..., 1].any()
    np.testing.assert_array_equal(pw[..., 2], pw[..., 0])
    np.testing.assert_array_equal(pw[..., 3], pw[..., 0])
    assert (got[3][:, 0] == ref['scored'].sum(axis=(1, 2))).all()        # every width is 0


@pytest.mark.parametrize('directed', [False, True])
def test_saturated_probabilities_stay_finite(da, directed):
    """positions scaled until |eta| reaches 800: p is 0 or 1 for most samples"""
    Y, Xs, ic, radii, _ = _inputs(40, 2, 2, 7, directed)
    Xs = Xs * (800.0 / np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1)).max())
    if directed:
        rng = np.random.RandomState(5)
        radii, ic = rng.uniform(0.8, 1.25, radii.shape), rng.uniform(0.4, 0.6, ic.shape)
    from score_ref import linear_predictor
    eta = linear_predictor(Xs, ic, radii, directed)
    assert np.abs(eta).max() > 750 and (proba_ref.expit(eta) == 0).any()
    got, _ = _run(da, (Y, Xs, ic, radii, None), directed, label='saturated dir=%d' % directed)
    assert np.isfinite(got[4]).all() and (got[4] >= 0).all() and (got[4][..., [0, 2, 3]] <= 1).all()


def test_masked_dyads_are_in_pointwise_and_in_no_table(da):
    for directed in (False, True):
        inputs = _inputs(37, 2, 3, 9, directed, True)
        Y, Xs, ic, radii, mask = inputs
        masked, ref = _run(da, inputs, directed, label='masked dir=%d' % directed)
        plain, _ = _run(da, (Y, Xs, ic, radii, None), directed, label='plain dir=%d' % directed)
        assert masked[4].tobytes() == plain[4].tobytes()
        n_masked = ref['exists'].sum(axis=(1, 2)) - ref['scored'].sum(axis=(1, 2))
        assert (n_masked > 0).all()
        np.testing.assert_array_equal(plain[0][..., 0].sum(axis=1) - masked[0][..., 0].sum(axis=1), n_masked)
    # an undirected handle: either orientation of a mask bit excludes the dyad
    Y, Xs, ic, radii, mask = _inputs(37, 2, 3, 9, False, True)
    both = mask | mask.transpose(0, 2, 1)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 37, 3, 'undirected') as c:
        outs = [c.proba_accumulate(bits, Xs, ic, None, 0.9, mask=da.engine.pack_network(m))
                for m in (mask, both, np.triu(both, 1), np.tril(both, -1))]
    for o in outs[1:]:
        for x, y in zip(o[:4], outs[0][:4]):
            assert x.tobytes() == y.tobytes()


def test_calls_are_reproducible_and_pointwise_does_not_change_the_tables(da):
    for directed in (False, True):
        Y, Xs, ic, radii, mask = _inputs(130, 2, 5, 12, directed, True)
        bits, pm = da.engine.pack_network(Y), da.engine.pack_network(mask)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            a = c.proba_accumulate(bits, Xs, ic, radii, 0.8, mask=pm, pointwise=True)
            b = c.proba_accumulate(bits, Xs, ic, radii, 0.8, mask=pm, pointwise=True)
            n = c.proba_accumulate(bits, Xs, ic, radii, 0.8, mask=pm)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            f = c.proba_accumulate(bits, Xs, ic, radii, 0.8, mask=pm)
        assert n[4] is None and f[4] is None
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for other in (n, f):
            for x, y in zip(other[:4], a[:4]):
                assert x.tobytes() == y.tobytes()


def _raw(c, bits, Xs, ic, radii, S, level, n_bins, edges, n_edges=None):
    """the library's own answer, past the checks of Chain.proba_accumulate"""
    from dynetlsm_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    n_edges = edges.size if n_edges is None else n_edges
    keep = [np.ascontiguousarray(Xs), np.ascontiguousarray(ic),
            np.ascontiguousarray(radii) if radii is not None else None,
            np.zeros((c.T, 64, 3), dtype=np.uint64), np.zeros(c.T, dtype=np.uint64),
            np.zeros((c.T, c.N, 2), dtype=np.uint64), np.zeros((c.T, 18), dtype=np.uint64)]
    u64 = _lib.c_u64_p
    return c._L.dlsm_proba_accumulate(
        c._h, bits.ctypes.data_as(_lib.c_u32_p), None, keep[0].ctypes.data_as(dp), keep[1].ctypes.data_as(dp),
        keep[2].ctypes.data_as(dp) if radii is not None else None, S, ctypes.c_double(level), n_bins,
        edges.ctypes.data_as(dp), n_edges, keep[3].ctypes.data_as(u64), keep[4].ctypes.data_as(u64),
        keep[5].ctypes.data_as(u64), keep[6].ctypes.data_as(u64), None)


def test_columns_beyond_the_lds_are_refused_with_the_largest_s_that_fits(da):
    Y, Xs, ic, _, _ = _inputs(3, 1, 1, 1000, False)
    bits = da.engine.pack_network(Y)

    def K(S, level):
        return min(int(np.floor((1.0 - level) / 2.0 * (S - 1))) + 2, S)

    assert K(1000, 0.5) == 251
    with da.Chain(1, 3, 1, 'undirected') as c:
        with pytest.raises(da.EngineError) as e:
            c.proba_accumulate(bits, Xs, ic, None, 0.5)
        assert e.value.code == -5
        m = re.search(r'largest S that fits is (\d+)', str(e.value))
        assert m, str(e.value)
        fit = int(m.group(1))
        # the limit the code declares: 144 KB, two columns of K doubles for each of one row of 64 dyads
        assert 2 * K(fit, 0.5) * 64 * 8 <= 144 << 10 < 2 * K(fit + 1, 0.5) * 64 * 8
        with pytest.raises(da.EngineError) as e:
            c.proba_accumulate(bits, Xs[:fit + 1], ic[:fit + 1], None, 0.5)
        assert e.value.code == -5
        _run(da, (Y, Xs[:fit], ic[:fit], None, None), False, level=0.5, label='S=%d' % fit, chain=c)


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 4, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.proba_accumulate(bits, Xs, ic, None, 0.9)
        with pytest.raises(ValueError):
            c.proba_accumulate(bits[:1], Xs, ic, radii, 0.9)
        with pytest.raises(ValueError):
            c.proba_accumulate(bits, Xs, ic, radii, 0.9, mask=bits[:1])
        with pytest.raises(ValueError, match='two samples'):
            c.proba_accumulate(bits, Xs[:1], ic[:1], radii[:1], 0.9)
        for level in (0.0, 1.0, -0.1, 1.5):
            with pytest.raises(ValueError, match='level'):
                c.proba_accumulate(bits, Xs, ic, radii, level)
        for n_bins in (0, 65):
            with pytest.raises(ValueError, match='n_bins'):
                c.proba_accumulate(bits, Xs, ic, radii, 0.9, n_bins=n_bins)
        with pytest.raises(ValueError, match='16'):
            c.proba_accumulate(bits, Xs, ic, radii, 0.9, width_edges=np.linspace(0.01, 0.9, 17))
        with pytest.raises(ValueError, match='ascending'):
            c.proba_accumulate(bits, Xs, ic, radii, 0.9, width_edges=(0.2, 0.1))
        Yb = Y.copy()
        Yb[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.proba_accumulate(da.engine.pack_network(Yb), Xs, ic, radii, 0.9)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.proba_accumulate(bits, Xs, ic, radii * 0, 0.9)
        assert e.value.code == -4
        pad = bits.copy()
        pad[0, 3, 0] |= np.uint32(1 << 20)                       # N = 9: a bit beyond column 8
        with pytest.raises(da.EngineError) as e:
            c.proba_accumulate(pad, Xs, ic, radii, 0.9)
        assert e.value.code == -4
        # the library's own checks
        ok = (bits, Xs, ic, radii, 4, 0.9, 20, EDGES)
        assert _raw(c, *ok) == 0
        assert _raw(c, bits, Xs, ic, radii, 1, 0.9, 20, EDGES) == -1
        for level in (0.0, 1.0, float('nan')):
            assert _raw(c, bits, Xs, ic, radii, 4, level, 20, EDGES) == -1
        for n_bins in (0, 65):
            assert _raw(c, bits, Xs, ic, radii, 4, 0.9, n_bins, EDGES) == -1
        assert _raw(c, bits, Xs, ic, radii, 4, 0.9, 20, np.linspace(0.01, 0.9, 17)) == -1
        assert _raw(c, bits, Xs, ic, radii, 4, 0.9, 20, (0.2, 0.1)) == -4
        assert _raw(c, bits, Xs, ic, radii, 4, 0.9, 20, (0.1, float('inf'))) == -4
        assert _raw(c, bits, Xs, ic, None, 4, 0.9, 20, EDGES) == -1


def _check_result(model, res, label, held=None, n_bins=20, level=0.9):
    """``res`` against proba_ref on the model's trace rows"""
    ids = res.sample_ids
    directed = bool(model.is_directed)
    ic = np.asarray(model.intercepts_)[ids].reshape(len(ids), -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_)[ids] if directed else None
    Y = np.asarray(model.Y_fit_).copy()
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = 0
    T, N = Y.shape[:2]
    ref = proba_ref.reference(Y, model.Xs_[ids], ic, radii, directed, level, n_bins, EDGES, held)
    full = np.stack([res.mean, res.sd, res.lower, res.upper], axis=-1)
    if not directed:                                               # symmetric with a zero diagonal
        np.testing.assert_array_equal(full, full.transpose(0, 2, 1, 3))
        assert not full[:, idx, idx].any()
        full = np.where(ref['exists'][..., None], full, 0.0)
    cnt = res.counts
    _check((cnt['calib'], cnt['brier'], cnt['node_sums'], res.width_hist_t, full), ref, label, n_bins)
    np.testing.assert_array_equal(res.width_edges, EDGES)
    assert res.n == int(ref['scored'].sum()) and (res.n_t == ref['scored'].sum(axis=(1, 2))).all()
    # the derived scores against brute force on the reference's tables, to the fixed-point bound of 2^-32 per dyad
    pooled = [[sum(ref['calib'][t][b][c] for t in range(T)) for c in range(3)] for b in range(n_bins)]
    for rows, bf, brier, ece, at in [(ref['calib'][t], ref['brier'][t], res.brier_t[t], res.ece_t[t], t)
                                     for t in range(T)] + [(pooled, sum(ref['brier']), res.brier, res.ece, T)]:
        n, rel, want_brier, want_ece = proba_ref.calibration(rows, bf)
        assert abs(brier - want_brier) <= 2.0 ** -32 + 1e-15 and abs(ece - want_ece) <= 2.0 ** -32 + 1e-15, label
        np.testing.assert_array_equal(res.calibration['n'][at], [r[0] for r in rel])
        np.testing.assert_array_equal(res.calibration['ties'][at], [r[1] for r in rel])
        np.testing.assert_allclose(res.calibration['mean_predicted'][at], [r[2] for r in rel], rtol=0,
                                   atol=2.0 ** -32 + 1e-15)
        np.testing.assert_array_equal(res.calibration['observed_frequency'][at], [r[3] for r in rel])
    # expected degrees: the sum over the nodes is the sum of mean predicted x n over the table
    table = float(np.nansum(res.calibration['mean_predicted'][T] * res.calibration['n'][T]))
    Ys = (Y != 0) & ref['scored']
    if directed:
        assert res.expected_degree is None and res.observed_degree is None
        for deg in (res.expected_out_degree, res.expected_in_degree):
            assert abs(deg.sum() - table) <= res.n * 2.0 ** -32 + 1e-13 * table, label
        np.testing.assert_array_equal(res.observed_out_degree, Ys.sum(axis=2))
        np.testing.assert_array_equal(res.observed_in_degree, Ys.sum(axis=1))
        want = np.where(ref['scored'], ref['pw'][..., 0], 0.0)
        np.testing.assert_allclose(res.expected_out_degree, want.sum(axis=2), rtol=0, atol=N * 2.0 ** -32 + 1e-12)
        np.testing.assert_allclose(res.expected_in_degree, want.sum(axis=1), rtol=0, atol=N * 2.0 ** -32 + 1e-12)
    else:
        assert res.expected_out_degree is None and res.observed_in_degree is None
        assert abs(res.expected_degree.sum() - 2 * table) <= 2 * res.n * 2.0 ** -32 + 1e-13 * table, label
        np.testing.assert_array_equal(res.observed_degree, Ys.sum(axis=2) + Ys.sum(axis=1))
        want = np.where(ref['scored'], ref['pw'][..., 0], 0.0)
        np.testing.assert_allclose(res.expected_degree, want.sum(axis=2) + want.sum(axis=1), rtol=0,
                                   atol=N * 2.0 ** -32 + 1e-12)
    text = res.summary()
    assert 'brier' in text and 'ece' in text and 'reliability' in text and repr(res) == text
    return ref


@pytest.mark.parametrize('directed', [False, True])
def test_end_to_end_on_a_short_lsm_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 30
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.edge_probabilities(m)
    assert res.n_samples == m.Xs_.shape[0] - m.n_burn_ and res.sample_ids[0] == m.n_burn_
    assert res.n == T * N * (N - 1) // (1 if directed else 2)
    _check_result(m, res, 'lsm dir=%d ' % directed)
    few = da.edge_probabilities(m, n_samples=30, level=0.5, pointwise=False, n_bins=10)
    assert few.n_samples == 30 and few.mean is None and few.upper is None and few.n_bins == 10
    assert few.sample_ids[-1] == m.Xs_.shape[0] - 1 and few.n == res.n
    assert 0 < res.brier < 0.25 and 0 <= res.ece < 0.5
    print(res.summary())


def test_end_to_end_on_a_sample_missing_fit(da):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 30
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=3)['Y']
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=False)
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, random_state=4, sample_missing=True).fit(Yt)
    res = da.edge_probabilities(m, n_samples=40)
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    assert index.shape[0] > 0 and res.n == T * N * (N - 1) // 2 - index.shape[0]
    _check_result(m, res, 'held out ', held)
    # a held-out dyad has its posterior predictive probability in the pointwise arrays
    t, i, j = index[0]
    assert 0 < res.mean[t, i, j] < 1 and res.lower[t, i, j] <= res.mean[t, i, j] <= res.upper[t, i, j]


def test_end_to_end_on_a_small_hdp_lpcm(da):
    from test_gpu_gof import _splitting
    Y = _splitting(30, 2, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=60, burn=20, tune=20, n_components=4, random_state=1).fit(Y)
    res = da.edge_probabilities(hdp)
    _check_result(hdp, res, 'hdp ')
    hdp.release_device_trace()                        # the call then makes a chain of its own
    again = da.edge_probabilities(hdp)
    assert again.counts == res.counts and again.width_hist_t.tobytes() == res.width_hist_t.tobytes()
    assert again.mean.tobytes() == res.mean.tobytes() and again.upper.tobytes() == res.upper.tobytes()
