"""In-sample scores on the device (csrc/kernels_score.hpp, dynetlsm_amd/scores.py) against the host
restatement tests/score_ref.py.  Needs an MI355X: -m gpu.

The four integers of every time step and of the pooled histogram are compared exactly.  That needs the
device's pbar to fall into the same bin as the host's: the inputs (tests/score_cases.py) are drawn with seeds
for which every scored dyad keeps its key when pbar moves by a relative 1e-12 either way - asserted on the
host before the device is called - and the device's exp, sqrt and division are within a few ulp (the
docstring of tests/test_gpu_ic.py), so the two pbar differ by far less.  The log-loss sums get the rule of
ic_ref.tolerance: 16 eps + 4 ulp, eps = |float64 - longdouble| of score_ref."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ic_ref  # noqa: E402
import score_cases  # noqa: E402
import score_ref  # noqa: E402
from test_gpu_ic import _case  # noqa: E402

pytestmark = pytest.mark.gpu

# roc_auc_score integrates the ROC curve in float64: its own rounding, a few ulp of a number below 1
SKLEARN_ULPS = 8 * np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _device(da, Y, Xs, ic, radii, mask, directed):
    T, N, D = Xs.shape[1:]
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        return c.score_accumulate(da.engine.pack_network(Y), Xs, ic, radii,
                                  mask=None if mask is None else da.engine.pack_network(mask))


def _check(got, ref, label):
    """the integers exactly, the log-loss sums within 16 eps + 4 ulp of score_ref"""
    counts, ll = got
    assert counts.dtype == np.uint64 and counts.shape == (len(ref['counts']), 4)
    print(label, 'device', counts.tolist(), 'host', ref['counts'])
    assert [tuple(int(v) for v in row) for row in counts.tolist()] == [tuple(r) for r in ref['counts']], label
    assert np.isfinite(ll).all(), label
    tol, eps = ic_ref.tolerance(ref['logloss'], ref['logloss_ld'])
    err = np.abs(ll - ref['logloss'])
    print('%s logloss eps %.3e  max err %.3e  max err/tol %.3f' % (label, eps, err.max(), (err / tol).max()))
    assert (err <= tol).all(), (label, eps, float(err.max()))


@pytest.mark.parametrize('index', range(len(score_cases.CASES)), ids=score_cases.IDS)
def test_counts_and_logloss_against_the_reference_on_the_shape_grid(da, index):
    (Y, Xs, ic, radii, mask), ref = score_cases.case(index)
    directed = score_cases.CASES[index][4]
    assert score_cases.stable(ref)                        # the precondition of the exact comparison
    got = _device(da, Y, Xs, ic, radii, mask, directed)
    _check(got, ref, score_cases.IDS[index])
    res = da.scores.scores_from_counts(*got, is_directed=directed)
    assert abs(res.auc - ref['auc_exact']) <= res.auc_bound + SKLEARN_ULPS
    for t, exact in enumerate(ref['auc_exact_t']):
        assert abs(res.auc_t[t] - exact) <= res.auc_bound_t[t] + SKLEARN_ULPS


def test_calls_are_reproducible_bit_for_bit(da):
    index = score_cases.IDS.index('N130-T3-D8-S7-dir-mask')
    (Y, Xs, ic, radii, mask), _ = score_cases.case(index)
    a = _device(da, Y, Xs, ic, radii, mask, True)
    b = _device(da, Y, Xs, ic, radii, mask, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_more_time_steps_than_one_group_of_histograms(da):
    """T = 8 is beyond the time steps whose histograms are held at once: the pooled counts span both groups"""
    rng = np.random.RandomState(5)
    T, N, D, S = 8, 33, 2, 2
    Y, Xs, ic, radii = _case(rng, S, T, N, D, False)
    ref = score_ref.reference(Y, Xs, ic, None, False)
    assert score_cases.stable(ref)
    _check(_device(da, Y, Xs, ic, None, None, False), ref, 'T=8')


@pytest.mark.parametrize('directed', [False, True])
def test_all_positions_equal_is_one_bin(da, directed):
    """whole wavefronts add into one counter: the path that adds the lane count once"""
    rng = np.random.RandomState(11 + directed)
    T, N, D, S = 2, 33, 2, 3
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    Xs[:] = Xs[:, :, :1]
    ref = score_ref.reference(Y, Xs, ic, radii, directed)
    assert score_cases.stable(ref) and len(set(score_ref.key(ref['pbar'][ref['scored']]).tolist())) == 1
    got = _device(da, Y, Xs, ic, radii, None, directed)
    _check(got, ref, 'equal dir=%d' % directed)
    res = da.scores.scores_from_counts(*got)
    assert res.auc == 0.5 and res.auc_bound == 0.5
    assert (res.auc_t == 0.5).all() and (res.auc_bound_t == 0.5).all()


@pytest.mark.parametrize('scale', [200.0, 600.0])
@pytest.mark.parametrize('directed', [False, True])
def test_underflowing_probabilities_share_the_lowest_bin_and_the_logloss_stays_finite(da, directed, scale):
    """positions scaled by 200: every pbar is below 2^-63; by 600: most are 0 in float64 as well, and
    -log pbar of a dyad with y = 1 is still its distance"""
    rng = np.random.RandomState(21 + directed)
    T, N, D, S = 2, 33, 8, 3
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed, density=0.5)
    Xs *= scale
    if directed:                                          # (positive intercepts: eta falls with the distance)
        radii[:] = rng.uniform(0.8, 1.25, radii.shape)
        ic[:] = rng.uniform(0.4, 0.6, ic.shape)
    ref = score_ref.reference(Y, Xs, ic, radii, directed)
    p = ref['pbar'][ref['scored']]
    assert p.max() < 2.0 ** -63 and (p.min() < 1e-200 if scale == 200.0 else np.median(p) == 0.0)
    assert (score_ref.key(p) == score_ref.KEY_LO).all()
    assert np.isfinite(ref['logloss']).all() and ref['logloss'].min() > 1e4
    got = _device(da, Y, Xs, ic, radii, None, directed)
    _check(got, ref, 'underflow dir=%d x%d' % (directed, scale))
    for n_pos, n_neg, u2, ties in got[0].tolist():
        assert u2 == ties == n_pos * n_neg > 0


def test_a_time_step_without_edges_and_a_fully_masked_network(da):
    rng = np.random.RandomState(31)
    T, N, D, S = 2, 33, 2, 3
    Y, Xs, ic, radii = _case(rng, S, T, N, D, False)
    Y[1] = 0
    ref = score_ref.reference(Y, Xs, ic, None, False)
    assert score_cases.stable(ref)
    got = _device(da, Y, Xs, ic, None, None, False)
    _check(got, ref, 'no edges at t=1')
    res = da.scores.scores_from_counts(*got)
    assert res.n_pos_t[1] == 0 and math.isnan(res.auc_t[1]) and math.isnan(res.auc_bound_t[1])
    assert np.isfinite(res.log_loss_t).all()
    assert 0 <= res.auc <= 1 and res.auc_t[0] == score_ref.auc_of_counts(ref['counts'][0])[0]
    # nothing to score: no error, no dyad
    counts, ll = _device(da, Y, Xs, ic, None, np.ones((T, N, N), dtype=bool), False)
    assert not counts.any() and not ll.any()
    none = da.scores.scores_from_counts(counts, ll)
    assert none.n == 0 and math.isnan(none.auc) and math.isnan(none.auc_bound) and math.isnan(none.log_loss)


def _host(model, res, mask=None):
    """score_ref's reference from the trace rows ``res`` used (None: the point estimate)"""
    directed = bool(model.is_directed)
    if res.sample_ids is None:
        Xs, ic = np.asarray(model.X_)[None], np.ravel(model.intercept_)[None]
        radii = np.asarray(model.radii_)[None] if directed else None
    else:
        ids = res.sample_ids
        Xs, ic = model.Xs_[ids], np.asarray(model.intercepts_)[ids].reshape(len(ids), -1)
        radii = np.asarray(model.radiis_)[ids] if directed else None
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    Y = np.asarray(model.Y_fit_).copy()
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = 0
    return score_ref.reference(Y, Xs, ic, radii, directed, mask)


def _check_result(res, ref, label):
    print(label, 'auc %.6f +- %.2e, exact %.6f; log-loss %.6f' % (res.auc, res.auc_bound, ref['auc_exact'],
                                                                   res.log_loss))
    assert abs(res.auc - ref['auc_exact']) <= res.auc_bound + SKLEARN_ULPS, label
    for t, exact in enumerate(ref['auc_exact_t']):
        assert abs(res.auc_t[t] - exact) <= res.auc_bound_t[t] + SKLEARN_ULPS, (label, t)
    assert (res.n_pos, res.n_neg) == tuple(ref['counts'][-1][:2])
    assert res.auc_bound < 1e-3 and 0.5 < res.auc <= 1.0
    np.testing.assert_allclose(res.logloss_sum_t, ref['logloss'], rtol=1e-11)
    np.testing.assert_allclose(res.log_loss, ref['logloss'].sum() / res.n, rtol=1e-11)


@pytest.mark.parametrize('directed', [False, True])
def test_facade_on_a_short_lsm_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 40
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=100, burn=50, tune=50, is_directed=directed, random_state=4).fit(Y)
    n_dyads = T * N * (N - 1) // (1 if directed else 2)
    # the point estimate: the device counterpart of auc_
    point = da.in_sample_scores(m, estimate='map')
    assert point.sample_ids is None and point.n == n_dyads
    assert abs(point.auc - m.auc_) <= point.auc_bound + SKLEARN_ULPS, (point.auc, m.auc_, point.auc_bound)
    _check_result(point, _host(m, point), 'map dir=%d' % directed)
    # the posterior mean over 20 rows of the trace
    res = da.in_sample_scores(m, n_samples=20)
    assert len(res.sample_ids) == 20 and res.sample_ids[0] == m.n_burn_ and res.sample_ids[-1] == m.Xs_.shape[0] - 1
    assert res.n == n_dyads and (res.n_t == n_dyads // T).all()
    _check_result(res, _host(m, res), 'posterior dir=%d' % directed)
    assert 'auc_bound' in res.summary()
    every = da.in_sample_scores(m)
    assert len(every.sample_ids) == m.Xs_.shape[0] - m.n_burn_
    print(res.summary())


@pytest.mark.parametrize('directed', [False, True])
def test_facade_scores_the_observed_dyads_of_a_sample_missing_fit(da, directed):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 40
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=3, directed=directed)['Y']
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=directed)
    m = da.DynamicNetworkLSM(n_iter=100, burn=50, tune=50, is_directed=directed, random_state=4,
                             sample_missing=True).fit(Yt)
    res = da.in_sample_scores(m, n_samples=20)
    n_dyads = T * N * (N - 1) // (1 if directed else 2)
    assert index.shape[0] > 0 and res.n == n_dyads - index.shape[0]
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    _check_result(res, _host(m, res, held), 'held out dir=%d' % directed)


def test_facade_on_a_small_hdp_lpcm(da):
    from test_gpu_gof import _splitting
    Y = _splitting(30, 2, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=60, burn=20, tune=20, n_components=4, random_state=1).fit(Y)
    res = da.in_sample_scores(hdp)
    _check_result(res, _host(hdp, res), 'hdp ')
    point = da.in_sample_scores(hdp, estimate='map')
    assert abs(point.auc - hdp.auc_) <= point.auc_bound + SKLEARN_ULPS


def test_bad_arguments_are_rejected(da):
    from conftest import load_golden
    with pytest.raises(ValueError, match='not fit'):
        da.in_sample_scores(da.DynamicNetworkLSM())
    Y = load_golden('monks.npz')['Y_undirected']
    m = da.DynamicNetworkLSM(n_iter=20, burn=10, tune=10, random_state=4).fit(Y)
    with pytest.raises(ValueError, match='exceeds'):
        da.in_sample_scores(m, n_samples=m.Xs_.shape[0])
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 2, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.score_accumulate(bits, Xs, ic, None)
        with pytest.raises(ValueError):
            c.score_accumulate(bits, Xs, ic, radii, mask=bits[:1])
        Yb = Y.copy()
        Yb[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.score_accumulate(da.engine.pack_network(Yb), Xs, ic, radii)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.score_accumulate(bits, Xs, ic, radii * 0)
        assert e.value.code == -4
