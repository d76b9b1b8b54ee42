"""Tie dynamics on the device (csrc/kernels_dynamics.hpp, dynetlsm_amd/dynamics.py) against the host restatement
tests/dynamics_ref.py.  Needs an MI355X: -m gpu.

Tolerance of delta_mean and delta_sd: the project's rule of ic_ref.tolerance, 16 eps + 4 ulp of the value, with eps
the reference's own error on that input: the larger of max |float64 - longdouble| and the largest change when every
p_s is moved by +-4 ulp with random signs - the device's exp and division allowance.  Nothing enters it from the code
under test.

prob_up and prob_down, the class counts, the histogram of up and the nodes' counts must be the reference's exactly;
every case first asserts on its own inputs that no eta_{t+1} - eta_t is close enough to 0 for a rounding to turn its
sign (dynamics_ref.signs_are_stable).  The fixed-point sums are compared with a derived bound: the number of dyads
in the sum times one unit of 2^-32 - the fix of a dyad moves by at most one unit when the mean is off by a few ulp.
No dyad is left out."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dynamics_ref  # noqa: E402
import proba_ref  # noqa: E402
from test_gpu_ic import _case  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ('delta_mean', 'delta_sd', 'prob_up', 'prob_down')


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _model(directed):
    return 'directed' if directed else 'undirected'


def _ints(a):
    return np.asarray(a).astype(object)


def _min_count(level, S):
    return int(math.ceil(level * S - 1e-12))


def _check(got, ref, label):
    """device outputs (transitions, hist_up, node_changes, node_turnover, pointwise) against the reference"""
    trans, hist, changes, turn, pw = got
    exists, scored = ref['exists'], ref['scored']
    assert dynamics_ref.signs_are_stable(ref['eta'], ref['eta_ld']), label + ': pick another seed'
    assert np.isfinite(pw).all(), label
    assert not pw[~exists].any(), label                             # undirected: only i < j is filled
    for c in (0, 1):
        tol, eps = dynamics_ref.tolerance(ref, c)
        err = np.abs(pw[..., c] - ref['pw'][..., c])
        print('%s %-10s eps %.3e  max err %.3e  max err/tol %.3f' % (label, NAMES[c], eps, err.max(),
                                                                      (err / tol).max()))
        assert (err <= tol).all(), (label, NAMES[c], eps, float(err.max()), float((err / tol).max()))
    assert (pw[..., 1] >= 0).all() and (np.abs(pw[..., 0]) <= 1).all(), label
    np.testing.assert_array_equal(pw[..., 2], ref['pw'][..., 2], err_msg=label + ' prob_up')
    np.testing.assert_array_equal(pw[..., 3], ref['pw'][..., 3], err_msg=label + ' prob_down')
    # the counts are exact, the fixed-point sums within one unit per dyad
    want, tr = _ints(ref['transitions']), _ints(trans)
    np.testing.assert_array_equal(tr[..., 0], want[..., 0], err_msg=label + ' class counts')
    assert (np.abs(tr - want) <= want[..., :1]).all(), (label, 'sums per class')
    np.testing.assert_array_equal(_ints(hist), _ints(ref['hist_up']), err_msg=label + ' histogram of up')
    np.testing.assert_array_equal(_ints(changes), _ints(ref['node_changes']), err_msg=label + ' node changes')
    per_node = np.stack([scored.sum(axis=2), scored.sum(axis=1)], axis=-1).astype(object)
    assert (np.abs(_ints(turn) - _ints(ref['node_turnover'])) <= per_node).all(), (label, 'node turnover')
    n_u = _ints(scored.sum(axis=(1, 2)))
    assert (tr[..., 0].sum(axis=1) == n_u).all() and (_ints(hist).sum(axis=1) == n_u).all(), label
    # a dyad enters one row slot and one column slot with the same integer
    assert (_ints(turn)[..., 0].sum(axis=1) == _ints(turn)[..., 1].sum(axis=1)).all(), label
    ch = _ints(changes)
    assert (ch[..., 0].sum(axis=1) == ch[..., 1].sum(axis=1)).all(), label
    assert (ch[..., 2].sum(axis=1) == ch[..., 3].sum(axis=1)).all(), label


def _mask(rng, T, N):
    """10 % of the entries at random and one whole row"""
    mask = rng.rand(T, N, N) < 0.1
    mask[rng.randint(T), rng.randint(N), :] = True
    return mask


@functools.lru_cache(maxsize=None)
def _inputs(N, T, D, S, directed, masked=False, seed=0):
    rng = np.random.RandomState(1000 * seed + 16 * N + D + 8 * directed + S + 64 * T)
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    return Y, Xs, ic, radii, (_mask(rng, T, N) if masked else None)


def _run(da, inputs, directed, min_count=None, n_bins=20, label='', chain=None):
    Y, Xs, ic, radii, mask = inputs
    S, T, N, D = Xs.shape
    min_count = _min_count(0.9, S) if min_count is None else min_count
    bits = da.engine.pack_network(Y)
    pm = da.engine.pack_network(mask) if mask is not None else None
    ref = dynamics_ref.reference(Y, Xs, ic, radii, directed, min_count, n_bins, mask)
    if chain is None:
        with da.Chain(T, N, D, _model(directed)) as c:
            got = c.dynamics_accumulate(bits, Xs, ic, radii, min_count, mask=pm, n_bins=n_bins, pointwise=True)
    else:
        got = chain.dynamics_accumulate(bits, Xs, ic, radii, min_count, mask=pm, n_bins=n_bins, pointwise=True)
    assert got[4].shape == (T - 1, N, N, 4) and got[0].shape == (T - 1, 4, 4) and got[1].shape == (T - 1, n_bins)
    _check(got, ref, label)
    return got, ref


@pytest.mark.parametrize('N,T,D,S,directed', [(70, 3, 2, 20, False), (37, 4, 3, 25, True)])
def test_parity_on_two_tiles_a_ragged_edge_and_several_steps(da, N, T, D, S, directed):
    got, ref = _run(da, _inputs(N, T, D, S, directed, True), directed, label='N=%d dir=%d' % (N, directed))
    # the steps differ: a step that read the wrong pair of time steps would not pass
    assert not np.array_equal(ref['up'][0], ref['up'][1])


@pytest.mark.parametrize('directed', [False, True])
def test_past_one_tile_chunk_and_wavefront_with_a_single_step(da, directed):
    """N = 200: four column tiles, seven row blocks of 32 rows; T = 2: one step"""
    _run(da, _inputs(200, 2, 2, 8, directed, True), directed, label='N=200 dir=%d' % directed)


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('D', range(1, 9))
def test_every_instantiation(da, D, directed):
    _run(da, _inputs(20, 2, D, 12, directed, True), directed, n_bins=7, label='D=%d dir=%d' % (D, directed))


@pytest.mark.parametrize('directed', [False, True])
def test_identical_consecutive_time_steps_are_exact_ties(da, directed):
    Y, Xs, ic, radii, _ = _inputs(40, 3, 2, 7, directed)
    Xs = Xs.copy()
    Xs[:, 1] = Xs[:, 0]
    got, ref = _run(da, (Y, Xs, ic, radii, None), directed, label='tied dir=%d' % directed)
    trans, hist, changes, turn, pw = got
    assert not pw[0].any()                                           # delta_mean, delta_sd, up and down: exactly 0
    assert hist[0, 0] == ref['scored'][0].sum() and not hist[0, 1:].any()
    assert not changes[0].any() and not turn[0].any()
    assert pw[1, ..., 0].any() and hist[1, 1:].any()                 # step 1 moves (and matched the reference)


@pytest.mark.parametrize('directed', [False, True])
def test_ties_between_the_samples(da, directed):
    Y, Xs, ic, radii, _ = _inputs(40, 3, 2, 7, directed)
    sub = (lambda idx: radii[idx]) if directed else (lambda idx: None)
    rng = np.random.RandomState(3)
    # every row three times, shuffled
    rep = np.repeat(np.arange(7), 3)[rng.permutation(21)]
    _run(da, (Y, Xs[rep], ic[rep], sub(rep), None), directed, label='thrice dir=%d' % directed)
    # a constant trace: sd = 0 exactly, and the direction is certain wherever the step is not a tie
    rep = np.zeros(9, dtype=int)
    got, ref = _run(da, (Y, Xs[rep], ic[rep], sub(rep), None), directed, label='constant dir=%d' % directed)
    pw = got[4]
    assert not pw[..., 1].any()
    ex = ref['exists']
    assert np.isin(pw[..., 2][ex], (0.0, 1.0)).all() and (pw[..., 2][ex] + pw[..., 3][ex] == 1.0).all()
    assert (got[1][:, 1:-1] == 0).all()                              # the histogram: first and last bin only


@pytest.mark.parametrize('directed', [False, True])
def test_saturated_probabilities_stay_finite(da, directed):
    """positions scaled until |eta| reaches 800: p is 0 or 1 for most samples"""
    Y, Xs, ic, radii, _ = _inputs(40, 3, 2, 7, directed)
    Xs = Xs * (800.0 / np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1)).max())
    if directed:
        rng = np.random.RandomState(5)
        radii, ic = rng.uniform(0.8, 1.25, radii.shape), rng.uniform(0.4, 0.6, ic.shape)
    from score_ref import linear_predictor
    eta = linear_predictor(Xs, ic, radii, directed)
    assert np.abs(eta).max() > 750 and (proba_ref.expit(eta) == 0).any()
    got, _ = _run(da, (Y, Xs, ic, radii, None), directed, label='saturated dir=%d' % directed)
    pw = got[4]
    assert np.isfinite(pw).all() and (np.abs(pw[..., 0]) <= 1).all() and (pw[..., 2] + pw[..., 3] <= 1).all()


def test_a_mask_bit_at_one_time_step_removes_the_dyad_from_both_of_its_steps(da):
    for directed in (False, True):
        Y, Xs, ic, radii, _ = _inputs(37, 4, 3, 9, directed)
        t, i, j = 2, 5, 30
        mask = np.zeros(Y.shape, dtype=bool)
        mask[t, i, j] = True
        masked, ref = _run(da, (Y, Xs, ic, radii, mask), directed, label='one bit dir=%d' % directed)
        plain, _ = _run(da, (Y, Xs, ic, radii, None), directed, label='plain dir=%d' % directed)
        assert masked[4].tobytes() == plain[4].tobytes()
        lost = plain[0][..., 0].sum(axis=1).astype(np.int64) - masked[0][..., 0].sum(axis=1).astype(np.int64)
        np.testing.assert_array_equal(lost, [0, 1, 1])               # steps t - 1 and t
        np.testing.assert_array_equal(plain[1].sum(axis=1).astype(np.int64) - masked[1].sum(axis=1).astype(np.int64),
                                      [0, 1, 1])
        assert masked[0][0].tobytes() == plain[0][0].tobytes() and masked[2][0].tobytes() == plain[2][0].tobytes()
        assert masked[3][0].tobytes() == plain[3][0].tobytes()
        other = np.ones(37, dtype=bool)                              # only the two nodes of the dyad change
        other[[i, j]] = False
        for tab in (2, 3):
            assert masked[tab][1:][:, other].tobytes() == plain[tab][1:][:, other].tobytes()
        assert (masked[3][1:, i, 0] < plain[3][1:, i, 0]).all() and (masked[3][1:, j, 1] < plain[3][1:, j, 1]).all()


def test_masked_dyads_are_in_pointwise_and_in_no_table(da):
    for directed in (False, True):
        inputs = _inputs(37, 3, 3, 9, directed, True)
        Y, Xs, ic, radii, mask = inputs
        masked, ref = _run(da, inputs, directed, label='masked dir=%d' % directed)
        plain, _ = _run(da, (Y, Xs, ic, radii, None), directed, label='plain dir=%d' % directed)
        assert masked[4].tobytes() == plain[4].tobytes()
        n_masked = ref['exists'].sum(axis=(1, 2)) - ref['scored'].sum(axis=(1, 2))
        assert (n_masked > 0).all()
        np.testing.assert_array_equal(plain[0][..., 0].sum(axis=1) - masked[0][..., 0].sum(axis=1), n_masked)
    # an undirected handle: either orientation of a mask bit excludes the dyad
    Y, Xs, ic, radii, mask = _inputs(37, 3, 3, 9, False, True)
    both = mask | mask.transpose(0, 2, 1)
    bits = da.engine.pack_network(Y)
    with da.Chain(3, 37, 3, 'undirected') as c:
        outs = [c.dynamics_accumulate(bits, Xs, ic, None, 8, mask=da.engine.pack_network(m))
                for m in (mask, both, np.triu(both, 1), np.tril(both, -1))]
    for o in outs[1:]:
        for x, y in zip(o[:4], outs[0][:4]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('directed', [False, True])
def test_min_count_at_both_ends_and_at_the_default(da, directed):
    inputs = _inputs(37, 3, 3, 20, directed, True)
    seen = []
    with da.Chain(3, 37, 3, _model(directed)) as c:
        for min_count in (1, 20, _min_count(0.9, 20)):
            got, ref = _run(da, inputs, directed, min_count=min_count, label='min_count=%d' % min_count, chain=c)
            seen.append(int(got[2].sum()))
            if min_count == 1:                                       # a dyad can then count as risen and as fallen
                assert ((ref['up'] >= 1) & (ref['down'] >= 1) & ref['scored']).any()
    assert _min_count(0.9, 20) == 18 and seen[0] > seen[2] >= seen[1]


def test_calls_are_reproducible_and_pointwise_does_not_change_the_tables(da):
    for directed in (False, True):
        Y, Xs, ic, radii, mask = _inputs(130, 3, 5, 12, directed, True)
        bits, pm = da.engine.pack_network(Y), da.engine.pack_network(mask)
        with da.Chain(3, 130, 5, _model(directed)) as c:
            a = c.dynamics_accumulate(bits, Xs, ic, radii, 10, mask=pm, pointwise=True)
            b = c.dynamics_accumulate(bits, Xs, ic, radii, 10, mask=pm, pointwise=True)
            n = c.dynamics_accumulate(bits, Xs, ic, radii, 10, mask=pm)
        with da.Chain(3, 130, 5, _model(directed)) as c:
            f = c.dynamics_accumulate(bits, Xs, ic, radii, 10, mask=pm)
        assert n[4] is None and f[4] is None and a[0].any() and a[3].any()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for other in (n, f):
            for x, y in zip(other[:4], a[:4]):
                assert x.tobytes() == y.tobytes()


def _raw(c, bits, Xs, ic, radii, S, min_count, n_bins):
    """the library's own answer, past the checks of Chain.dynamics_accumulate"""
    from dynetlsm_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    U = max(c.T - 1, 1)
    keep = [np.ascontiguousarray(Xs), np.ascontiguousarray(ic),
            np.ascontiguousarray(radii) if radii is not None else None,
            np.zeros((U, 4, 4), dtype=np.uint64), np.zeros((U, 64), dtype=np.uint64),
            np.zeros((U, c.N, 4), dtype=np.uint64), np.zeros((U, c.N, 2), dtype=np.uint64)]
    u64 = _lib.c_u64_p
    return c._L.dlsm_dynamics_accumulate(
        c._h, bits.ctypes.data_as(_lib.c_u32_p), None, keep[0].ctypes.data_as(dp), keep[1].ctypes.data_as(dp),
        keep[2].ctypes.data_as(dp) if radii is not None else None, S, min_count, n_bins,
        keep[3].ctypes.data_as(u64), keep[4].ctypes.data_as(u64), keep[5].ctypes.data_as(u64),
        keep[6].ctypes.data_as(u64), None)


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 4, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.dynamics_accumulate(bits, Xs, ic, None, 4)
        with pytest.raises(ValueError):
            c.dynamics_accumulate(bits[:1], Xs, ic, radii, 4)
        with pytest.raises(ValueError):
            c.dynamics_accumulate(bits, Xs, ic, radii, 4, mask=bits[:1])
        with pytest.raises(ValueError, match='two samples'):
            c.dynamics_accumulate(bits, Xs[:1], ic[:1], radii[:1], 1)
        for min_count in (0, 5, -1, 2.5):
            with pytest.raises(ValueError, match='min_count'):
                c.dynamics_accumulate(bits, Xs, ic, radii, min_count)
        for n_bins in (0, 65):
            with pytest.raises(ValueError, match='n_bins'):
                c.dynamics_accumulate(bits, Xs, ic, radii, 4, n_bins=n_bins)
        Yb = Y.copy()
        Yb[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.dynamics_accumulate(da.engine.pack_network(Yb), Xs, ic, radii, 4)
        assert e.value.code == -4
        with pytest.raises(da.EngineError) as e:
            c.dynamics_accumulate(bits, Xs, ic, radii * 0, 4)
        assert e.value.code == -4
        pad = bits.copy()
        pad[0, 3, 0] |= np.uint32(1 << 20)                       # N = 9: a bit beyond column 8
        with pytest.raises(da.EngineError) as e:
            c.dynamics_accumulate(pad, Xs, ic, radii, 4)
        assert e.value.code == -4
        # the library's own checks
        assert _raw(c, bits, Xs, ic, radii, 4, 4, 20) == 0
        assert _raw(c, bits, Xs, ic, radii, 1, 1, 20) == -1
        for min_count in (0, 5, -3):
            assert _raw(c, bits, Xs, ic, radii, 4, min_count, 20) == -1
        for n_bins in (0, 65):
            assert _raw(c, bits, Xs, ic, radii, 4, 4, n_bins) == -1
        assert _raw(c, bits, Xs, ic, None, 4, 4, 20) == -1
        assert _raw(c, pad, Xs, ic, radii, 4, 4, 20) == -4
        assert _raw(c, bits, Xs, ic, radii * 0, 4, 4, 20) == -4
    # a handle with one time step has no step
    with da.Chain(1, 9, 2, 'directed') as c:
        with pytest.raises(ValueError, match='two time steps'):
            c.dynamics_accumulate(bits[:1], Xs[:, :1], ic, radii, 4)
        assert _raw(c, np.ascontiguousarray(bits[:1]), Xs[:, :1], ic, radii, 4, 4, 20) == -1


def _check_result(model, res, label, held=None, n_bins=20, level=0.9):
    """``res`` against dynamics_ref on the model's trace rows"""
    ids = res.sample_ids
    S = len(ids)
    directed = bool(model.is_directed)
    ic = np.asarray(model.intercepts_)[ids].reshape(S, -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_)[ids] if directed else None
    Y = np.asarray(model.Y_fit_).copy()
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = 0
    T, N = Y.shape[:2]
    assert res.n_samples == S and res.level == level and res.min_count == _min_count(level, S)
    ref = dynamics_ref.reference(Y, model.Xs_[ids], ic, radii, directed, res.min_count, n_bins, held)
    full = np.stack([res.delta_mean, res.delta_sd, res.prob_up, res.prob_down], axis=-1)
    assert full.shape == (T - 1, N, N, 4)
    if not directed:                                               # symmetric with a zero diagonal
        np.testing.assert_array_equal(full, full.transpose(0, 2, 1, 3))
        assert not full[:, idx, idx].any()
        full = np.where(ref['exists'][..., None], full, 0.0)
    cnt = res.counts
    _check((cnt['transitions'], cnt['hist_up'], cnt['node_changes'], cnt['node_turnover'], full), ref, label)
    scored = ref['scored']
    n_u = scored.sum(axis=(1, 2))
    assert res.n == int(scored.sum()) and (res.n_t == n_u).all()
    # the ties at t over the scored steps either persisted or dissolved
    ties_t = ((Y[:-1] != 0) & scored).sum(axis=(1, 2))
    np.testing.assert_array_equal(res.observed_persisted_t + res.observed_dissolved_t, ties_t)
    np.testing.assert_array_equal(res.observed_formed_t, ((Y[:-1] == 0) & (Y[1:] != 0) & scored).sum(axis=(1, 2)))
    assert res.observed_persisted + res.observed_dissolved == int(ties_t.sum())
    # the derived numbers against the reference's float64 values, to the fixed-point bound of 2^-32 per dyad
    for u in range(T - 1):
        sc = scored[u]
        bound = 2 * n_u[u] * 2.0 ** -32 + 1e-10                     # the reference's own fix and the device's unit
        assert abs(res.expected_persisted_t[u] - ref['persist'][u][sc].sum()) <= bound, label
        assert abs(res.expected_formed_t[u] - (ref['pbar1'][u][sc] - ref['persist'][u][sc]).sum()) <= 2 * bound
        assert abs(res.expected_dissolved_t[u] - (ref['pbar0'][u][sc] - ref['persist'][u][sc]).sum()) <= 2 * bound
        had = sc & (Y[u] != 0)
        if had.any():
            assert abs(res.persistence_expected_t[u] - ref['pbar1'][u][had].mean()) <= 2 * 2.0 ** -32 + 1e-12, label
            assert res.persistence_observed_t[u] == (Y[u + 1][had] != 0).sum() / had.sum()
    rose, fell = (ref['up'] >= res.min_count) & scored, (ref['down'] >= res.min_count) & scored
    np.testing.assert_array_equal(res.n_strengthened_t, rose.sum(axis=(1, 2)))
    np.testing.assert_array_equal(res.n_weakened_t, fell.sum(axis=(1, 2)))
    size = np.where(scored, np.abs(ref['pw'][..., 0]), 0.0)
    if directed:
        assert res.strengthened is None and res.turnover is None
        np.testing.assert_array_equal(res.strengthened_out, rose.sum(axis=2))
        np.testing.assert_array_equal(res.weakened_in, fell.sum(axis=1))
        np.testing.assert_allclose(res.turnover_out, size.sum(axis=2), rtol=0, atol=2 * N * 2.0 ** -32 + 1e-12)
        np.testing.assert_allclose(res.turnover_in, size.sum(axis=1), rtol=0, atol=2 * N * 2.0 ** -32 + 1e-12)
    else:
        assert res.strengthened_out is None and res.turnover_in is None
        np.testing.assert_array_equal(res.strengthened, rose.sum(axis=2) + rose.sum(axis=1))
        np.testing.assert_array_equal(res.weakened, fell.sum(axis=2) + fell.sum(axis=1))
        np.testing.assert_allclose(res.turnover, size.sum(axis=2) + size.sum(axis=1), rtol=0,
                                   atol=2 * N * 2.0 ** -32 + 1e-12)
    np.testing.assert_array_equal(res.prob_up_hist, np.array(ref['hist_up'], dtype=np.int64))
    top = res.top_changes(k=5)
    assert len(top) <= 5 and all(abs(a[3]) >= abs(b[3]) for a, b in zip(top, top[1:]))
    for u, i, j, dm, pu in top:
        assert dm == res.delta_mean[u, i, j] and max(ref['up'][u, i, j], ref['down'][u, i, j]) >= res.min_count
    text = res.summary()
    for word in ('persistence', 'formed', 'dissolved', 'strengthened'):
        assert word in text
    assert repr(res) == text
    return ref


@pytest.mark.parametrize('directed', [False, True])
def test_end_to_end_on_a_short_lsm_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 30
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.tie_dynamics(m)
    assert res.n_samples == m.Xs_.shape[0] - m.n_burn_ and res.sample_ids[0] == m.n_burn_
    assert res.n == (T - 1) * N * (N - 1) // (1 if directed else 2)
    _check_result(m, res, 'lsm dir=%d ' % directed)
    few = da.tie_dynamics(m, n_samples=30, level=0.6, pointwise=False, n_bins=10)
    assert few.n_samples == 30 and few.delta_mean is None and few.prob_down is None and few.n_bins == 10
    assert few.sample_ids[-1] == m.Xs_.shape[0] - 1 and few.n == res.n and few.min_count == 18
    assert few.observed_persisted == res.observed_persisted
    assert 0 < res.expected_persisted < res.n and 0 <= res.persistence_expected <= 1
    print(res.summary())


def test_end_to_end_on_a_sample_missing_fit(da):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 30
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=3)['Y']
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=False)
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, random_state=4, sample_missing=True).fit(Yt)
    res = da.tie_dynamics(m, n_samples=40)
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    ref = _check_result(m, res, 'held out ', held)
    assert index.shape[0] > 0 and res.n == int(ref['scored'].sum()) < (T - 1) * N * (N - 1) // 2
    # a held-out dyad is in the pointwise arrays of both of its steps
    t, i, j = index[0]
    for u in (t - 1, t):
        if 0 <= u < T - 1:
            assert not ref['scored'][u, min(i, j), max(i, j)] and res.delta_sd[u, i, j] > 0


def test_end_to_end_on_a_small_hdp_lpcm(da):
    from test_gpu_gof import _splitting
    Y = _splitting(30, 3, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=60, burn=20, tune=20, n_components=4, random_state=1).fit(Y)
    res = da.tie_dynamics(hdp)
    _check_result(hdp, res, 'hdp ')
    hdp.release_device_trace()                        # the call then makes a chain of its own
    again = da.tie_dynamics(hdp)
    assert again.counts == res.counts
    assert again.delta_mean.tobytes() == res.delta_mean.tobytes() and again.prob_up.tobytes() == res.prob_up.tobytes()
