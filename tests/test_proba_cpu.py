"""Posterior edge probabilities without a GPU: the host restatement tests/proba_ref.py against a dyad worked out by
hand, the arithmetic of EdgeProbabilityResult against brute force on the integer tables, the facade's argument
checks (before the library is loaded), the C-ABI declaration and its binding, and the code object of the new
kernel (no scratch memory and no spilled register in any instantiation)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import proba_ref  # noqa: E402

EDGES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)


def test_reference_against_a_dyad_worked_out_by_hand():
    """S = 5, two nodes at distance 1 with intercepts 2, 0, 1, -1, 3: eta = 1, -1, 0, -2, 2.  level 0.8: alpha =
    0.1, the positions 0.4 and 3.6 of the sorted p: both quantiles are interpolated"""
    eta = [1.0, -1.0, 0.0, -2.0, 2.0]
    p = [1.0 / (1.0 + math.exp(-e)) for e in eta]
    srt = sorted(p)
    mean = math.fsum(p) / 5
    sd = math.sqrt(math.fsum((v - mean) ** 2 for v in p) / 4)
    lower = srt[0] + 0.4 * (srt[1] - srt[0])
    upper = srt[3] + 0.6 * (srt[4] - srt[3])
    Xs = np.zeros((5, 1, 2, 1))
    Xs[:, 0, 1, 0] = 1.0
    ic = np.stack([np.array(eta) + 1.0, np.zeros(5)], axis=1)
    Y = np.array([[[0, 1], [1, 0]]])
    edges = (0.5, 0.8)
    ref = proba_ref.reference(Y, Xs, ic, None, False, 0.8, 4, edges)
    for key in ('pw', 'pw_ld'):
        got = ref[key][0, 0, 1]
        for g, want in zip(got, (mean, sd, lower, upper)):
            assert abs(float(g) - want) <= 4 * np.spacing(want), (key, float(g), want)
        assert not ref[key][0, 1, 0].any() and not ref[key][0, 0, 0].any()
    assert abs(mean - 0.5) < 1e-15                                 # the etas are symmetric about 0
    # the tables of this one dyad: bin floor(0.5 * 4) = 2 (or 1 if the mean rounds below 1/2), y = 1
    b = int(proba_ref.mean_bin(ref['pw'][0, 0, 1, 0], 4))
    q = proba_ref.fix(ref['pw'][0, 0, 1, 0])
    assert abs(q - (1 << 31)) <= 1
    assert ref['calib'][0][b] == [1, 1, q] and sum(r[0] for r in ref['calib'][0]) == 1
    assert abs(ref['brier'][0] - (1 << 30)) <= 1                   # (1 - 1/2)^2
    assert ref['node_sums'][0] == [[q, 0], [0, q]]
    width = upper - lower
    assert 0.5 < width < 0.8 and ref['hist'][0] == [0, 1, 0]
    # numpy's positions: 0.1 * 4 and 0.9 * 4 of five values
    assert proba_ref.fix(0.0) == 0 and proba_ref.fix(1.0) == 1 << 32 and proba_ref.fix(0.75) == 3 << 30
    # expit saturates without overflow
    big = proba_ref.expit(np.array([-800.0, 800.0, -40.0]))
    assert big[0] == 0 and big[1] == 1 and 0 < big[2] < 1e-17


def _synthetic_tables(rng, T, N, n_bins, directed):
    """integer tables of random scored dyads with a bin and a class left empty, and what they were made from"""
    exists = np.broadcast_to(proba_ref.score_ref.dyad_mask(N, directed), (T, N, N))
    scored = exists & (rng.rand(T, N, N) < 0.8)
    pw = np.zeros((T, N, N, 4))
    pbar = rng.beta(0.6, 2.0, (T, N, N))
    pbar[(pbar >= 2.0 / n_bins) & (pbar < 3.0 / n_bins)] *= 0.1    # bin 2 stays empty
    pw[..., 0] = pbar
    pw[..., 2] = pbar * rng.uniform(0.3, 1.0, pbar.shape)
    pw[..., 3] = np.minimum(1.0, pbar + rng.uniform(0.0, 0.4, pbar.shape))
    Y = (rng.rand(T, N, N) < pbar).astype(np.int64)
    Y[T - 1] = 0                                                   # the last time step has no tie
    return Y, pw, scored, proba_ref.tables(Y, pw, scored, n_bins, EDGES)


def test_result_arithmetic_against_brute_force():
    import dynetlsm_amd as da
    from dynetlsm_amd.probabilities import _observed_degrees
    rng = np.random.RandomState(4)
    for directed in (False, True):
        T, N, nb = 3, 14, 10
        Y, pw, scored, (calib, brier, node, hist) = _synthetic_tables(rng, T, N, nb, directed)
        excluded = ~scored
        if not directed:                                           # either orientation excludes
            excluded = np.triu(excluded, 1)
            excluded[0] = excluded[0].T
        obs = _observed_degrees(Y != 0, excluded, directed)
        res = da.EdgeProbabilityResult(np.arange(50), 50, 0.9, np.array(calib, dtype=np.uint64),
                                       np.array(brier, dtype=np.uint64), np.array(node, dtype=np.uint64), EDGES,
                                       np.array(hist, dtype=np.uint64), obs, directed, N, pw)
        p, y = pw[..., 0], (Y != 0)
        for t in list(range(T)) + [T]:
            sc = scored[t] if t < T else scored
            pt, yt = (p[t][sc], y[t][sc]) if t < T else (p[sc], y[sc])
            n = int(sc.sum())
            bins = proba_ref.mean_bin(pt, nb)
            got_brier = res.brier_t[t] if t < T else res.brier
            got_ece = res.ece_t[t] if t < T else res.ece
            np.testing.assert_allclose(got_brier, np.mean((yt - pt) ** 2), rtol=0, atol=2.0 ** -32)
            ece = 0.0
            for b in range(nb):
                at = bins == b
                cal = res.calibration
                assert cal['n'][t, b] == at.sum() and cal['ties'][t, b] == yt[at].sum()
                if at.any():
                    np.testing.assert_allclose(cal['mean_predicted'][t, b], pt[at].mean(), rtol=0, atol=2.0 ** -32)
                    assert cal['observed_frequency'][t, b] == yt[at].sum() / at.sum()
                    ece += at.sum() / n * abs(yt[at].mean() - pt[at].mean())
                else:
                    assert np.isnan(cal['mean_predicted'][t, b]) and np.isnan(cal['observed_frequency'][t, b])
            np.testing.assert_allclose(got_ece, ece, rtol=0, atol=2.0 ** -32)
            want = proba_ref.calibration(calib[t], brier[t]) if t < T else None
            if want is not None:
                assert res.n_t[t] == want[0] == n
                np.testing.assert_allclose(res.brier_t[t], want[2], rtol=1e-14)
                np.testing.assert_allclose(res.ece_t[t], want[3], rtol=1e-12)
        assert np.isnan(res.calibration['mean_predicted'][:, 2]).all() and (res.calibration['n'][:, 2] == 0).all()
        assert res.n_ties_t[T - 1] == 0 and (res.calibration['observed_frequency'][T - 1][
            res.calibration['n'][T - 1] > 0] == 0).all()
        assert res.n == int(scored.sum()) == res.n_t.sum() and res.n_ties == int(y[scored].sum())
        np.testing.assert_array_equal(res.calibration['n'][T], res.calibration['n'][:T].sum(axis=0))
        np.testing.assert_array_equal(res.width_hist, res.width_hist_t.sum(axis=0))
        assert res.width_hist.sum() == res.n
        ps, ys = np.where(scored, p, 0.0), y & scored
        if directed:
            np.testing.assert_allclose(res.expected_out_degree, ps.sum(axis=2), rtol=0, atol=N * 2.0 ** -32)
            np.testing.assert_allclose(res.expected_in_degree, ps.sum(axis=1), rtol=0, atol=N * 2.0 ** -32)
            np.testing.assert_array_equal(res.observed_out_degree, ys.sum(axis=2))
            np.testing.assert_array_equal(res.observed_in_degree, ys.sum(axis=1))
            assert res.expected_degree is None
            np.testing.assert_array_equal(res.mean, p)
        else:
            np.testing.assert_allclose(res.expected_degree, ps.sum(axis=2) + ps.sum(axis=1), rtol=0,
                                       atol=N * 2.0 ** -32)
            np.testing.assert_array_equal(res.observed_degree, ys.sum(axis=2) + ys.sum(axis=1))
            assert res.expected_out_degree is None
        text = res.summary()
        assert 'brier' in text and 'ece' in text and 'reliability' in text and 'nan' in text and repr(res) == text
    # nothing scored at all: NaN scores, no error
    empty = da.EdgeProbabilityResult(np.arange(2), 2, 0.9, np.zeros((1, 4, 3), dtype=np.uint64),
                                     np.zeros(1, dtype=np.uint64), np.zeros((1, 3, 2), dtype=np.uint64), EDGES,
                                     np.zeros((1, 8), dtype=np.uint64), (np.zeros((1, 3)), np.zeros((1, 3))), False, 3)
    assert np.isnan(empty.brier) and np.isnan(empty.ece) and np.isnan(empty.brier_t).all() and empty.n == 0
    assert empty.mean is None and 'brier' in empty.summary()
    # sums beyond 2^53 stay exact: Python ints
    big = da.EdgeProbabilityResult(np.arange(2), 2, 0.9, np.array([[[1 << 31, 5, (1 << 62) + 1]]], dtype=np.uint64),
                                   np.array([1 << 61], dtype=np.uint64), np.zeros((1, 3, 2), dtype=np.uint64), EDGES,
                                   np.zeros((1, 8), dtype=np.uint64), (np.zeros((1, 3)), np.zeros((1, 3))), False, 3)
    assert big.counts['calib'][0][0][2] == (1 << 62) + 1 and big.brier == 0.25


def test_undirected_pointwise_arrays_are_symmetric_with_a_zero_diagonal():
    import dynetlsm_amd as da
    rng = np.random.RandomState(1)
    T, N = 2, 6
    pw = np.where(np.triu(np.ones((N, N), dtype=bool), 1)[None, :, :, None], rng.rand(T, N, N, 4), 0.0)
    res = da.EdgeProbabilityResult(np.arange(2), 2, 0.9, np.zeros((T, 4, 3), dtype=np.uint64),
                                   np.zeros(T, dtype=np.uint64), np.zeros((T, N, 2), dtype=np.uint64), EDGES,
                                   np.zeros((T, 8), dtype=np.uint64), (np.zeros((T, N)), np.zeros((T, N))), False, N,
                                   pw)
    for c, a in enumerate((res.mean, res.sd, res.lower, res.upper)):
        np.testing.assert_array_equal(a, a.transpose(0, 2, 1))
        assert not a[:, np.arange(N), np.arange(N)].any()
        np.testing.assert_array_equal(np.triu(a, 1), pw[..., c])


def test_facade_argument_checks_come_before_any_device_call():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib

    class Unfitted(object):
        pass

    class Fitted(object):
        is_directed = False
        n_burn_ = 4
        Y_fit_ = np.zeros((2, 5, 5))
        Xs_ = np.zeros((10, 2, 5, 2))
        intercepts_ = np.zeros((10, 1))

    loaded = _lib._LIB
    with pytest.raises(ValueError, match='not fit'):
        da.edge_probabilities(Unfitted())
    for level in (0.0, 1.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='level'):
            da.edge_probabilities(Fitted(), level=level)
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.edge_probabilities(Fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='two samples'):
        da.edge_probabilities(Fitted(), n_samples=1)

    class OneRow(Fitted):
        n_burn_ = 9
    with pytest.raises(ValueError, match='two samples'):
        da.edge_probabilities(OneRow())
    with pytest.raises(ValueError, match='16'):
        da.edge_probabilities(Fitted(), width_edges=np.linspace(0.01, 0.9, 17))
    for edges in ((0.2, 0.1), (0.1, 0.1), (0.1, float('inf')), (float('nan'),)):
        with pytest.raises(ValueError, match='ascending'):
            da.edge_probabilities(Fitted(), width_edges=edges)
    for n_bins in (0, 65, 2.5):
        with pytest.raises(ValueError, match='n_bins'):
            da.edge_probabilities(Fitted(), n_bins=n_bins)
    assert _lib._LIB is loaded                                     # none of this loaded the library


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build, dependencies
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_proba_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_proba_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 16 and args[0].startswith('dlsm_chain') and args[-1].endswith('pointwise')
    res, argtypes = _lib.SIGNATURES['dlsm_proba_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[7] is ctypes.c_double and args[7] == 'double level'
    assert hasattr(ctypes.CDLL(build()), 'dlsm_proba_accumulate')
    assert callable(da.edge_probabilities) and callable(da.Chain.proba_accumulate)
    for name in ('edge_probabilities', 'EdgeProbabilityResult'):
        assert name in da.__all__
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dlsm_proba_accumulate(' in doc
    names = {os.path.basename(d) for d in dependencies()}
    assert {'kernels_proba.hpp', 'capi_proba.hpp'} <= names


def test_every_instantiation_of_the_kernel_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_proba_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        assert md[name]['vgpr'] <= 512, (name, md[name])
        # the static part leaves the 144 KB of the two columns within the 160 KB of a workgroup
        assert md[name]['lds'] + (144 << 10) <= (160 << 10), (name, md[name])
    assert sorted(k for k in md if k.startswith('k_proba_')) == sorted(names)
