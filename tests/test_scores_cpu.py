"""In-sample scores without a GPU: ScoreResult from hand-made counts, the rank key, and the host
restatement tests/score_ref.py against scikit-learn's AUC of the probabilities themselves."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import score_cases  # noqa: E402
import score_ref  # noqa: E402

# roc_auc_score integrates the ROC curve in float64: its own rounding, a few ulp of a number below 1
SKLEARN_ULPS = 8 * np.finfo(np.float64).eps


def test_score_result_from_hand_made_counts():
    from dynetlsm_amd.scores import scores_from_counts, ScoreResult
    # t = 0: positives all above the negatives; t = 1: 3 positives, 4 negatives, u2 = 15, one tied pair
    counts = [[2, 3, 12, 0], [3, 4, 15, 1], [5, 7, 40, 3]]
    res = scores_from_counts(counts, [1.5, 3.5], sample_ids=np.arange(4), is_directed=True)
    assert isinstance(res, ScoreResult)
    assert res.auc_t.tolist() == [1.0, 15 / 24] and res.auc_bound_t.tolist() == [0.0, 1 / 24]
    assert res.auc == 40 / 70 and res.auc_bound == 3 / 70
    assert res.n_pos == 5 and res.n_neg == 7 and res.n == 12
    assert res.n_pos_t.tolist() == [2, 3] and res.n_neg_t.tolist() == [3, 4] and res.n_t.tolist() == [5, 7]
    assert res.log_loss_t.tolist() == [1.5 / 5, 3.5 / 7] and res.log_loss == 5.0 / 12
    text = res.summary()
    assert 'auc_bound' in text and 'log_loss' in text and 't=1' in text and '4 samples' in text
    # the same from what the device returns: a uint64 array
    again = scores_from_counts(np.array(counts, dtype=np.uint64), np.array([1.5, 3.5]))
    assert again.auc == res.auc and again.auc_bound == res.auc_bound and again.sample_ids is None
    with pytest.raises(ValueError):
        scores_from_counts(counts, [1.5])


def test_score_result_with_an_empty_class_and_with_all_ties():
    from dynetlsm_amd.scores import scores_from_counts
    # t = 0 has no positive; t = 1 is one bin: u2 = pos * neg = ties
    res = scores_from_counts([[0, 6, 0, 0], [4, 5, 20, 20], [4, 11, 20 + 2 * 4 * 6, 20]], [0.25, 9.0])
    assert math.isnan(res.auc_t[0]) and math.isnan(res.auc_bound_t[0]) and res.log_loss_t[0] == 0.25 / 6
    assert res.auc_t[1] == 0.5 and res.auc_bound_t[1] == 0.5
    assert res.auc == 68 / 88 and res.auc_bound == 20 / 88
    # nothing scored at all
    none = scores_from_counts([[0, 0, 0, 0], [0, 0, 0, 0]], [0.0])
    assert none.n == 0 and math.isnan(none.auc) and math.isnan(none.auc_bound) and math.isnan(none.log_loss)
    assert 'nan' in none.summary()


def test_score_result_divides_exact_integers_beyond_float_range():
    """u2 near 2^64: the quotient is that of the integers, not of their float64 roundings"""
    from dynetlsm_amd.scores import scores_from_counts
    n_pos, n_neg = 3 * 2 ** 30 + 1, 2 ** 31 - 3
    u2 = 2 * n_pos * n_neg - 12345
    assert 2 ** 63 < u2 < 2 ** 64
    res = scores_from_counts(np.array([[n_pos, n_neg, u2, 7]] * 2, dtype=np.uint64), [1.0])
    assert res.counts[1][2] == u2
    assert res.auc == u2 / (2 * n_pos * n_neg) and res.auc < 1.0
    assert res.auc_bound == 7 / (2 * n_pos * n_neg)


def test_key_is_monotone_and_clamped():
    rng = np.random.RandomState(0)
    p = np.sort(np.concatenate([rng.rand(20000), np.exp(rng.uniform(-60, 0, 20000)),
                                [0.0, 1e-300, 2.0 ** -64, 2.0 ** -63, 2.0 ** -63 * (1 + 2.0 ** -14), 0.5, 1.0]]))
    k = score_ref.key(p)
    assert (np.diff(k) >= 0).all()
    assert k.min() == score_ref.KEY_LO and k.max() == score_ref.KEY_HI
    assert score_ref.key(0.0) == score_ref.key(2.0 ** -80) == score_ref.key(2.0 ** -63) == score_ref.KEY_LO
    assert score_ref.key(2.0 ** -63 * (1 + 2.0 ** -15)) == score_ref.KEY_LO + 1
    assert score_ref.key(1.0) == score_ref.KEY_HI == score_ref.KEY_LO + score_ref.N_BINS - 1
    assert score_ref.N_BINS == 2064385
    # 2^15 bins per octave
    assert score_ref.key(0.5) - score_ref.key(0.25) == 2 ** 15
    # the stability precondition sees a probability next to a bin's edge: half a float32 ulp below the
    # bin's first float32, where the conversion from float64 turns
    assert score_ref.keys_are_stable(np.array([0.3, 0.7]))
    lo = (np.float32(0.3).view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)
    edge = (float(lo) + float(np.nextafter(lo, np.float32(0)))) / 2
    assert score_ref.key(edge * (1 + 1e-12)) == score_ref.key(edge * (1 - 1e-12)) + 1
    assert score_ref.keys_are_stable(np.array([float(lo)])) and not score_ref.keys_are_stable(np.array([edge]))


def test_rank_counts_against_brute_force():
    rng = np.random.RandomState(1)
    k = score_ref.KEY_LO + rng.randint(0, 40, 300)
    y = rng.rand(300) < 0.3
    n_pos, n_neg, u2, ties = score_ref.rank_counts(k, y)
    kp, kn = k[y][:, None], k[~y][None, :]
    assert (n_pos, n_neg) == (int(y.sum()), int((~y).sum()))
    assert u2 == 2 * int((kp > kn).sum()) + int((kp == kn).sum()) and ties == int((kp == kn).sum())


@pytest.mark.parametrize('index', range(len(score_cases.CASES)), ids=score_cases.IDS)
def test_key_auc_is_within_its_bound_of_the_exact_auc(index):
    (Y, Xs, ic, radii, mask), ref = score_cases.case(index)
    N, T, D, S, directed, masked, _ = score_cases.CASES[index]
    assert score_cases.stable(ref)                        # what the device test relies on
    n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
    if not masked:
        assert ref['counts'][T][0] + ref['counts'][T][1] == T * n_dyads
    else:
        assert 0 < ref['counts'][T][0] + ref['counts'][T][1] < 0.95 * T * n_dyads
    for c in (0, 1):                                      # the classes of the steps add up to the pooled ones
        assert sum(row[c] for row in ref['counts'][:T]) == ref['counts'][T][c]
    for row, exact in zip(ref['counts'], list(ref['auc_exact_t']) + [ref['auc_exact']]):
        auc, bound = score_ref.auc_of_counts(row)
        assert 0 <= bound <= 0.5 and abs(auc - exact) <= bound + SKLEARN_ULPS, (row, auc, exact, bound)
    # the two evaluations of the log-loss: -log mean exp(l_s) against pbar itself
    p = ref['pbar']
    direct = -np.where(ref['scored'], np.where(Y != 0, np.log(p), np.log1p(-p)), 0.0).sum(axis=(1, 2))
    np.testing.assert_allclose(ref['logloss'], direct, rtol=1e-12)
    # and through the package's plain function
    from dynetlsm_amd.scores import scores_from_counts
    res = scores_from_counts(ref['counts'], ref['logloss'], is_directed=directed)
    assert res.auc == score_ref.auc_of_counts(ref['counts'][T])[0]
    assert abs(res.auc - ref['auc_exact']) <= res.auc_bound + SKLEARN_ULPS


def test_the_facade_rejects_what_information_criteria_rejects():
    import dynetlsm_amd as da
    with pytest.raises(ValueError, match='not fit'):
        da.in_sample_scores(da.DynamicNetworkLSM())

    class Fitted(object):
        is_directed = False
        n_burn_ = 4
        Y_fit_ = np.zeros((2, 5, 5))
        intercepts_ = np.zeros((10, 1))
        Xs_ = np.zeros((10, 2, 5, 2))

    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match='positive integer'):
            da.in_sample_scores(Fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='exceeds the 6 kept samples'):
        da.in_sample_scores(Fitted(), n_samples=7)
    with pytest.raises(ValueError, match='estimate'):
        da.in_sample_scores(Fitted(), estimate='mean')


def test_excluded_dyads_follow_missing_index_and_nan_mask():
    from dynetlsm_amd.scores import _excluded_dyads

    class M(object):
        pass

    m = M()
    assert _excluded_dyads(m, (2, 4, 4), False) is None
    m.missing_index_ = np.array([[0, 1, 3], [1, 0, 2]])
    ex = _excluded_dyads(m, (2, 4, 4), False)
    assert ex.sum() == 2 and ex[0, 1, 3] and ex[1, 0, 2]
    # nan_mask_: one entry per dyad in the order of metrics.network_auc (undirected: t, i < j row-major)
    n = M()
    n.nan_mask_ = np.zeros(2 * 6, dtype=bool)
    n.nan_mask_[[1, 6 + 5]] = True                        # (0, 0, 2) and (1, 2, 3)
    ex = _excluded_dyads(n, (2, 4, 4), False)
    assert ex.sum() == 2 and ex[0, 0, 2] and ex[1, 2, 3]
    d = M()
    d.nan_mask_ = np.zeros(2 * 12, dtype=bool)
    d.nan_mask_[[3, 12 + 11]] = True                      # (0, 1, 0) and (1, 3, 2)
    ex = _excluded_dyads(d, (2, 4, 4), True)
    assert ex.sum() == 2 and ex[0, 1, 0] and ex[1, 3, 2]


def test_header_binding_and_library_agree_on_the_entry_point():
    import ctypes
    import re
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_score_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_score_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 9 and args[2].endswith('mask') and args[-1].endswith('logloss_sum')
    assert len(_lib.SIGNATURES['dlsm_score_accumulate'][1]) == len(args)
    assert hasattr(ctypes.CDLL(build()), 'dlsm_score_accumulate')


def test_every_instantiation_of_the_kernels_is_free_of_scratch_memory():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'profiles'))
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_score_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    names += ['k_score_scan', 'k_score_reduce_logloss']
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        # a 256-thread workgroup must fit a SIMD's 512 registers per lane
        assert md[name]['vgpr'] <= 512, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_score_')) == sorted(names)
