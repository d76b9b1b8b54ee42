"""Tie dynamics without a GPU: the host restatement tests/dynamics_ref.py against a triple-loop brute force and the
identities of its tables, the arithmetic of TieDynamicsResult on hand-made tables, the facade's argument checks
(before the library is loaded), the C-ABI declaration and its binding, and the code object of the new kernel (no
scratch memory and no spilled register in any instantiation)."""
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

import dynamics_ref  # noqa: E402
import proba_ref  # noqa: E402
from standin_estimator import StandInEstimator  # noqa: E402

sys.path.insert(0, ROOT)
from dynetlsm_amd.dynamics import FIX, _min_count  # noqa: E402  (loads no library)

assert FIX == 1 << 32 == dynamics_ref.UNIT


def _small_case(directed, seed=0):
    rng = np.random.RandomState(seed + 10 * directed)
    S, T, N, D = 4, 3, 5, 2
    Xs = rng.randn(S, T, N, D)
    ic = np.stack([rng.uniform(0.5, 1.5, S), rng.uniform(0.2, 0.8, S) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    Y = (rng.rand(T, N, N) < 0.4).astype(np.int64)
    if not directed:
        Y = np.triu(Y, 1) + np.triu(Y, 1).transpose(0, 2, 1)
    Y[:, np.arange(N), np.arange(N)] = 0
    mask = np.zeros((T, N, N), dtype=bool)
    mask[1, 0, 3] = mask[0, 2, 1] = mask[2, 4, 0] = True          # (2, 1), (4, 0): the lower orientation
    return Y, Xs, ic, radii, mask


def _eta(Xs, ic, radii, directed, s, t, i, j):
    dist = math.sqrt(sum((Xs[s, t, i, d] - Xs[s, t, j, d]) ** 2 for d in range(Xs.shape[3])))
    if directed:
        return ic[s, 0] * (1 - dist / radii[s, j]) + ic[s, 1] * (1 - dist / radii[s, i])
    return ic[s, 0] - dist


def _expit(x):
    return 1 / (1 + math.exp(-x)) if x >= 0 else math.exp(x) / (1 + math.exp(x))


@pytest.mark.parametrize('directed', [False, True])
def test_reference_against_a_triple_loop(directed):
    Y, Xs, ic, radii, mask = _small_case(directed)
    S, T, N, _ = Xs.shape
    min_count, n_bins = _min_count(0.75, S), 4                     # what the facade passes at level 0.75: 3 of 4
    assert min_count == 3
    ref = dynamics_ref.reference(Y, Xs, ic, radii, directed, min_count, n_bins, mask)
    assert dynamics_ref.signs_are_stable(ref['eta'], ref['eta_ld'])
    tr = [[[0] * 4 for _ in range(4)] for _ in range(T - 1)]
    hist = [[0] * n_bins for _ in range(T - 1)]
    changes = [[[0] * 4 for _ in range(N)] for _ in range(T - 1)]
    turn = [[[0] * 2 for _ in range(N)] for _ in range(T - 1)]
    n_scored = 0
    for u in range(T - 1):
        for i in range(N):
            for j in range(N):
                if not (i != j if directed else i < j):
                    assert not ref['exists'][u, i, j] and not ref['pw'][u, i, j].any()
                    assert not ref['pw_ld'][u, i, j].any() and not ref['scored'][u, i, j]
                    continue
                assert ref['exists'][u, i, j]
                e0 = [_eta(Xs, ic, radii, directed, s, u, i, j) for s in range(S)]
                e1 = [_eta(Xs, ic, radii, directed, s, u + 1, i, j) for s in range(S)]
                p0, p1 = [_expit(e) for e in e0], [_expit(e) for e in e1]
                d = [b - a for a, b in zip(p0, p1)]
                mean = math.fsum(d) / S
                sd = math.sqrt(math.fsum((v - mean) ** 2 for v in d) / (S - 1))
                up = sum(b > a for a, b in zip(e0, e1))
                down = sum(b < a for a, b in zip(e0, e1))
                for key in ('pw', 'pw_ld'):
                    got = [float(v) for v in ref[key][u, i, j]]
                    assert abs(got[0] - mean) <= 1e-15 and abs(got[1] - sd) <= 1e-15, (key, got, mean, sd)
                    assert got[2] == up / S and got[3] == down / S
                assert ref['up'][u, i, j] == up and ref['down'][u, i, j] == down
                masked = any(mask[t, i, j] or (not directed and mask[t, j, i]) for t in (u, u + 1))
                assert ref['scored'][u, i, j] == (not masked)
                if masked:
                    continue
                n_scored += 1
                pbar0, pbar1 = math.fsum(p0) / S, math.fsum(p1) / S
                persist = math.fsum(a * b for a, b in zip(p0, p1)) / S
                row = tr[u][2 * int(Y[u, i, j] != 0) + int(Y[u + 1, i, j] != 0)]
                row[0] += 1
                for v, x in ((1, pbar0), (2, pbar1), (3, persist)):
                    row[v] += proba_ref.fix(x)
                hist[u][min(up * n_bins // S, n_bins - 1)] += 1
                if up >= min_count:
                    changes[u][i][0] += 1
                    changes[u][j][1] += 1
                if down >= min_count:
                    changes[u][i][2] += 1
                    changes[u][j][3] += 1
                turn[u][i][0] += proba_ref.fix(abs(mean))
                turn[u][j][1] += proba_ref.fix(abs(mean))
    assert n_scored == int(ref['scored'].sum()) and 0 < n_scored < (T - 1) * N * (N - 1) // (1 if directed else 2)
    assert ref['hist_up'] == hist and ref['node_changes'] == changes
    got = np.array(ref['transitions'], dtype=object)
    want = np.array(tr, dtype=object)
    assert (got[..., 0] == want[..., 0]).all()
    assert (abs(got - want) <= want[..., :1]).all()                # fsum against numpy's sum: a unit per dyad at most
    per_node = np.stack([ref['scored'].sum(axis=2), ref['scored'].sum(axis=1)], axis=-1).astype(object)
    assert (abs(np.array(ref['node_turnover'], dtype=object) - np.array(turn, dtype=object)) <= per_node).all()
    assert got[..., 0].sum() == n_scored and (got[:, 1:, 0].sum() > 0)          # some ties among them


@pytest.mark.parametrize('directed', [False, True])
def test_identities_of_the_reference_tables(directed):
    Y, Xs, ic, radii, mask = _small_case(directed, seed=3)
    ref = dynamics_ref.reference(Y, Xs, ic, radii, directed, 3, 7, mask)
    n_u = ref['scored'].sum(axis=(1, 2))
    for u, tab in enumerate(ref['transitions']):
        assert sum(row[0] for row in tab) == n_u[u] == sum(ref['hist_up'][u])
        s0, s1, sp = (sum(row[v] for row in tab) for v in (1, 2, 3))
        sc = ref['scored'][u]
        assert s0 == sum(proba_ref.fix(x) for x in ref['pbar0'][u][sc])
        assert s1 == sum(proba_ref.fix(x) for x in ref['pbar1'][u][sc])
        # expected formed - expected dissolved: the persisted part cancels exactly
        assert (s1 - sp) - (s0 - sp) == s1 - s0
        # every node's slots: a dyad enters one row slot and one column slot
        ch = np.array(ref['node_changes'][u], dtype=object)
        assert ch[:, 0].sum() == ch[:, 1].sum() == int(((ref['up'][u] >= 3) & sc).sum())
        assert ch[:, 2].sum() == ch[:, 3].sum() == int(((ref['down'][u] >= 3) & sc).sum())
        to = np.array(ref['node_turnover'][u], dtype=object)
        assert to[:, 0].sum() == to[:, 1].sum()
    # min_count above S / 2: no dyad is in both
    assert not ((ref['up'] >= 3) & (ref['down'] >= 3)).any()
    # the same identity through the result object
    import dynetlsm_amd as da
    res = da.TieDynamicsResult(np.arange(4), 4, 0.75, 3, ref['transitions'], ref['hist_up'], ref['node_changes'],
                               ref['node_turnover'], directed, 5)
    tr = ref['transitions']
    for u in range(2):
        s0, s1 = (sum(row[v] for row in tr[u]) for v in (1, 2))
        assert res.expected_formed_t[u] - res.expected_dissolved_t[u] == pytest.approx((s1 - s0) / FIX, abs=1e-12)


def test_signs_are_stable_is_a_precondition_on_the_inputs():
    eta = np.zeros((2, 3, 2, 2))
    assert dynamics_ref.signs_are_stable(eta, eta.astype(np.longdouble))         # exact ties
    eta[:, 1] = 1.0
    assert dynamics_ref.signs_are_stable(eta)
    eta[0, 2, 0, 1] = 1.0 + 1e-12                                                # a difference a rounding could flip
    assert not dynamics_ref.signs_are_stable(eta)
    big = np.zeros((1, 2, 1, 1))
    big[0, 0], big[0, 1] = 800.0, 800.0 + 1e-7                                   # relative to |eta|
    assert not dynamics_ref.signs_are_stable(big)
    assert dynamics_ref.up_bin([0, 5, 9, 10], 4, 10).tolist() == [0, 2, 3, 3]


def _hand_made(directed):
    """U = 2 steps, N = 3.  Step 1 has no tie at t: its persistence rate has an empty denominator"""
    q = FIX // 4
    transitions = [[[10, 4 * q, 6 * q, 1 * q], [2, 2 * q, 5 * q, 1 * q], [3, 8 * q, 4 * q, 3 * q],
                    [5, 16 * q, 18 * q, 15 * q]],
                   [[7, 4 * q, 4 * q, 1 * q], [1, 1 * q, 3 * q, 1 * q], [0, 0, 0, 0], [0, 0, 0, 0]]]
    hist_up = [[12, 3, 5], [8, 0, 0]]
    node_changes = [[[2, 0, 1, 0], [1, 1, 0, 1], [0, 2, 0, 0]], [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]]
    node_turnover = [[[q, 0], [2 * q, q], [0, 2 * q]], [[0, 0], [q, 0], [0, q]]]
    return transitions, hist_up, node_changes, node_turnover


def test_result_arithmetic_on_hand_made_tables():
    import dynetlsm_amd as da
    tr, hist, changes, turn = _hand_made(False)
    as_u64 = [np.array(a, dtype=np.uint64) for a in (tr, hist, changes, turn)]
    for directed in (False, True):
        res = da.TieDynamicsResult(np.arange(10, 30), 20, 0.9, 18, *as_u64, is_directed=directed, n_nodes=3)
        assert res.n_samples == 20 and res.level == 0.9 and res.min_count == 18 and res.n_steps == 2
        assert res.counts['transitions'] == tr and res.counts['node_turnover'] == turn
        assert all(type(v) is int for v in res.counts['transitions'][0][0])
        np.testing.assert_array_equal(res.n_t, [20, 8])
        np.testing.assert_array_equal(res.observed_persisted_t, [5, 0])
        np.testing.assert_array_equal(res.observed_formed_t, [2, 1])
        np.testing.assert_array_equal(res.observed_dissolved_t, [3, 0])
        assert (res.n, res.observed_persisted, res.observed_formed, res.observed_dissolved) == (28, 5, 3, 3)
        # sums in quarters: persist 20 and 2, pbar_t 30 and 5, pbar_{t+1} 33 and 7
        np.testing.assert_array_equal(res.expected_persisted_t, [5.0, 0.5])
        np.testing.assert_array_equal(res.expected_formed_t, [(33 - 20) / 4, (7 - 2) / 4])
        np.testing.assert_array_equal(res.expected_dissolved_t, [(30 - 20) / 4, (5 - 2) / 4])
        assert res.expected_persisted == 5.5 and res.expected_formed == 4.5 and res.expected_dissolved == 3.25
        # rates: persistence over y_t = 1 (classes 2 and 3), formation over y_t = 0 (classes 0 and 1)
        assert res.persistence_observed_t[0] == 5 / 8 and np.isnan(res.persistence_observed_t[1])
        assert res.persistence_expected_t[0] == (4 + 18) / 4 / 8 and np.isnan(res.persistence_expected_t[1])
        assert res.formation_observed_t.tolist() == [2 / 12, 1 / 8]
        assert res.formation_expected_t.tolist() == [(6 + 5) / 4 / 12, (4 + 3) / 4 / 8]
        assert res.persistence_observed == 5 / 8 and res.persistence_expected == 22 / 4 / 8
        assert res.formation_observed == 3 / 20 and res.formation_expected == 18 / 4 / 20
        np.testing.assert_array_equal(res.n_strengthened_t, [3, 0])
        np.testing.assert_array_equal(res.n_weakened_t, [1, 1])
        np.testing.assert_array_equal(res.prob_up_hist, hist)
        if directed:
            assert res.strengthened is None and res.weakened is None and res.turnover is None
            np.testing.assert_array_equal(res.strengthened_out, [[2, 1, 0], [0, 0, 0]])
            np.testing.assert_array_equal(res.strengthened_in, [[0, 1, 2], [0, 0, 0]])
            np.testing.assert_array_equal(res.weakened_out, [[1, 0, 0], [0, 1, 0]])
            np.testing.assert_array_equal(res.weakened_in, [[0, 1, 0], [0, 0, 1]])
            np.testing.assert_array_equal(res.turnover_out, [[0.25, 0.5, 0], [0, 0.25, 0]])
            np.testing.assert_array_equal(res.turnover_in, [[0, 0.25, 0.5], [0, 0, 0.25]])
        else:
            assert res.strengthened_out is None and res.weakened_in is None and res.turnover_out is None
            np.testing.assert_array_equal(res.strengthened, [[2, 2, 2], [0, 0, 0]])
            np.testing.assert_array_equal(res.weakened, [[1, 1, 0], [0, 1, 1]])
            np.testing.assert_array_equal(res.turnover, [[0.25, 0.75, 0.5], [0, 0.25, 0.25]])
        assert res.delta_mean is None and res.prob_down is None
        with pytest.raises(ValueError, match='pointwise'):
            res.top_changes()
        text = res.summary()
        for word in ('persistence', 'formed', 'dissolved', 'strengthened', 'nan'):
            assert word in text, word
        assert repr(res) == text
    # nothing scored at all: NaN rates, no error; sums beyond 2^53 stay exact
    empty = da.TieDynamicsResult(np.arange(2), 2, 0.9, 2, np.zeros((1, 4, 4), dtype=np.uint64),
                                 np.zeros((1, 5), dtype=np.uint64), np.zeros((1, 3, 4), dtype=np.uint64),
                                 np.zeros((1, 3, 2), dtype=np.uint64), False, 3)
    assert empty.n == 0 and np.isnan(empty.persistence_observed) and np.isnan(empty.formation_expected_t).all()
    assert 'persistence' in empty.summary()
    big = np.zeros((1, 4, 4), dtype=np.uint64)
    big[0, 3] = [1 << 31, (1 << 62) + 1, (1 << 62) + 1, 1 << 61]
    res = da.TieDynamicsResult(np.arange(2), 2, 0.9, 2, big, np.zeros((1, 5), dtype=np.uint64),
                               np.zeros((1, 3, 4), dtype=np.uint64), np.zeros((1, 3, 2), dtype=np.uint64), False, 3)
    assert res.counts['transitions'][0][3][1] == (1 << 62) + 1 and res.persistence_expected == ((1 << 62) + 1) / (
        (1 << 31) * FIX)


def test_pointwise_arrays_and_top_changes():
    import dynetlsm_amd as da
    U, N, S = 2, 4, 10
    zeros = (np.zeros((U, 4, 4), dtype=np.uint64), np.zeros((U, 3), dtype=np.uint64),
             np.zeros((U, N, 4), dtype=np.uint64), np.zeros((U, N, 2), dtype=np.uint64))
    pw = np.zeros((U, N, N, 4))
    # (step, i, j): delta_mean, prob_up, prob_down
    for (u, i, j), (dm, pu, pd) in {(0, 0, 1): (0.30, 1.0, 0.0), (0, 1, 2): (-0.50, 0.1, 0.9),
                                    (0, 0, 3): (0.90, 0.8, 0.2),       # large but not certain at 9 of 10
                                    (1, 2, 3): (-0.10, 0.0, 1.0), (1, 0, 2): (0.40, 0.9, 0.0)}.items():
        pw[u, i, j] = (dm, 0.05, pu, pd)
    und = da.TieDynamicsResult(np.arange(S), S, 0.9, 9, *zeros, is_directed=False, n_nodes=N, pointwise=pw)
    for a in (und.delta_mean, und.delta_sd, und.prob_up, und.prob_down):
        np.testing.assert_array_equal(a, a.transpose(0, 2, 1))
        assert not a[:, np.arange(N), np.arange(N)].any()
    np.testing.assert_array_equal(np.triu(und.delta_mean, 1), pw[..., 0])
    assert und.top_changes() == [(0, 1, 2, -0.5, 0.1), (1, 0, 2, 0.4, 0.9), (0, 0, 1, 0.3, 1.0), (1, 2, 3, -0.1, 0.0)]
    assert und.top_changes(k=2) == und.top_changes()[:2]
    assert und.top_changes(step=1) == [(1, 0, 2, 0.4, 0.9), (1, 2, 3, -0.1, 0.0)]
    assert und.top_changes(k=1, step=0) == [(0, 1, 2, -0.5, 0.1)]
    with pytest.raises(ValueError, match='step'):
        und.top_changes(step=2)
    dire = da.TieDynamicsResult(np.arange(S), S, 0.9, 9, *zeros, is_directed=True, n_nodes=N, pointwise=pw)
    np.testing.assert_array_equal(dire.delta_mean, pw[..., 0])
    assert dire.top_changes(k=1) == [(0, 1, 2, -0.5, 0.1)]


def _fitted(T=3, n_iter=20, burn=8):
    est = StandInEstimator(n_iter=n_iter, burn=burn).fit(np.zeros((T, 5, 5)))
    est.is_directed = False
    est.Y_fit_ = np.zeros((T, 5, 5))
    est.Xs_ = np.zeros((n_iter, T, 5, 2))
    return est


def test_facade_argument_checks_come_before_any_device_call():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    loaded = _lib._LIB
    with pytest.raises(ValueError, match='not fit'):
        da.tie_dynamics(StandInEstimator())
    for level in (0.5, 1.0, 0.0, 0.3, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='level'):
            da.tie_dynamics(_fitted(), level=level)
    for n_bins in (0, 65, 2.5):
        with pytest.raises(ValueError, match='n_bins'):
            da.tie_dynamics(_fitted(), n_bins=n_bins)
    for bad in (0, -3, 2.5, 13):               # 12 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.tie_dynamics(_fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='two samples'):
        da.tie_dynamics(_fitted(), n_samples=1)
    with pytest.raises(ValueError, match='two samples'):
        da.tie_dynamics(_fitted(burn=19))
    with pytest.raises(ValueError, match='two time steps'):
        da.tie_dynamics(_fitted(T=1))
    assert _lib._LIB is loaded                                     # none of this loaded the library
    assert [_min_count(0.9, S) for S in (2, 10, 11, 100)] == [2, 9, 10, 90]
    assert _min_count(0.7, 10) == 7 and _min_count(0.51, 2) == 2 and _min_count(0.999, 20) == 20


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build, dependencies
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_dynamics_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_dynamics_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 14 and args[0].startswith('dlsm_chain') and args[-1].endswith('pointwise')
    assert args[7] == 'int min_count' and args[8] == 'int n_bins'
    res, argtypes = _lib.SIGNATURES['dlsm_dynamics_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[7] is ctypes.c_int and argtypes[9] is _lib.c_u64_p
    lib = ctypes.CDLL(build())
    assert hasattr(lib, 'dlsm_dynamics_accumulate') and lib.dlsm_abi_version() == 1
    assert callable(da.tie_dynamics) and callable(da.Chain.dynamics_accumulate)
    for name in ('dynamics', 'tie_dynamics', 'TieDynamicsResult'):
        assert name in da.__all__ and hasattr(da, name)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dlsm_dynamics_accumulate(' in doc
    names = {os.path.basename(d) for d in dependencies()}
    assert {'kernels_dynamics.hpp', 'capi_dynamics.hpp'} <= names


def test_every_instantiation_of_the_kernel_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_dyn_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        assert md[name]['vgpr'] <= 512, (name, md[name])
        # two time steps x two buffers of a sample's block stay under 24 KB; with the tables, under 32 KB
        assert md[name]['lds'] <= (32 << 10), (name, md[name])
    assert sorted(k for k in md if k.startswith('k_dyn_')) == sorted(names)
