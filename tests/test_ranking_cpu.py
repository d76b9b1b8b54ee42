"""Link prediction without a GPU: the host restatement tests/topk_ref.py against a network of three nodes worked out
by hand, the arithmetic of TopDyadsResult (sort, tie-break, pooled, for_node, precision_at_k) on hand-made candidates
handed over in shuffled order, the facade's argument checks (before the library is loaded), the C-ABI declaration and
its binding, and the code objects of the two new sample-loop kernels (no scratch memory and no spilled register in any
instantiation)."""
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

import topk_ref  # noqa: E402


def _expit(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_reference_against_three_nodes_worked_out_by_hand():
    """Nodes at 0, 1 and 3 on a line, S = 2 samples with intercepts 1 and 3: eta of (0, 1) is 0 and 2, of (0, 2)
    -2 and 0, of (1, 2) -1 and 1, so pbar(0, 1) > pbar(1, 2) = 1/2 > pbar(0, 2); the one tie is (0, 1)"""
    Xs = np.zeros((2, 1, 3, 1))
    Xs[:, 0, :, 0] = [0.0, 1.0, 3.0]
    ic = np.array([[1.0, 0.0], [3.0, 0.0]])
    Y = np.zeros((1, 3, 3))
    Y[0, 0, 1] = Y[0, 1, 0] = 1
    p01 = (0.5 + _expit(2.0)) / 2
    p02 = (_expit(-2.0) + 0.5) / 2
    sd01 = abs(_expit(2.0) - 0.5) / math.sqrt(2.0)            # two values: |a - b| / sqrt(2)
    ref = topk_ref.reference(Y, Xs, ic, None, False, 'all', True)
    assert [tuple(a.tolist()) for a in ref['rank'][0]] == [(0, 1, 0), (1, 2, 2)]       # (0,1), (1,2), (0,2)
    for key in ('pw', 'pw_ld'):
        pw = ref[key][0]
        assert abs(float(pw[0, 1, 0]) - p01) <= 4 * np.spacing(p01)
        assert abs(float(pw[0, 2, 0]) - p02) <= 4 * np.spacing(p02)
        assert abs(float(pw[1, 2, 0]) - 0.5) <= 4 * np.spacing(0.5)
        assert abs(float(pw[0, 1, 1]) - sd01) <= 8 * np.spacing(sd01)
        assert not pw[1, 0].any() and not pw[0, 0].any()                                # undirected: i < j only
    assert ref['eligible_t'].tolist() == [3]
    # ascending
    up = topk_ref.reference(Y, Xs, ic, None, False, 'all', False)
    assert [tuple(a.tolist()) for a in up['rank'][0]] == [(0, 1, 0), (2, 2, 1)]        # (0,2), (1,2), (0,1)
    # eligibility: the tie, the non-ties, and a mask bit given as (2, 0) excludes the dyad (0, 2)
    mask = np.zeros((1, 3, 3), dtype=bool)
    mask[0, 2, 0] = True
    want = {('non_ties', None): [(1, 2), (0, 2)], ('ties', None): [(0, 1)],
            ('observed', None): [(0, 1), (1, 2), (0, 2)], ('missing', None): [],
            ('non_ties', 'm'): [(1, 2)], ('ties', 'm'): [(0, 1)],
            ('observed', 'm'): [(0, 1), (1, 2)], ('missing', 'm'): [(0, 2)], ('all', 'm'): [(0, 1), (1, 2), (0, 2)]}
    for (among, m), dyads in want.items():
        r = topk_ref.reference(Y, Xs, ic, None, False, among, True, mask if m else None)
        assert list(zip(*(a.tolist() for a in r['rank'][0]))) == dyads, (among, m)
        assert r['eligible_t'].tolist() == [len(dyads)]
    # the cut: all three values are far apart, so every k is decided; two equal values cut by (i, j) are decided
    # only when the group's neighbours are far away
    tol = topk_ref.tolerances(ref)[0]
    assert all(topk_ref.cut_is_decided(ref, 0, k, tol) for k in (1, 2, 3, 10))
    Xs2 = np.zeros((2, 1, 3, 1))
    Xs2[:, 0, :, 0] = [0.0, 1.0, 2.0]                      # (0, 1) and (1, 2) at the same distance
    eq = topk_ref.reference(Y, Xs2, ic, None, False, 'all', True)
    assert eq['pw'][0, 0, 1, 0] == eq['pw'][0, 1, 2, 0]
    assert [tuple(a.tolist()) for a in eq['rank'][0]] == [(0, 1, 0), (1, 2, 2)]
    assert topk_ref.cut_is_decided(eq, 0, 1, topk_ref.tolerances(eq)[0])
    Xs2[:, 0, 2, 0] = 2.0 + 4e-15                          # nearly the same distance: the cut is not decided
    near = topk_ref.reference(Y, Xs2, ic, None, False, 'all', True)
    assert near['pw'][0, 0, 1, 0] != near['pw'][0, 1, 2, 0]
    assert not topk_ref.cut_is_decided(near, 0, 1, topk_ref.tolerances(near)[0])


def test_result_sorts_breaks_ties_pools_and_scores():
    import dynetlsm_amd as da
    rng = np.random.RandomState(3)
    for largest in (True, False):
        # two time steps of candidates with repeated probabilities, in shuffled order
        steps, rows = [], []
        for t, n in enumerate((9, 6)):
            i = rng.randint(0, 7, n)
            j = (i + 1 + rng.randint(0, 3, n)) % 8
            keep = np.unique(np.stack([i, j], axis=1), axis=0, return_index=True)[1]
            i, j = i[keep], j[keep]
            proba = rng.choice([0.125, 0.25, 0.5, 0.75], i.size)
            sd = rng.rand(i.size)
            y = rng.randint(0, 2, i.size)
            perm = rng.permutation(i.size)
            steps.append((i[perm], j[perm], y[perm], proba[perm], sd[perm]))
            rows += [(t, int(a), int(b), float(p), float(s), int(c)) for a, b, p, s, c in zip(i, j, proba, sd, y)]
        k = 4
        res = da.TopDyadsResult(np.arange(5), 5, k, 'all', largest, True, 8, steps, [20, 20])
        sign = -1.0 if largest else 1.0
        want = []
        for t in (0, 1):
            want += sorted((r for r in rows if r[0] == t), key=lambda r: (sign * r[3], r[1], r[2]))[:k]
        got = list(zip(res.t.tolist(), res.i.tolist(), res.j.tolist(), res.proba.tolist(), res.sd.tolist(),
                       res.y.tolist()))
        assert got == want
        assert res.eligible_t.tolist() == [20, 20]
        for t in (0, 1):
            at = res.at(t)
            assert list(zip(*(a.tolist() for a in at))) == [r for r in want if r[0] == t]
        # pooled: the merge of the lists per time step by (probability, t, i, j)
        merged = sorted(want, key=lambda r: (sign * r[3], r[0], r[1], r[2]))
        for kk in (1, 3, 4):
            assert list(zip(*(a.tolist() for a in res.pooled(kk)))) == merged[:kk]
        assert list(zip(*(a.tolist() for a in res.pooled()))) == merged[:k]
        with pytest.raises(ValueError):
            res.pooled(k + 1)
        # the k first over all time steps are the same from the full lists: a subset of the lists per time step
        full = sorted(rows, key=lambda r: (sign * r[3], r[0], r[1], r[2]))[:k]
        assert merged[:k] == full
        node = 3
        assert list(zip(*(a.tolist() for a in res.for_node(node)))) == [r for r in want if node in (r[1], r[2])]
        with pytest.raises(ValueError):
            res.for_node(8)
        with pytest.raises(ValueError):
            res.at(2)
        Y_true = rng.randint(0, 2, (2, 8, 8))
        Y_true[0, 0, 1] = -1                                     # a missing entry is no tie
        hits = [Y_true[r[0], r[1], r[2]] == 1 for r in want]
        assert res.precision_at_k(Y_true) == sum(hits) / len(hits)
        with pytest.raises(ValueError):
            res.precision_at_k(Y_true[:1])
        text = res.summary()
        assert 'top dyads' in text and 'proba' in text and repr(res) == text
    # nothing eligible anywhere
    none = np.zeros(0)
    empty = da.TopDyadsResult(np.arange(2), 2, 3, 'missing', True, False, 4, [(none, none, none, none, none)], [0])
    assert empty.t.size == 0 and empty.at(0).i.size == 0 and np.isnan(empty.precision_at_k(np.zeros((1, 4, 4))))
    assert 'no eligible dyad' in empty.summary() and empty.pooled().t.size == 0


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
        da.top_dyads(Unfitted())
    for k in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='k must'):
            da.top_dyads(Fitted(), k=k)
    for among in ('edges', None, 0):
        with pytest.raises(ValueError, match='among'):
            da.top_dyads(Fitted(), among=among)
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.top_dyads(Fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='two samples'):
        da.top_dyads(Fitted(), n_samples=1)
    with pytest.raises(ValueError, match='missing'):
        da.top_dyads(Fitted(), among='missing')

    class WithNaN(Fitted):
        Xs_ = np.zeros((10, 2, 5, 2))
    WithNaN.Xs_[7, 1, 2, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        da.top_dyads(WithNaN())

    class WithInf(Fitted):
        intercepts_ = np.zeros((10, 1))
    WithInf.intercepts_[9, 0] = np.inf
    with pytest.raises(ValueError, match='finite'):
        da.top_dyads(WithInf())
    assert _lib._LIB is loaded                                     # none of this loaded the library


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build, dependencies
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_topk_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_topk_accumulate'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert len(args) == 15 and args[0].startswith('dlsm_chain') and args[-1].endswith('diag')
    assert args[7:11] == ['int among', 'int largest', 'int64_t k', 'int64_t max_candidates']
    res, argtypes = _lib.SIGNATURES['dlsm_topk_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[9] is ctypes.c_int64 and argtypes[10] is ctypes.c_int64
    assert hasattr(ctypes.CDLL(build()), 'dlsm_topk_accumulate')
    # the profile slots of the three phases, in the header and in the binding
    for name in ('TOPK_COUNT', 'TOPK_SCAN', 'TOPK_EMIT'):
        q = re.search(r'\bDLSM_K_%s\s*=\s*(\d+)' % name, src)
        assert q and int(q.group(1)) == getattr(_lib, 'K_' + name), name
    assert callable(da.top_dyads) and callable(da.Chain.topk_accumulate) and da.ranking.top_dyads is da.top_dyads
    for name in ('top_dyads', 'TopDyadsResult', 'ranking'):
        assert name in da.__all__
    assert da.Chain.TOPK_AMONG == topk_ref.AMONG                   # the order is the C-ABI's numbering
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dlsm_topk_accumulate(' in doc
    names = {os.path.basename(d) for d in dependencies()}
    assert {'kernels_topk.hpp', 'capi_topk.hpp'} <= names


def test_every_instantiation_of_the_sample_loop_kernels_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_topk_%s<%d,%s>' % (phase, d, m) for phase in ('count', 'emit') for d in range(1, 9)
             for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        assert md[name]['vgpr'] <= 512, (name, md[name])
    assert md['k_topk_threshold']['scratch_bytes'] == 0 and md['k_topk_threshold']['vgpr_spill'] == 0
    assert sorted(k for k in md if k.startswith('k_topk_')) == sorted(names + ['k_topk_threshold'])
