"""Per-node link prediction without a GPU: the host restatement tests/partners_ref.py against three nodes worked out by
hand, the arithmetic of TopPartnersResult on hand-made arrays with padding, the facade's argument checks (before the
library is loaded), the C-ABI declaration, its binding and its profile slot, and the code objects of k_partners_select
(no scratch memory and no spilled register in any instantiation)."""
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

import partners_ref  # noqa: E402


def _expit(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_reference_against_three_nodes_worked_out_by_hand():
    """Nodes at 0, 1 and 3 on a line, S = 2 samples with intercepts 1 and 3: eta of {0, 1} is 0 and 2, of {0, 2}
    -2 and 0, of {1, 2} -1 and 1, so pbar{0, 1} > pbar{1, 2} = 1/2 > pbar{0, 2}; the one tie is {0, 1}.  Node 0
    prefers 1 to 2, node 1 prefers 0 to 2, node 2 prefers 1 to 0."""
    Xs = np.zeros((2, 1, 3, 1))
    Xs[:, 0, :, 0] = [0.0, 1.0, 3.0]
    ic = np.array([[1.0, 0.0], [3.0, 0.0]])
    Y = np.zeros((1, 3, 3))
    Y[0, 0, 1] = 1                                            # the upper triangle is what an undirected model reads
    p01 = (0.5 + _expit(2.0)) / 2
    p02 = (_expit(-2.0) + 0.5) / 2
    sd01 = abs(_expit(2.0) - 0.5) / math.sqrt(2.0)
    ref = partners_ref.reference(Y, Xs, ic, None, False, 'all', True)
    assert [r.tolist() for r in ref['rank'][0]] == [[1, 2], [0, 2], [1, 0]]
    assert ref['eligible_n'].tolist() == [[2, 2, 2]]
    for key in ('pw', 'pw_ld'):
        pw = ref[key][0]
        for i, j, want in ((0, 1, p01), (0, 2, p02), (1, 2, 0.5)):
            assert abs(float(pw[i, j, 0]) - want) <= 4 * np.spacing(want)
            assert (pw[i, j] == pw[j, i]).all() and pw[j, i, 1] > 0        # symmetrised
        assert abs(float(pw[1, 0, 1]) - sd01) <= 8 * np.spacing(sd01)
        assert not pw[0, 0].any() and not pw[2, 2].any()
    assert ref['Y'][0].tolist() == [[False, True, False], [True, False, False], [False, False, False]]
    up = partners_ref.reference(Y, Xs, ic, None, False, 'all', False)
    assert [r.tolist() for r in up['rank'][0]] == [[2, 1], [2, 0], [0, 1]]
    # eligibility: a mask bit given as (2, 0) excludes the dyad {0, 2} from both of its rows
    mask = np.zeros((1, 3, 3), dtype=bool)
    mask[0, 2, 0] = True
    want = {('non_ties', None): [[2], [2], [1, 0]], ('ties', None): [[1], [0], []],
            ('observed', None): [[1, 2], [0, 2], [1, 0]], ('missing', None): [[], [], []],
            ('non_ties', 'm'): [[], [2], [1]], ('ties', 'm'): [[1], [0], []],
            ('observed', 'm'): [[1], [0, 2], [1]], ('missing', 'm'): [[2], [], [0]],
            ('all', 'm'): [[1, 2], [0, 2], [1, 0]]}
    for (among, m), rows in want.items():
        r = partners_ref.reference(Y, Xs, ic, None, False, among, True, mask if m else None)
        assert [x.tolist() for x in r['rank'][0]] == rows, (among, m)
        assert r['eligible_n'].tolist() == [[len(x) for x in rows]]
    # an undirected model does not read the lower triangle of the network
    Ylow = Y.copy()
    Ylow[0, 2, 1] = 1
    r = partners_ref.reference(Ylow, Xs, ic, None, False, 'ties', True)
    assert [x.tolist() for x in r['rank'][0]] == [[1], [0], []]
    # directed: the rows read their own orientation.  Radii 1: eta(i -> j) = (b_in + b_out)(1 - d)
    rad = np.ones((2, 3))
    Yd = np.zeros((1, 3, 3))
    Yd[0, 1, 0] = 1
    md = np.zeros((1, 3, 3), dtype=bool)
    md[0, 0, 2] = True
    d = partners_ref.reference(Yd, Xs, ic, rad, True, 'non_ties', True, md)
    assert [x.tolist() for x in d['rank'][0]] == [[1], [2], [1, 0]]
    assert d['pw'][0, 0, 1, 0] > d['pw'][0, 1, 2, 0] > d['pw'][0, 0, 2, 0]
    # the cut of a row: far apart values are decided; two equal values cut by j only with far neighbours
    tol = partners_ref.tolerances(ref)[0]
    assert all(partners_ref.row_cut_is_decided(ref, 0, i, k, tol) for i in range(3) for k in (1, 2, 5))
    Xs2 = np.zeros((2, 1, 3, 1))
    Xs2[:, 0, :, 0] = [0.0, 1.0, 2.0]                      # node 1 is as far from 0 as from 2
    eq = partners_ref.reference(Y, Xs2, ic, None, False, 'all', True)
    assert eq['pw'][0, 1, 0, 0] == eq['pw'][0, 1, 2, 0] and eq['rank'][0][1].tolist() == [0, 2]
    assert partners_ref.row_cut_is_decided(eq, 0, 1, 1, partners_ref.tolerances(eq)[0])
    Xs2[:, 0, 2, 0] = 2.0 + 4e-15
    near = partners_ref.reference(Y, Xs2, ic, None, False, 'all', True)
    assert near['pw'][0, 1, 0, 0] != near['pw'][0, 1, 2, 0]
    assert not partners_ref.row_cut_is_decided(near, 0, 1, 1, partners_ref.tolerances(near)[0])
    assert partners_ref.row_cut_is_decided(near, 0, 0, 1, partners_ref.tolerances(near)[0])


def _hand_made(direction='out', largest=True):
    """T = 2, N = 4, k = 3: node 0 has three partners at t = 0 and one at t = 1, node 1 two and none, node 2 was not
    asked for, node 3 has one and two"""
    import dynetlsm_amd as da
    nan = np.nan
    partner = np.array([[[1, 3, 2], [0, 2, -1], [-1, -1, -1], [0, -1, -1]],
                        [[2, -1, -1], [-1, -1, -1], [-1, -1, -1], [1, 2, -1]]])
    proba = np.array([[[.9, .5, .25], [.9, .125, nan], [nan] * 3, [.5, nan, nan]],
                      [[.75, nan, nan], [nan] * 3, [nan] * 3, [.625, .5, nan]]])
    if not largest:
        partner, proba = partner.copy(), proba.copy()
        partner[0, 0], proba[0, 0] = [2, 3, 1], [.25, .5, .9]
    sd = proba / 8
    y = np.where(partner >= 0, (partner % 2 == 0).astype(np.int64), -1)
    eligible = np.array([[3, 2, -1, 1], [1, 0, -1, 2]])
    return da.TopPartnersResult(np.arange(4, 9), 5, 3, 'all', largest, direction, True, partner, proba, sd, y,
                                eligible)


def test_result_lists_entries_without_padding_and_scores_them():
    import dynetlsm_amd as da
    res = _hand_made()
    assert res.n_time_steps == 2 and res.n_nodes == 4 and res.k == 3 and res.nodes.tolist() == [0, 1, 3]
    assert res.n_samples == 5 and res.sample_ids.tolist() == [4, 5, 6, 7, 8] and res.is_directed
    d = res.as_dyads()
    assert isinstance(d, da.ranking.DyadList)
    assert list(zip(d.t.tolist(), d.i.tolist(), d.j.tolist())) == [
        (0, 0, 1), (0, 0, 3), (0, 0, 2), (0, 1, 0), (0, 1, 2), (0, 3, 0), (1, 0, 2), (1, 3, 1), (1, 3, 2)]
    assert d.proba.tolist() == [.9, .5, .25, .9, .125, .5, .75, .625, .5]
    assert d.sd.tolist() == [p / 8 for p in d.proba.tolist()] and d.y.tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 1]
    n0 = res.for_node(0)
    assert list(zip(*(a.tolist() for a in n0)))[:2] == [(0, 0, 1, .9, .9 / 8, 0), (0, 0, 3, .5, .5 / 8, 0)]
    assert n0.t.tolist() == [0, 0, 0, 1] and (n0.i == 0).all()
    assert res.for_node(0, 1).j.tolist() == [2] and res.for_node(1, 1).j.size == 0
    assert res.for_node(2).j.size == 0 and res.for_node(3, t=1).j.tolist() == [1, 2]
    at1 = res.at(1)
    assert list(zip(at1.i.tolist(), at1.j.tolist())) == [(0, 2), (3, 1), (3, 2)] and (at1.t == 1).all()
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            res.for_node(bad)
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            res.at(bad)
        with pytest.raises(ValueError):
            res.for_node(0, bad)
    # against a full network, brute force
    rng = np.random.RandomState(5)
    Y_true = rng.randint(0, 2, (2, 4, 4))
    Y_true[0, 0, 1] = -1                                       # a missing entry is no tie
    hits = [Y_true[t, i, j] == 1 for t, i, j in zip(d.t, d.i, d.j)]
    assert res.precision_at_k(Y_true) == sum(hits) / len(hits)
    want = []
    for t in (0, 1):
        got_one = [any(Y_true[t, i, j] == 1 for j in res.partner[t, i] if j >= 0) for i in (0, 1, 3)]
        want.append(sum(got_one) / 3.0)
    assert res.hit_rate(Y_true).tolist() == want
    with pytest.raises(ValueError):
        res.precision_at_k(Y_true[:1])
    with pytest.raises(ValueError):
        res.hit_rate(Y_true[:, :3])
    # direction 'in': the entry (i, partner) is the tie partner -> i
    rin = _hand_made('in')
    hits = [Y_true[t, j, i] == 1 for t, i, j in zip(d.t, d.i, d.j)]
    assert rin.precision_at_k(Y_true) == sum(hits) / len(hits)
    want = [sum(any(Y_true[t, j, i] == 1 for j in rin.partner[t, i] if j >= 0) for i in (0, 1, 3)) / 3.0
            for t in (0, 1)]
    assert rin.hit_rate(Y_true).tolist() == want
    up = _hand_made(largest=False)
    assert up.for_node(0, 0).j.tolist() == [2, 3, 1] and not up.largest
    text = res.summary()
    assert 'top partners' in text and 'proba' in text and repr(res) == text and '3 of 4 nodes' in text
    # nothing returned
    none = da.TopPartnersResult(np.arange(2), 2, 2, 'missing', True, 'out', False, np.full((1, 3, 2), -1),
                                np.full((1, 3, 2), np.nan), np.full((1, 3, 2), np.nan), np.full((1, 3, 2), -1),
                                np.zeros((1, 3)))
    assert none.as_dyads().t.size == 0 and np.isnan(none.precision_at_k(np.zeros((1, 3, 3))))
    assert none.hit_rate(np.ones((1, 3, 3))).tolist() == [0.0] and 'no eligible partner' in none.summary()
    with pytest.raises(ValueError):
        da.TopPartnersResult(np.arange(2), 2, 3, 'all', True, 'out', False, np.full((1, 3, 2), -1),
                             np.full((1, 3, 2), np.nan), np.full((1, 3, 2), np.nan), np.full((1, 3, 2), -1),
                             np.zeros((1, 3)))


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

    class Directed(Fitted):
        is_directed = True
        intercepts_ = np.zeros((10, 2))
        radiis_ = np.ones((10, 5))

    loaded = _lib._LIB
    with pytest.raises(ValueError, match='not fit'):
        da.top_partners(Unfitted())
    for k in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='k must'):
            da.top_partners(Fitted(), k=k)
    with pytest.raises(ValueError, match='at most 64'):
        da.top_partners(Fitted(), k=65)
    with pytest.raises(ValueError, match='at most 64'):
        da.top_partners(Unfitted(), k=65)                         # before anything of the model is read
    for among in ('edges', None, 0):
        with pytest.raises(ValueError, match='among'):
            da.top_partners(Fitted(), among=among)
    for direction in ('both', None, 0, 'OUT'):
        with pytest.raises(ValueError, match='direction'):
            da.top_partners(Directed(), direction=direction)
    with pytest.raises(ValueError, match="direction='in'"):
        da.top_partners(Fitted(), direction='in')
    for nodes in ([], [5], [-1], [0.5], 3, [[0, 1]], [True, False]):
        with pytest.raises(ValueError, match='nodes'):
            da.top_partners(Fitted(), nodes=nodes)
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.top_partners(Fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='two samples'):
        da.top_partners(Fitted(), n_samples=1)
    with pytest.raises(ValueError, match='missing'):
        da.top_partners(Fitted(), among='missing')
    with pytest.raises(ValueError, match='missing'):
        da.top_partners(Directed(), among='missing', direction='in')

    class WithNaN(Fitted):
        Xs_ = np.zeros((10, 2, 5, 2))
    WithNaN.Xs_[7, 1, 2, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        da.top_partners(WithNaN())

    class WithInf(Directed):
        radiis_ = np.ones((10, 5))
    WithInf.radiis_[9, 0] = np.inf
    with pytest.raises(ValueError, match='finite'):
        da.top_partners(WithInf(), direction='in')
    assert _lib._LIB is loaded                                     # none of this loaded the library


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build, dependencies
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_partners_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_partners_accumulate'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert len(args) == 16 and args[0].startswith('dlsm_chain') and args[-1] == 'int32_t *eligible'
    assert args[6:12] == ['int S', 'int among', 'int largest', 'int k', 'const int32_t *row_blocks',
                          'int n_row_blocks']
    res, argtypes = _lib.SIGNATURES['dlsm_partners_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[9] is ctypes.c_int and argtypes[10] is _lib.c_i32_p and argtypes[13] is _lib.c_double_p
    assert hasattr(ctypes.CDLL(build()), 'dlsm_partners_accumulate')
    # dlsm_topk_accumulate keeps its parameters
    q = re.search(r'\bint\s+dlsm_topk_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert len(q.group(1).split(',')) == 15 == len(_lib.SIGNATURES['dlsm_topk_accumulate'][1])
    # the profile slot, in the header and in the binding
    slot = re.search(r'\bDLSM_K_PARTNERS\s*=\s*(\d+)', src)
    count = re.search(r'\bDLSM_K_COUNT\s*=\s*(\d+)', src)
    assert slot and int(slot.group(1)) == _lib.K_PARTNERS == 15 and int(count.group(1)) == 16
    assert callable(da.top_partners) and callable(da.Chain.partners_accumulate)
    assert da.ranking.top_partners is da.top_partners and da.ranking.TopPartnersResult is da.TopPartnersResult
    for name in ('top_partners', 'TopPartnersResult'):
        assert name in da.__all__ and name in da.ranking.__all__
    assert da.Chain.TOPK_AMONG == partners_ref.AMONG and da.Chain.PARTNERS_K_MAX == 64
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dlsm_partners_accumulate(' in doc
    names = {os.path.basename(d) for d in dependencies()}
    assert {'kernels_partners.hpp', 'capi_partners.hpp'} <= names


def test_every_instantiation_of_the_selection_kernel_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_partners_select<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        assert md[name]['vgpr'] <= 512, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_partners_')) == sorted(names)
