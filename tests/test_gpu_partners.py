"""Per-node link prediction on the device (csrc/kernels_partners.hpp, dynetlsm_amd/ranking.py) against the host
restatement tests/partners_ref.py.  Needs an MI355X: -m gpu.

Tolerance of proba and sd: the project's rule of proba_ref.tolerance, 16 eps + 4 ulp of the value, with eps the
reference's own error on that input: the larger of max |float64 - longdouble| and the largest change when every p_s is
moved by +-4 ulp with random signs.  Nothing enters it from the code under test.

The set of partners of every row is compared exactly and no row is left out.  Every case first asserts on its own
inputs (partners_ref.row_cut_is_decided) that the cut of every row is decided at that tolerance: the reference's k-th
and (k + 1)-th value differ by more than twice the tolerance, or they lie in a group of bit-equal values whose
neighbours on both sides are that far away.  A case that fails the condition fails with 'pick another seed'.  Inside a
list the device's own values must be sorted, ties by j, and the reference's values along it must not rise
(largest=False: fall) by more than twice the tolerance; the padding is exactly where eligible < k."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import partners_ref  # noqa: E402
from test_gpu_ic import _case  # noqa: E402
from test_gpu_topk import _coincident, _inputs, _model, _trace_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 7, 64)


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _is_padding(partner, proba, sd, y):
    return bool((partner == -1).all() and (y == -1).all() and np.isnan(proba).all() and np.isnan(sd).all())


def _check(got, ref, tols, k, largest, label, rows=None):
    """(partner, proba, sd, y, eligible) of Chain.partners_accumulate against the reference; ``rows``: the asked
    nodes, the others are padding with eligible = -1"""
    partner, proba, sd, y, eligible = got
    tol_p, tol_sd = tols
    T, N = ref['eligible_n'].shape
    assert partner.shape == proba.shape == sd.shape == y.shape == (T, N, k) and eligible.shape == (T, N), label
    assert partner.dtype == y.dtype == eligible.dtype == np.int64 and proba.dtype == sd.dtype == np.float64
    asked = np.ones(N, dtype=bool)
    if rows is not None:
        asked[:] = False
        asked[np.asarray(rows)] = True
    np.testing.assert_array_equal(eligible[:, asked], ref['eligible_n'][:, asked], err_msg=label)
    assert (eligible[:, ~asked] == -1).all(), label
    assert _is_padding(partner[:, ~asked], proba[:, ~asked], sd[:, ~asked], y[:, ~asked]), label
    worst = 0.0
    for t in range(T):
        for i in np.nonzero(asked)[0]:
            assert partners_ref.row_cut_is_decided(ref, t, i, k, tol_p), \
                '%s t=%d i=%d k=%d: pick another seed' % (label, t, i, k)
            want = ref['rank'][t][i]
            n = min(k, want.size)
            j = partner[t, i, :n]
            assert _is_padding(partner[t, i, n:], proba[t, i, n:], sd[t, i, n:], y[t, i, n:]), (label, t, i)
            assert sorted(j.tolist()) == sorted(want[:n].tolist()), (label, t, i)
            if not n:
                continue
            p, s = proba[t, i, :n], sd[t, i, :n]
            want_p, want_sd = ref['pw'][t, i, j, 0], ref['pw'][t, i, j, 1]
            tp, ts = tol_p[t, i, j], tol_sd[t, i, j]
            err_p, err_sd = np.abs(p - want_p), np.abs(s - want_sd)
            worst = max(worst, float((err_p / tp).max()), float((err_sd / ts).max()))
            assert (err_p <= tp).all(), (label, t, i, 'proba', float((err_p / tp).max()))
            assert (err_sd <= ts).all(), (label, t, i, 'sd', float((err_sd / ts).max()))
            np.testing.assert_array_equal(y[t, i, :n], ref['Y'][t, i, j].astype(np.int64), err_msg=label)
            # sorted by its own values, ties by j
            np.testing.assert_array_equal(np.lexsort((j, -p if largest else p)), np.arange(n), err_msg=label)
            # the reference's values along the list
            step = np.diff(want_p) * (1.0 if largest else -1.0)
            assert (step <= 2.0 * np.maximum(tp[1:], tp[:-1])).all(), (label, t, i, 'order')
    return worst


def _packed(da, inputs):
    Y, mask = inputs[0], inputs[4]
    return da.engine.pack_network(Y), (da.engine.pack_network(mask) if mask is not None else None)


def _run(da, chain, inputs, directed, k, among, largest, label, base=None, tols=None, rows=None):
    Y, Xs, ic, radii, mask = inputs
    bits, pm = _packed(da, inputs)
    ref = partners_ref.reference(Y, Xs, ic, radii, directed, among, largest, mask, base=base)
    got = chain.partners_accumulate(bits, Xs, ic, radii, k, among=among, largest=largest, mask=pm, rows=rows)
    worst = _check(got, ref, partners_ref.tolerances(ref) if tols is None else tols, k, largest, label, rows)
    return got, ref, worst


def _same_bytes(a, b, sel=None):
    for u, v in zip(a, b):
        if sel is not None:
            u, v = u[:, sel], v[:, sel]
        assert np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes()


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('N,T,D,S,directed', [(70, 2, 2, 20, False), (37, 3, 3, 25, True), (40, 2, 5, 12, True)])
def test_parity_on_two_column_tiles_and_ragged_edges(da, N, T, D, S, directed, masked):
    """every among, both orders, k = 1, inside a list and the whole list; the mask is asymmetric, so the undirected
    case reads either orientation of it"""
    inputs = _inputs(N, T, D, S, directed, masked)
    base = partners_ref.values(inputs[1], inputs[2], inputs[3], directed)
    tols = partners_ref.tolerances(base)
    worst = 0.0
    with da.Chain(T, N, D, _model(directed)) as c:
        for among in partners_ref.AMONG:
            for largest in (True, False):
                for k in KS:
                    label = 'N=%d dir=%d masked=%d %s largest=%d k=%d' % (N, directed, masked, among, largest, k)
                    if among == 'missing' and not masked:
                        with pytest.raises(ValueError, match='mask'):
                            c.partners_accumulate(da.engine.pack_network(inputs[0]), inputs[1], inputs[2], inputs[3],
                                                  k, among=among, largest=largest)
                        continue
                    worst = max(worst, _run(da, c, inputs, directed, k, among, largest, label, base, tols)[2])
    print('N=%d dir=%d masked=%d: max err/tol %.3f' % (N, directed, masked, worst))


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('D', range(1, 9))
def test_every_instantiation(da, D, directed):
    inputs = _inputs(20, 1, D, 12, directed, True)
    with da.Chain(1, 20, D, _model(directed)) as c:
        for among, largest in (('non_ties', True), ('ties', False), ('missing', True)):
            _run(da, c, inputs, directed, 5, among, largest, 'D=%d dir=%d %s' % (D, directed, among))


@pytest.mark.parametrize('directed', [False, True])
def test_k_beyond_the_eligible_partners_returns_all_of_them_ranked(da, directed):
    inputs = _inputs(12, 2, 2, 9, directed, True)
    with da.Chain(2, 12, 2, _model(directed)) as c:
        for among in partners_ref.AMONG:
            for largest in (True, False):
                (partner, proba, _, _, eligible), ref, _ = _run(da, c, inputs, directed, 64, among, largest,
                                                                'k=64 dir=%d %s' % (directed, among))
                assert (eligible <= 11).all()
                np.testing.assert_array_equal((partner >= 0).sum(axis=2), ref['eligible_n'])
                np.testing.assert_array_equal(np.isfinite(proba).sum(axis=2), ref['eligible_n'])
                assert (partner[:, :, 11:] == -1).all()


@pytest.mark.parametrize('directed', [False, True])
def test_a_row_without_an_eligible_partner_is_all_padding(da, directed):
    """The mask covers row and column r of time step 1: row (1, r) has nothing to choose from among the observed
    dyads.  The other time steps are byte-identical to the run without it; a row of time step 1 that did not list r
    keeps its list byte for byte (r was not among its k first, so its k first are the same) and counts r out."""
    N, T, r, k = 37, 3, 20, 7
    Y, Xs, ic, radii, mask = _inputs(N, T, 3, 25, directed, True)
    covered = mask.copy()
    covered[1, r, :] = True
    covered[1, :, r] = True
    plain = (Y, Xs, ic, radii, mask)
    inputs = (Y, Xs, ic, radii, covered)
    with da.Chain(T, N, 3, _model(directed)) as c:
        for among in ('non_ties', 'ties', 'observed'):
            got, _, _ = _run(da, c, inputs, directed, k, among, True, 'covered %s' % among)
            other, ref, _ = _run(da, c, plain, directed, k, among, True, 'plain %s' % among)
            assert got[4][1, r] == 0 and _is_padding(*(a[1, r] for a in got[:4]))
            for t in (0, 2):
                for a, b in zip(got, other):
                    assert a[t].tobytes() == b[t].tobytes()
            keeps = ~(other[0][1] == r).any(axis=1)
            keeps[r] = False
            assert keeps.sum() >= 5
            for a, b in zip(got[:4], other[:4]):
                assert a[1][keeps].tobytes() == b[1][keeps].tobytes()
            np.testing.assert_array_equal(got[4][1][keeps], (other[4][1] - ref['eligible'][1, :, r])[keeps])
        # every partner of r is missing
        got, ref, _ = _run(da, c, inputs, directed, k, 'missing', True, 'covered missing')
        assert got[4][1, r] == N - 1 and (got[0][1, r] >= 0).all()
    # a node without ties, ranked under 'ties'
    Y0 = Y.copy()
    Y0[0, r, :] = 0
    Y0[0, :, r] = 0
    with da.Chain(T, N, 3, _model(directed)) as c:
        got, _, _ = _run(da, c, (Y0, Xs, ic, radii, mask), directed, k, 'ties', False, 'no ties')
        other, ref, _ = _run(da, c, plain, directed, k, 'ties', False, 'plain ties')
        assert got[4][0, r] == 0 and _is_padding(*(a[0, r] for a in got[:4]))
        for t in (1, 2):
            for a, b in zip(got, other):
                assert a[t].tobytes() == b[t].tobytes()
        keeps = ~(other[0][0] == r).any(axis=1)
        keeps[r] = False
        for a, b in zip(got[:4], other[:4]):
            assert a[0][keeps].tobytes() == b[0][keeps].tobytes()


def _line(directed, N=130, S=6, seed=5):
    """D = 1, T = 1: the nodes on a line in index order with gaps uniform in [0.03, 0.07], the same in every sample
    up to a common shift per sample (directed: one radius per sample, and intercepts with a positive sum): in every
    sample the probability falls with |i - j|"""
    rng = np.random.RandomState(seed + directed)
    x = np.cumsum(rng.uniform(0.03, 0.07, N))
    Xs = (x[None, :] + rng.randn(S)[:, None])[:, None, :, None]
    ic = np.stack([rng.uniform(0.2, 1.5, S), rng.uniform(0.2, 1.5, S)], axis=1)
    radii = np.repeat(rng.uniform(0.5, 2.0, S)[:, None], N, axis=1) if directed else None
    Y = _case(rng, 1, 1, N, 1, directed)[0]
    return Y, np.ascontiguousarray(Xs), ic, radii, None


@pytest.mark.parametrize('directed', [False, True])
def test_the_list_is_carried_over_three_column_tiles_with_every_candidate_entering(da, directed):
    N = 130
    inputs = _line(directed)
    base = partners_ref.values(inputs[1], inputs[2], inputs[3], directed)
    tols = partners_ref.tolerances(base)
    p = base['pw'][0, :, :, 0]
    assert (np.diff(p[N - 1, :N - 1]) > 0).all(), 'row N-1 must rise with j: every candidate enters from the top'
    assert (np.diff(p[0, 1:]) < 0).all(), 'row 0 must fall with j: with largest=False every candidate enters'
    with da.Chain(1, N, 1, _model(directed)) as c:
        for among in ('all', 'non_ties'):
            for largest in (True, False):
                for k in KS:
                    got, ref, _ = _run(da, c, inputs, directed, k, among, largest,
                                       'line dir=%d %s largest=%d k=%d' % (directed, among, largest, k), base, tols)
                    if among == 'all':
                        if largest:                  # the last k columns, from the last one down
                            np.testing.assert_array_equal(got[0][0, N - 1], np.arange(N - 2, N - 2 - k, -1))
                        else:
                            np.testing.assert_array_equal(got[0][0, 0], np.arange(N - 1, N - 1 - k, -1))


@pytest.mark.parametrize('directed', [False, True])
def test_exact_ties_are_cut_by_j(da, directed):
    """nodes 3, 40 and 69 share positions (and radii) in every sample: every other row holds a group of three
    bit-equal values that spans both column tiles"""
    inputs = _coincident(directed)
    N, T = 70, 2
    base = partners_ref.values(inputs[1], inputs[2], inputs[3], directed)
    tols = partners_ref.tolerances(base)
    with da.Chain(T, N, 2, _model(directed)) as c:
        cuts = 0
        for largest in (True, False):
            ref = partners_ref.reference(inputs[0], inputs[1], inputs[2], inputs[3], directed, 'all', largest,
                                         base=base)
            # the k that cut through a group of bit-equal values in some row, and those rows
            cut_rows = {}
            for t in range(T):
                for i in range(N):
                    j = ref['rank'][t][i]
                    v = ref['pw'][t, i, j, 0]
                    for k in np.nonzero(v[:-1] == v[1:])[0] + 1:
                        if k <= 64:
                            cut_rows.setdefault(int(k), []).append((t, i))
            ks = sorted(cut_rows)
            assert len(ks) >= 6, 'the groups of coincident nodes are missing'
            for k in ks[:2] + ks[len(ks) // 2:len(ks) // 2 + 2] + ks[-2:]:
                got, _, _ = _run(da, c, inputs, directed, k, 'all', largest,
                                 'ties dir=%d largest=%d k=%d' % (directed, largest, k), base, tols)
                # the reference's stable sort keeps j ascending inside a group: the device returns that very prefix
                for t, i in cut_rows[k]:
                    np.testing.assert_array_equal(got[0][t, i], ref['rank'][t][i][:k])
                    cuts += 1
        assert cuts >= 12


@pytest.mark.parametrize('directed', [False, True])
def test_all_nodes_at_one_position_list_the_first_k_eligible_partners(da, directed):
    N, T = 70, 2
    Y, Xs, ic, radii, mask = _inputs(N, T, 2, 8, directed, True)
    Xs = np.broadcast_to(Xs[:, :, :1, :], Xs.shape).copy()
    inputs = (Y, Xs, ic, radii, mask)
    with da.Chain(T, N, 2, _model(directed)) as c:
        for among, largest, k in (('all', True, 7), ('non_ties', False, 64), ('observed', True, 1)):
            (partner, proba, _, _, _), ref, _ = _run(da, c, inputs, directed, k, among, largest,
                                                     'one position dir=%d %s' % (directed, among))
            assert len(np.unique(ref['pw'][..., 0][ref['exists']])) == 1
            for t in range(T):
                for i in range(N):
                    want = np.nonzero(ref['eligible'][t, i])[0][:k]
                    np.testing.assert_array_equal(partner[t, i, :want.size], want)
            assert len(np.unique(proba[np.isfinite(proba)])) == 1


def test_agrees_with_top_dyads_bit_for_bit(da):
    N, T, k = 40, 2, 64
    for directed in (False, True):
        Y, Xs, ic, radii, _ = _inputs(N, T, 2, 8, directed)
        bits = da.engine.pack_network(Y)
        dyads = N * (N - 1) // (1 if directed else 2)
        with da.Chain(T, N, 2, _model(directed)) as c:
            partner, proba, sd, y, eligible = c.partners_accumulate(bits, Xs, ic, radii, k, among='all')
            steps, _ = c.topk_accumulate(bits, Xs, ic, radii, dyads, among='all')
        assert (eligible == N - 1).all() and (partner[:, :, :N - 1] >= 0).all()
        for t in range(T):
            i, r = np.nonzero(partner[t] >= 0)
            j, p, s, yy = partner[t, i, r], proba[t, i, r], sd[t, i, r], y[t, i, r]
            if not directed:
                # each dyad in both of its rows, with the same bits
                a, b = np.minimum(i, j), np.maximum(i, j)
                order = np.lexsort((i, b, a))
                a, b, p, s, yy = a[order], b[order], p[order], s[order], yy[order]
                assert (a[0::2] == a[1::2]).all() and (b[0::2] == b[1::2]).all() and a.size == 2 * dyads
                for col in (p, s, yy):
                    assert col[0::2].tobytes() == col[1::2].tobytes()
                i, j, p, s, yy = a[0::2], b[0::2], p[0::2], s[0::2], yy[0::2]
            order = np.lexsort((j, i, -p))
            for got, want in zip((i, j, yy, p, s), steps[t]):
                assert got[order].tobytes() == want.tobytes()


def test_a_subset_of_rows_skips_row_blocks(da):
    import ctypes
    from dynetlsm_amd import _lib
    N, T, D, k = 70, 2, 2, 7                                   # row blocks of 32: 0..31, 32..63, 64..69
    rows = [66, 3, 5, 3]
    for directed in (False, True):
        inputs = _inputs(N, T, D, 20, directed, True)
        Y, Xs, ic, radii, mask = inputs
        bits, pm = _packed(da, inputs)
        with da.Chain(T, N, D, _model(directed)) as c:
            full, _, _ = _run(da, c, inputs, directed, k, 'non_ties', True, 'full dir=%d' % directed)
            part, _, _ = _run(da, c, inputs, directed, k, 'non_ties', True, 'rows dir=%d' % directed,
                              rows=np.array(rows))
            _same_bytes(part, full, sel=[3, 5, 66])
            # the raw call computes whole blocks and leaves the blocks that are not listed alone
            out = [np.zeros((T, N, k), dtype=np.int32), np.zeros((T, N, k, 2)), np.zeros((T, N, k), dtype=np.int32),
                   np.zeros((T, N), dtype=np.int32)]
            blocks = np.array([0, 2], dtype=np.int32)
            dp = ctypes.POINTER(ctypes.c_double)
            Xc, icc = np.ascontiguousarray(Xs), np.ascontiguousarray(ic)
            rc = c._L.dlsm_partners_accumulate(
                c._h, bits.ctypes.data_as(_lib.c_u32_p), pm.ctypes.data_as(_lib.c_u32_p), Xc.ctypes.data_as(dp),
                icc.ctypes.data_as(dp), radii.ctypes.data_as(dp) if directed else None, Xs.shape[0], 0, 1, k,
                blocks.ctypes.data_as(_lib.c_i32_p), 2, out[0].ctypes.data_as(_lib.c_i32_p),
                out[1].ctypes.data_as(dp), out[2].ctypes.data_as(_lib.c_i32_p), out[3].ctypes.data_as(_lib.c_i32_p))
            assert rc == 0
            listed = np.r_[0:32, 64:70]
            np.testing.assert_array_equal(out[3][:, listed], full[4][:, listed])
            np.testing.assert_array_equal(out[0][:, listed], full[0][:, listed])
            assert out[1][..., 0][:, listed].tobytes() == full[1][:, listed].tobytes()
            assert out[1][..., 1][:, listed].tobytes() == full[2][:, listed].tobytes()
            assert (out[3][:, 32:64] == -1).all() and (out[0][:, 32:64] == -1).all()
            assert (out[2][:, 32:64] == -1).all() and np.isnan(out[1][:, 32:64]).all()
        with da.Chain(T, N, D, _model(directed)) as c:
            for bad in ([], [70], [-1], [[1, 2]], [1.5]):
                with pytest.raises(ValueError, match='rows'):
                    c.partners_accumulate(bits, Xs, ic, radii, k, rows=bad)


class _Trace(object):
    """what the facade reads of a fitted directed model, around given trace rows"""

    def __init__(self, Y, Xs, ic, radii, mask):
        self.is_directed, self.n_burn_ = True, 0
        self.Y_fit_, self.Xs_, self.intercepts_, self.radiis_ = Y, Xs, ic, radii
        self.missing_index_ = np.argwhere(mask & ~np.eye(Y.shape[1], dtype=bool)[None])


def test_direction_in_ranks_the_senders_of_every_receiver(da):
    """against the reference on the transposed problem: Y and the mask transposed and the two intercepts swapped"""
    N, T, D, S = 37, 3, 3, 25
    Y, Xs, ic, radii, mask = _inputs(N, T, D, S, True, True)
    m = _Trace(Y, Xs, ic, radii, mask)
    Yt, mt = Y.transpose(0, 2, 1), (mask & ~np.eye(N, dtype=bool)[None]).transpose(0, 2, 1)
    base = partners_ref.values(Xs, ic[:, ::-1], radii, True)
    tols = partners_ref.tolerances(base)
    out = partners_ref.values(Xs, ic, radii, True)
    out_tol = partners_ref.tolerances(out)[0]
    for among, largest, k in (('non_ties', None, 7), ('ties', None, 1), ('missing', True, 64), ('all', False, 7)):
        res = da.top_partners(m, k=k, among=among, largest=largest, direction='in')
        assert res.direction == 'in' and res.is_directed and res.n_samples == S and res.largest == (
            among != 'ties' if largest is None else largest)
        ref = partners_ref.reference(Yt, Xs, ic[:, ::-1], radii, True, among, res.largest, mt, base=base)
        _check((res.partner, res.proba, res.sd, res.y, res.eligible), ref, tols, k, res.largest, 'in %s' % among)
        # the probability of partner -> i, as the reference of the problem as it stands has it
        d = res.as_dyads()
        assert (np.abs(d.proba - out['pw'][d.t, d.j, d.i, 0]) <= out_tol[d.t, d.j, d.i]).all()
        np.testing.assert_array_equal(d.y, (Y[d.t, d.j, d.i] != 0).astype(np.int64))
    outward = da.top_partners(m, k=7, direction='out')
    ref = partners_ref.reference(Y, Xs, ic, radii, True, 'non_ties', True, mask)
    _check((outward.partner, outward.proba, outward.sd, outward.y, outward.eligible), ref,
           partners_ref.tolerances(ref), 7, True, 'out')


def test_two_calls_on_one_chain_return_the_same_bits(da):
    for directed in (False, True):
        Y, Xs, ic, radii, mask = _inputs(130, 2, 5, 12, directed, True)
        bits, pm = da.engine.pack_network(Y), da.engine.pack_network(mask)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            a = c.partners_accumulate(bits, Xs, ic, radii, 64, mask=pm)
            b = c.partners_accumulate(bits, Xs, ic, radii, 64, mask=pm)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            f = c.partners_accumulate(bits, Xs, ic, radii, 64, mask=pm)
        _same_bytes(b, a)
        _same_bytes(f, a)
        assert (a[4] >= 64).any() and (a[0] >= 0).any()


def test_bad_arguments_are_rejected(da):
    import ctypes
    from dynetlsm_amd import _lib
    rng = np.random.RandomState(0)
    T, N, k_room = 2, 40, 64
    Y, Xs, ic, radii = _case(rng, 4, T, N, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(T, N, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.partners_accumulate(bits, Xs, ic, None, 3)
        with pytest.raises(ValueError):
            c.partners_accumulate(bits[:1], Xs, ic, radii, 3)
        with pytest.raises(ValueError, match='two samples'):
            c.partners_accumulate(bits, Xs[:1], ic[:1], radii[:1], 3)
        for k in (0, -2, 1.5, True, 65):
            with pytest.raises(ValueError, match='k must'):
                c.partners_accumulate(bits, Xs, ic, radii, k)
        with pytest.raises(ValueError, match='among'):
            c.partners_accumulate(bits, Xs, ic, radii, 3, among='edges')
        with pytest.raises(da.EngineError) as e:
            c.partners_accumulate(bits, Xs, ic, radii * 0, 3)
        assert e.value.code == -4
        # the library's own checks
        dp = ctypes.POINTER(ctypes.c_double)
        keep = [np.ascontiguousarray(Xs), np.ascontiguousarray(ic), np.ascontiguousarray(radii),
                np.zeros((T, N, k_room), dtype=np.int32), np.zeros((T, N, k_room, 2)),
                np.zeros((T, N, k_room), dtype=np.int32), np.zeros((T, N), dtype=np.int32)]

        def raw(S=4, among=0, largest=1, k=3, mask=None, radii=keep[2], blocks=None):
            b = None if blocks is None else np.asarray(blocks, dtype=np.int32)
            return c._L.dlsm_partners_accumulate(
                c._h, bits.ctypes.data_as(_lib.c_u32_p), mask, keep[0].ctypes.data_as(dp), keep[1].ctypes.data_as(dp),
                radii.ctypes.data_as(dp) if radii is not None else None, S, among, largest, k,
                None if b is None else b.ctypes.data_as(_lib.c_i32_p), 0 if b is None else b.size,
                keep[3].ctypes.data_as(_lib.c_i32_p), keep[4].ctypes.data_as(dp),
                keep[5].ctypes.data_as(_lib.c_i32_p), keep[6].ctypes.data_as(_lib.c_i32_p))

        assert raw() == 0 and (keep[6] >= 0).all()
        assert raw(S=1) == -1 and raw(among=5) == -1 and raw(among=-1) == -1 and raw(largest=2) == -1
        assert raw(k=0) == -1 and raw(k=65) == -1 and raw(among=3) == -1 and raw(radii=None) == -1
        assert raw(blocks=[1, 0]) == -1 and raw(blocks=[0, 0]) == -1            # N = 40: the blocks are 0 and 1
        assert raw(blocks=[2]) == -1 and raw(blocks=[-1]) == -1 and raw(blocks=[0, 1, 2]) == -1
        assert 'row_blocks' in c._L.dlsm_last_error(c._h).decode()
        assert raw(among=3, mask=bits.ctypes.data_as(_lib.c_u32_p)) == 0
        assert raw(k=64, blocks=[1]) == 0 and (keep[6][:, :32] == -1).all() and (keep[6][:, 32:] >= 0).all()
        good = c.partners_accumulate(bits, Xs, ic, radii, 3)
        assert (good[4] >= 0).all() and (good[0] >= 0).any()


def _brute_force_scores(res, Y_true):
    hits, rate = [], []
    for t in range(res.n_time_steps):
        found = 0
        for i in res.nodes:
            row = [Y_true[t, i, j] == 1 for j in res.partner[t, i] if j >= 0]
            hits += row
            found += any(row)
        rate.append(found / float(res.nodes.size))
    return sum(hits) / float(len(hits)), rate


@pytest.mark.parametrize('directed', [False, True])
def test_facade_on_a_short_lsm_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N, k = 3, 30, 5
    Ynet = synthetic_lsm_network(T=T, N=N, density=0.2, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Ynet)
    res = da.top_partners(m, k=k)
    assert res.among == 'non_ties' and res.largest and res.direction == 'out' and res.k == k
    assert res.n_samples == m.Xs_.shape[0] - m.n_burn_ and res.n_nodes == N and res.is_directed == directed
    assert res.nodes.tolist() == list(range(N))
    Y, Xs, ic, radii = _trace_inputs(m, res.sample_ids)
    ref = partners_ref.reference(Y, Xs, ic, radii, directed, 'non_ties', True)
    tols = partners_ref.tolerances(ref)
    _check((res.partner, res.proba, res.sd, res.y, res.eligible), ref, tols, k, True, 'facade dir=%d' % directed)
    # the same rows through the chain
    with da.Chain(T, N, Xs.shape[3], _model(directed)) as c:
        got = c.partners_accumulate(da.engine.pack_network(Y), Xs, ic, radii, k)
    _same_bytes((res.partner, res.proba, res.sd, res.y, res.eligible), got)
    assert (res.y[res.partner >= 0] == 0).all()
    # a few nodes
    some = da.top_partners(m, k=k, nodes=[0, 7, 29])
    assert some.nodes.tolist() == [0, 7, 29]
    _check((some.partner, some.proba, some.sd, some.y, some.eligible), ref, tols, k, True, 'nodes', rows=[0, 7, 29])
    _same_bytes((some.partner, some.proba, some.sd, some.y, some.eligible),
                (res.partner, res.proba, res.sd, res.y, res.eligible), sel=[0, 7, 29])
    # for_node and at
    n7 = res.for_node(7)
    assert (n7.i == 7).all() and n7.t.tolist() == np.repeat(np.arange(T), k).tolist()
    np.testing.assert_array_equal(n7.j, res.partner[:, 7].ravel())
    assert res.for_node(7, 1).proba.tobytes() == res.proba[1, 7].tobytes()
    at2 = res.at(2)
    assert (at2.t == 2).all() and at2.i.tolist() == np.repeat(np.arange(N), k).tolist()
    np.testing.assert_array_equal(at2.j, res.partner[2].ravel())
    assert some.as_dyads().t.size == 3 * T * k and some.for_node(3).t.size == 0
    # implausible ties: the default order is ascending
    ties = da.top_partners(m, k=3, among='ties', n_samples=30)
    assert not ties.largest and ties.n_samples == 30 and (ties.y[ties.partner >= 0] == 1).all()
    Yt, Xt, it, rt = _trace_inputs(m, ties.sample_ids)
    tref = partners_ref.reference(Yt, Xt, it, rt, directed, 'ties', False)
    _check((ties.partner, ties.proba, ties.sd, ties.y, ties.eligible), tref, partners_ref.tolerances(tref), 3, False,
           'facade ties dir=%d' % directed)
    # precision and hit rate against brute force
    assert res.precision_at_k(Ynet) == 0.0 and ties.precision_at_k(Ynet) == 1.0
    other = synthetic_lsm_network(T=T, N=N, density=0.3, seed=9, directed=directed)['Y']
    for r in (res, some):
        precision, rate = _brute_force_scores(r, other)
        assert r.precision_at_k(other) == precision and r.hit_rate(other).tolist() == rate
    assert 'top partners' in res.summary()
    with pytest.raises(ValueError, match='missing'):
        da.top_partners(m, among='missing')


def test_facade_ranks_the_held_out_dyads_of_a_sample_missing_fit(da):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N, k = 3, 30, 5
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=3)['Y']
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=False)
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, random_state=4, sample_missing=True).fit(Yt)
    res = da.top_partners(m, k=k, among='missing', n_samples=40)
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    held |= held.transpose(0, 2, 1)
    d = res.as_dyads()
    assert d.t.size and held[d.t, d.i, d.j].all()
    np.testing.assert_array_equal(res.eligible, held.sum(axis=2))
    Yf, Xs, ic, radii = _trace_inputs(m, res.sample_ids)
    ref = partners_ref.reference(Yf, Xs, ic, radii, False, 'missing', True, held)
    _check((res.partner, res.proba, res.sd, res.y, res.eligible), ref, partners_ref.tolerances(ref), k, True,
           'held out')
    precision, rate = _brute_force_scores(res, Y)
    assert res.precision_at_k(Y) == precision and res.hit_rate(Y).tolist() == rate
    observed = da.top_partners(m, k=k, among='observed', n_samples=40)
    o = observed.as_dyads()
    assert not held[o.t, o.i, o.j].any()
