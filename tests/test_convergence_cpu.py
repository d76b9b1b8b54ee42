"""Per-dyad convergence diagnostics without a GPU: the host restatement (tests/convergence_ref.py) against
multichain.split_rhat and on the series whose values are defined, the bins of the histograms, the host
functions behind ConvergenceResult.scalars, the argument checks that come before any device call, the C-ABI
declaration and its binding, and the code object of the new kernels (no scratch memory, no spill)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import convergence_ref as cr  # noqa: E402

RHAT_EDGES = (1.01, 1.05, 1.1, 1.2, 1.5, 2.0)
ESS_EDGES = (10, 50, 100, 200, 400, 1000)


def _one_dyad(series, n_segments, seg_len, batch_len, rhat_edges=RHAT_EDGES, ess_edges=ESS_EDGES,
              dtype=np.float64):
    """the replica on two nodes at one place whose intercept is the series: eta_s = series[s] exactly"""
    series = np.asarray(series, dtype=np.float64)
    S = series.shape[0]
    Xs = np.zeros((S, 1, 2, 1))
    ic = np.stack([series, np.zeros(S)], axis=1)
    return cr.accumulate(Xs, ic, None, False, n_segments, seg_len, batch_len, rhat_edges, ess_edges, dtype)


@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('directed', [False, True])
def test_replica_rhat_is_split_rhat_of_the_eta_series(C, directed):
    from dynetlsm_amd.multichain import split_rhat
    rng = np.random.RandomState(10 * C + directed)
    n, T, N, D = 12, 2, 5, 2
    S = C * n
    # chains around different centres and a drifting intercept: rhat on both sides of 1
    Xs = rng.randn(S, T, N, D) + np.repeat(0.5 * rng.randn(C, 1, N, D), n, axis=0)
    ic = np.stack([rng.uniform(0.0, 1.0, S) + np.linspace(0, 1, S), rng.uniform(0.0, 1.0, S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    eta = cr.eta_series(Xs, ic, radii, directed)
    rhat, ess = cr.series_rhat_ess(eta, 2 * C, n // 2, 2)
    pairs = [(t, i, j) for t in range(T) for i in range(N) for j in range(N) if (i != j if directed else i < j)]
    assert len(pairs) >= 12
    for t, i, j in pairs[:6] + pairs[-6:]:
        want = split_rhat(eta[:, t, i, j].reshape(C, n))
        assert np.isfinite(want) and want > 0.5
        assert abs(rhat[t, i, j] - want) <= 1e-12 * want, (t, i, j, rhat[t, i, j], want)
        assert ess[t, i, j] > 0


def test_series_with_defined_values():
    S = 24
    # a constant series: (1, S)
    hr, he, nr, ne, pw = _one_dyad(np.full(S, 0.3), 2, 12, 3)
    assert pw[0, 0, 1, 0] == 1.0 and pw[0, 0, 1, 1] == S
    assert (nr == 1.0).all() and (ne == S).all()
    assert hr[0].tolist() == [1, 0, 0, 0, 0, 0, 0] and he[0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    # chains that are each constant but differ: rhat = +inf, in the last bin; ess finite
    hr, he, nr, ne, pw = _one_dyad(np.repeat([0.25, 0.75], 12), 4, 6, 2)
    assert pw[0, 0, 1, 0] == np.inf and np.isfinite(pw[0, 0, 1, 1]) and pw[0, 0, 1, 1] > 0
    assert hr[0, -1] == 1 and hr[0].sum() == 1 and (nr == np.inf).all()
    # a series of period b: every batch mean is the same, ess = +inf in the last bin; rhat finite
    for h, b in ((12, 3), (13, 3)):                          # (13: a tail that enters no batch)
        series = np.tile(np.tile([0.5, -1.0, 2.25], 5)[:h], 2)
        hr, he, nr, ne, pw = _one_dyad(series, 2, h, b)
        assert pw[0, 0, 1, 1] == np.inf and np.isfinite(pw[0, 0, 1, 0]) and pw[0, 0, 1, 0] > 0
        assert he[0, -1] == 1 and he[0].sum() == 1 and (ne == np.inf).all()
    # the lower triangle and the diagonal stay zero
    assert pw[0, 1, 0].tolist() == [0, 0] and pw[0, 0, 0].tolist() == [0, 0] and pw[0, 1, 1].tolist() == [0, 0]
    # nothing is NaN in extended precision either
    out = _one_dyad(np.repeat([0.25, 0.75], 12), 4, 6, 2, dtype=np.longdouble)
    assert out[4].dtype == np.longdouble and out[4][0, 0, 1, 0] == np.inf


def test_every_edge_is_the_lower_bound_of_its_bin():
    for edges in (RHAT_EDGES, ESS_EDGES, (3.0,)):
        e = np.asarray(edges, dtype=np.float64)
        assert cr.bins(e, e).tolist() == list(range(1, len(e) + 1))
        assert cr.bins(np.nextafter(e, -np.inf), e).tolist() == list(range(len(e)))
        assert cr.bins([0.0, np.inf], e).tolist() == [0, len(e)]
    assert cr.bins([0.0, 5.0, np.inf], ()).tolist() == [0, 0, 0]
    # through the replica: the constant series has rhat = 1 and ess = S exactly
    S = 24
    hr, he = _one_dyad(np.full(S, 0.3), 2, 12, 3, rhat_edges=(0.5, 1.0, 1.5), ess_edges=(12.0, 24.0, 48.0))[:2]
    assert hr[0].tolist() == [0, 0, 1, 0] and he[0].tolist() == [0, 0, 1, 0]
    hr, he = _one_dyad(np.full(S, 0.3), 2, 12, 3, rhat_edges=(np.nextafter(1.0, 2.0),),
                       ess_edges=(np.nextafter(24.0, 25.0),))[:2]
    assert hr[0].tolist() == [1, 0] and he[0].tolist() == [1, 0]


@pytest.mark.parametrize('C,n', [(1, 8), (2, 30), (3, 41)])
def test_host_scalar_functions_agree_with_the_replica_on_one_dyad(C, n):
    from dynetlsm_amd import convergence as cv
    from dynetlsm_amd.multichain import split_rhat
    rng = np.random.RandomState(C + n)
    chains = np.cumsum(rng.randn(C, n), axis=1) * 0.3 + rng.randn(C, 1)
    q = cv.split_segments(chains)
    h = n // 2
    b = int(np.floor(np.sqrt(h)))
    assert q.shape == (2 * C, h)
    np.testing.assert_array_equal(q[0], chains[0, :h])
    np.testing.assert_array_equal(q[1], chains[0, h:2 * h])
    pw = _one_dyad(q.ravel(), 2 * C, h, b)[4]
    rhat, ess = cv.series_rhat(q), cv.series_ess(q, b)
    assert abs(rhat - pw[0, 0, 1, 0]) <= 1e-12 * rhat, (rhat, pw[0, 0, 1, 0])
    assert abs(ess - pw[0, 0, 1, 1]) <= 1e-10 * ess, (ess, pw[0, 0, 1, 1])
    assert cv.series_ess(q) == ess
    assert abs(rhat - split_rhat(chains)) <= 1e-12 * rhat
    # the defined values
    const = np.full((2, 6), 0.5)
    assert cv.series_rhat(const) == 1.0 and cv.series_ess(const, 2) == 12.0
    apart = np.repeat([[0.0], [0.0], [1.0], [1.0]], 6, axis=1)
    assert cv.series_rhat(apart) == np.inf and np.isfinite(cv.series_ess(apart, 2))
    assert cv.series_ess(np.tile([0.5, -1.0, 2.25], (2, 4)), 3) == np.inf


class _Fitted(object):                         # the attributes the function reads, nothing else
    is_directed = False
    thin = None
    n_burn_ = 4

    def __init__(self, n_rows=10, N=5, seed=0):
        rng = np.random.RandomState(seed)
        self.Y_fit_ = np.zeros((2, N, N))
        self.Xs_ = rng.randn(n_rows, 2, N, 2)
        self.intercepts_ = rng.randn(n_rows, 1)
        self.logps_ = rng.randn(n_rows)


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib

    def boom():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    with pytest.raises(ValueError, match='not fit'):
        da.convergence_diagnostics(da.DynamicNetworkLSM())
    with pytest.raises(ValueError, match='not fit'):
        da.convergence_diagnostics([_Fitted(), da.DynamicNetworkLSM()])
    with pytest.raises(ValueError):
        da.convergence_diagnostics([])
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.convergence_diagnostics(_Fitted(), n_samples=bad)
    # fewer than 4 kept rows
    with pytest.raises(ValueError, match='at least 4'):
        da.convergence_diagnostics(_Fitted(n_rows=7))
    with pytest.raises(ValueError, match='at least 4'):
        da.convergence_diagnostics(_Fitted(), n_samples=3)
    # chains that do not match
    a = _Fitted()
    other_rows, other_shape, other_net, other_dir = _Fitted(n_rows=12), _Fitted(N=6), _Fitted(), _Fitted()
    other_net.Y_fit_ = a.Y_fit_.copy()
    other_net.Y_fit_[0, 1, 2] = other_net.Y_fit_[0, 2, 1] = 1
    other_dir.is_directed = True

    class Other(_Fitted):
        pass
    for b, what in ((other_rows, 'kept rows'), (other_shape, 'shape'), (other_net, 'different networks'),
                    (other_dir, 'directed'), (Other(), 'classes')):
        with pytest.raises(ValueError, match=what):
            da.convergence_diagnostics([a, b])
    # edges
    for kw in (dict(rhat_edges=(1.1, 1.05)), dict(ess_edges=(10, 10)), dict(ess_edges=(1.0, np.nan)),
               dict(rhat_edges=(1.0, np.inf)), dict(rhat_edges=tuple(1 + 0.1 * k for k in range(17)))):
        with pytest.raises(ValueError, match='edges'):
            da.convergence_diagnostics(a, **kw)
    # everything in order: the next step is the device
    with pytest.raises(AssertionError, match='the library was loaded'):
        da.convergence_diagnostics([a, _Fitted(seed=1)])
    with pytest.raises(AssertionError, match='the library was loaded'):
        da.convergence_diagnostics(a, n_samples=4)


def test_result_fields_and_summary():
    from dynetlsm_amd.convergence import ConvergenceResult
    rng = np.random.RandomState(3)
    S, T, N, D = 24, 2, 7, 2
    Xs = rng.randn(S, T, N, D)
    ic = rng.randn(S, 2)
    hr, he, nr, ne, pw = cr.accumulate(Xs, ic, None, False, 4, 6, 2, RHAT_EDGES, ESS_EDGES)
    res = ConvergenceResult(2, 6, 2, [np.arange(12), np.arange(12)], RHAT_EDGES, ESS_EDGES, hr, he, nr, ne, False,
                            pw, {'logps': (1.01, 20.0)})
    assert (res.n_chains, res.n_segments, res.seg_len, res.batch_len, res.n_samples) == (2, 4, 6, 2, 24)
    assert res.n_dyads == T * N * (N - 1) // 2 and (res.n_dyads_t == N * (N - 1) // 2).all()
    np.testing.assert_array_equal(res.rhat_hist, hr.sum(axis=0))
    np.testing.assert_array_equal(res.ess_hist_t, he)
    mask = cr.dyad_mask(N, False)
    assert res.max_rhat == pw[..., 0][:, mask].max() and res.min_ess == pw[..., 1][:, mask].min()
    np.testing.assert_array_equal(res.max_rhat_t, pw[..., 0][:, mask].max(axis=1))
    np.testing.assert_array_equal(res.min_ess_t, pw[..., 1][:, mask].min(axis=1))
    worst = res.worst_nodes(5)
    assert len(worst) == 5 and worst[0][2] == res.max_rhat
    assert all(w[2] == nr[w[0], w[1]] and w[3] == ne[w[0], w[1]] for w in worst)
    assert [w[2] for w in worst] == sorted((w[2] for w in worst), reverse=True)
    assert len(res.worst_nodes(1000)) == T * N
    np.testing.assert_array_equal(res.pointwise_rhat, pw[..., 0])
    np.testing.assert_array_equal(res.pointwise_ess, pw[..., 1])
    text = res.summary()
    assert 'rhat >= 2' in text and 'ess < 10' in text and 'logps' in text and repr(res) == text
    none = ConvergenceResult(1, 6, 2, np.arange(12), (), (), hr[:, :1], he[:, :1], nr, ne, True)
    assert none.pointwise_rhat is None and none.pointwise_ess is None and 'rhat all' in none.summary()


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    from dynetlsm_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_convergence_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_convergence_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 16 and args[0].startswith('dlsm_chain') and args[-1].endswith('pointwise')
    res, argtypes = _lib.SIGNATURES['dlsm_convergence_accumulate']
    assert len(argtypes) == len(args)
    import ctypes
    from dynetlsm_amd.build import build
    assert hasattr(ctypes.CDLL(build()), 'dlsm_convergence_accumulate')


def test_every_instantiation_of_the_kernel_is_free_of_scratch_memory_and_spills():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_conv_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        # a 256-thread workgroup must fit a SIMD's 512 registers per lane
        assert md[name]['vgpr'] <= 512, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_conv_')) == sorted(names)
