"""The handle's device memory (dynetlsm_amd/csrc/device_mem.hpp): buffers that grow on a live handle leave the results
those of a handle that was sized right at once, bit for bit, and a handle gives all of its memory back.  Through the
C-ABI."""
import numpy as np
import pytest
import torch      # (one HIP runtime per process: torch's first)

from oracle import hdp_loop_oracle as hlo

pytestmark = pytest.mark.gpu

T, N, D = 3, 130, 2         # two batches of the pipelined sweep, the second nearly empty


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    return dynetlsm_amd


def _hyper():
    return hlo.Hyper(gamma=1.3, alpha_init=0.9, alpha=1.1, kappa=3.5, mean_variance_prior=2.4, b=1.7, a=2.0,
                     lambda_prior=0.9, lambda_variance_prior=0.01, gamma_prior_shape=1.0, gamma_prior_rate=0.1,
                     alpha_init_shape=1.0, alpha_init_rate=1.0, alpha_kappa_shape=5, alpha_kappa_rate=0.1,
                     a0=36.0, b0=9.3, c0=16.0, d0=9.4)


def _mixture(K, seed):
    rng = np.random.RandomState(seed)
    return dict(mu=rng.randn(K, D), sigma=rng.uniform(0.3, 0.9, K), z=rng.randint(0, K, size=(T, N)).astype(np.int64),
                beta=rng.dirichlet(np.ones(K)), w=rng.dirichlet(np.ones(K), size=(T, K)))


def _snapshot(eng, c, directed):
    """what the next stage starts from: positions, intercepts, radii and the positions' samplers"""
    s = dict(X=c.get_positions(), b=c.get_intercepts(), grid=c.get_samplers(eng.SamplerGrid(T, N, 0.1, tune=None)))
    if directed:
        s['radii'] = c.get_radii()
    return s


def _restore(c, s):
    c.set_positions(s['X']); c.set_intercepts(s['b']); c.set_samplers(s['grid'])
    if 'radii' in s:
        c.set_radii(s['radii'])


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k          # bitwise: NaN slots (the undirected trace's) included


def test_regrown_buffers_leave_the_hdp_loop_bitwise_unchanged(eng):
    """One handle, undirected: two pipelined sweeps, the LSM trace allocated for 4 rows and again for 9, the HDP-LPCM
    loop with 3 components and again with 6 (the label buffers, mu / sigma and the loop's workspace grow) - against a
    fresh handle that only ever saw the last stage."""
    rng = np.random.RandomState(5)
    X0 = rng.randn(T, N, D)
    Y = np.triu((rng.rand(T, N, N) < 0.15).astype(np.float64), 1)
    Y = Y + Y.transpose(0, 2, 1)
    m3, m6 = _mixture(3, 11), _mixture(6, 12)

    def stage(c, m, first):
        c.set_prior_mixture(m['mu'], m['sigma'], 0.8, m['z'])
        c.hdp_configure(_hyper(), m['beta'], m['w'], 0.5, 2.0, sweep_algo=4)
        c.hdp_trace_alloc(9)
        c.hdp_run(first, 2)
        c.synchronize()
        out = c.hdp_trace_read(first, 2)
        out.update(X=c.get_positions(), b=c.get_intercepts(), step=c.get_samplers(eng.SamplerGrid(T, N)).step_size)
        return out

    with eng.Chain(T, N, D, 'undirected', seed=41, chain_id=3) as c:
        c.upload_network(Y); c.set_positions(X0); c.set_intercepts([0.4])
        c.set_samplers(eng.SamplerGrid(T, N, 0.1, tune=None)); c.set_prior_random_walk(2.0, 0.1)
        c.sweep_positions(1, algo=4); c.sweep_positions(2, algo=4)
        c.trace_alloc(4); c.trace_alloc(9)
        stage(c, m3, 1)
        before = _snapshot(eng, c, False)
        got = stage(c, m6, 3)
    with eng.Chain(T, N, D, 'undirected', seed=41, chain_id=3) as c:
        c.upload_network(Y); _restore(c, before)
        want = stage(c, m6, 3)
    assert not np.array_equal(got['X'], before['X'])        # the last stage moved something
    _assert_same(got, want)


def test_regrown_control_buffers_leave_the_case_control_loop_bitwise_unchanged(eng):
    """One handle, case-control: the LSM loop with 2 controls per node and direction, then with 5 (the control lists,
    the term rows and the walking order grow, the rows' width and the entries per node change) - against a fresh
    handle that only ever saw 5."""
    from dynetlsm_amd.case_control import build_edge_lists
    rng = np.random.RandomState(6)
    X0 = 0.02 * rng.randn(T, N, D)
    radii = rng.dirichlet(np.ones(N) * 8.0)
    Y = (rng.rand(T, N, N) < 0.1).astype(np.float64)
    for t in range(T):
        np.fill_diagonal(Y[t], 0.0)
    deg, ie, oe = build_edge_lists(Y)

    def stage(c, n_control, first):
        c.resample_controls(first, n_control)
        c.lsm_configure([0.7, 0.5], 2.0, sweep_algo=4, step_size_radii=20000.)
        c.trace_alloc(9)
        c.lsm_run(first, 2)
        c.synchronize()
        Xs, ics, lps = c.trace_read(first, 2)
        return dict(Xs=Xs, ics=ics, lps=lps, radii=c.trace_read_radii(first, 2), X=c.get_positions(),
                    b=c.get_intercepts(), step=c.get_samplers(eng.SamplerGrid(T, N)).step_size)

    def start(c, s):
        c.upload_edges(ie, oe, deg); _restore(c, s); c.set_prior_random_walk(1e-3, 1e-4)

    first_state = dict(X=X0, b=np.array([0.8, 0.4]), radii=radii, grid=eng.SamplerGrid(T, N, 0.004, tune=None))
    with eng.Chain(T, N, D, 'case_control', seed=43, chain_id=4) as c:
        start(c, first_state)
        c.resample_controls(0, 2)
        c.sweep_positions(1, algo=4); c.sweep_positions(2, algo=4)
        c.trace_alloc(4)
        stage(c, 2, 1)
        before = _snapshot(eng, c, True)
        got = stage(c, 5, 3)
    with eng.Chain(T, N, D, 'case_control', seed=43, chain_id=4) as c:
        start(c, before)
        want = stage(c, 5, 3)
    assert not np.array_equal(got['X'], before['X'])
    _assert_same(got, want)


def test_handles_give_their_memory_back(eng):
    """12 cycles of create, configure, a 256 MB position trace, one iteration, destroy - and one whose run is refused
    at the argument check: the device's free memory after cycle 12 is within one trace of that after cycle 2 (a
    trace leaked per cycle would cost ten)."""
    Tl, Nl, rows = 4, 1024, 4096
    assert Tl * Nl * D * rows * 8 == 256 << 20
    rng = np.random.RandomState(7)
    X0 = rng.randn(Tl, Nl, D)
    Y = np.triu((rng.rand(Tl, Nl, Nl) < 0.02).astype(np.float64), 1)
    Y = Y + Y.transpose(0, 2, 1)
    free = {}
    for cycle in [1, 2, 3, 4, 5, 6, 'refused', 7, 8, 9, 10, 11, 12]:
        with eng.Chain(Tl, Nl, D, 'undirected', seed=9, chain_id=1) as c:
            c.upload_network(Y); c.set_positions(X0); c.set_intercepts([0.3])
            c.set_samplers(eng.SamplerGrid(Tl, Nl, 0.1, tune=None)); c.set_prior_random_walk(2.0, 0.1)
            c.lsm_configure(0.0, 2.0)
            c.trace_alloc(rows)
            if cycle == 'refused':
                with pytest.raises(eng.EngineError) as err:
                    c.lsm_run(1, 1, procrustes_ref=rows)
                assert err.value.code == -1         # DLSM_E_ARG
            else:
                c.lsm_run(1, 1)
                c.synchronize()
        free[cycle] = torch.cuda.mem_get_info()[0]
    print('free MB after cycle 2 / refused / 12:', free[2] >> 20, free['refused'] >> 20, free[12] >> 20)
    assert abs(free[12] - free[2]) <= 256 << 20
