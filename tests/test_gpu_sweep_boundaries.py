"""The pipelined sweep's boundary switches change no bit of any result: write-through hand-off stores
(DLSM_PIPE_WT: H rows, item records and the resolvers' results leave the launch through sc1 stores) and the
full-width head launch (DLSM_PIPE_HEAD_SPREAD: 8 nodes per evaluator workgroup where the launch has no resolver
and few items).  Each is a parent-equivalent path inside one library: the device-resident loop is run from the
same state and seed with both on, with each off in turn and with both off, and everything it leaves is compared
byte for byte."""
import numpy as np
import pytest
import torch      # noqa: F401  (one HIP runtime per process: torch's first; _head_nodes asks it for the CU count)

pytestmark = pytest.mark.gpu

SWITCHES = ('DLSM_PIPE_WT', 'DLSM_PIPE_HEAD_SPREAD')
# both on (the reference of every comparison), each off in turn, both off
SETTINGS = [(1, 1), (0, 1), (1, 0), (0, 0)]


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    from dynetlsm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, 'no HIP device: the engine has no CPU path'
    return dynetlsm_amd


def _head_nodes(T, N, D, spread=True):
    """nodes per evaluator workgroup of the head launch on this device: the host's rule (pipe_plan.hpp:
    pipe_eval_workgroups, pipe_parts, pipe_lds_eval_bytes, pipe_launch_qshift at l = -1) restated"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ne_wg = max(n_cu // 2, n_cu - T)
    parts = min(max(int(ne_wg * 16 / (T * 128.0) + 0.5), 1), 8)
    if parts > 1 and parts * T * 128 > ne_wg * 16:
        parts -= 1
    ntrip = (N + 63) // 64
    lds_bytes = (2048 + ((ntrip + parts - 1) // parts + 4 + 4) * 64 * D) * 8
    lds_eval = lds_bytes <= 128 * 129 * 8 and parts * T * 128 <= ne_wg * 16
    wgs8 = parts * ((T + 1) // 2) * 16          # the head evaluates batch 0 of the even slices
    return 8 if spread and lds_eval and wgs8 <= ne_wg else 16


def _net(seed, T, N, D):
    rng = np.random.RandomState(seed)
    X = rng.randn(T, N, D) * 0.05
    Y = np.triu((rng.rand(T, N, N) < 0.2).astype(np.float64), 1)
    return X, Y + Y.transpose(0, 2, 1)


def _set(monkeypatch, setting):
    for name, v in zip(SWITCHES, setting):
        monkeypatch.setenv(name, str(v))


def _lsm_three_iterations(eng, X, Y, tune, monkeypatch, setting, chain_id=1):
    """three iterations of lsm_run under `setting`: (trace, samplers, final positions, intercept's sampler), and
    the nodes per workgroup of the last head launch"""
    _set(monkeypatch, setting)
    T, N, D = X.shape
    gg = eng.SamplerGrid(T, N, 0.1, tune=tune, tune_interval=2)
    with eng.Chain(T, N, D, 'undirected', seed=23, chain_id=chain_id) as c:
        c.upload_network(Y); c.set_positions(X); c.set_intercepts([0.2])
        c.set_prior_random_walk(2.0, 0.1); c.set_samplers(gg)
        c.lsm_configure([0.2], 2.0, step_size_intercept=0.1, tune=tune, tune_interval=2,
                        n_iter_procrustes=10 ** 6, sweep_algo=4)
        c.trace_alloc(4)
        c.lsm_run(1, 3)
        Xs, ics, lps = c.trace_read(0, 4)
        g = c.get_samplers(gg)
        cfg = c.lsm_get_config()
        out = (Xs, ics, lps, g.step_size.copy(), g.n_accepted.copy(), g.n_steps.copy(), g.steps_until_tune.copy(),
               c.get_positions().copy(), np.array([cfg.i_step_size[0]]), np.array([cfg.i_n_accepted[0]]))
        return out, c.pipe_head_nodes()


def _same_bytes(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i)
        assert a.tobytes() == b.tobytes(), '%s: array %d differs' % (what, i)


# T=10 N=520 d=2: the head's 1920 items spread over 240 workgroups, the last batch has 8 nodes (tuning under way);
# T=4 N=640 d=3: exact batches, 7 parts; T=1 N=520 d=2: no odd slices
@pytest.mark.parametrize('T,N,D,tune', [(10, 520, 2, 6), (4, 640, 3, None), (1, 520, 2, None)])
def test_boundary_switches_change_no_bit(eng, T, N, D, tune, monkeypatch):
    X, Y = _net(41 + T, T, N, D)
    ref, q_ref = _lsm_three_iterations(eng, X, Y, tune, monkeypatch, SETTINGS[0])
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    assert not np.array_equal(ref[0][3], ref[0][0])                             # the chain moves
    if tune is None:
        assert ref[4].sum() > 0
    else:           # (the third step tunes and resets the counters: the step sizes have moved instead)
        assert np.any(ref[3] != 0.1) and np.all(ref[5] == 3)
    assert q_ref == _head_nodes(T, N, D)
    if (T, N) == (10, 520):
        assert q_ref == 8, 'the head launch was not spread: %d nodes per workgroup' % q_ref
    for setting in SETTINGS[1:]:
        got, q = _lsm_three_iterations(eng, X, Y, tune, monkeypatch, setting)
        assert q == (q_ref if setting[1] else 16)
        _same_bytes(got, ref, 'T=%d N=%d d=%d %s' % (T, N, D, dict(zip(SWITCHES, setting))))


def test_boundary_switches_with_two_chains_alive(eng, monkeypatch):
    """a second chain alive in the process: the resolvers multiply their own cross products (not served by the
    evaluators) - the block loads that read what the launch before stored write-through.  With a poll budget of
    zero a served resolver would give up at once and the call would fail: that the runs succeed shows that the
    resolvers took their own path"""
    T, N, D = 4, 520, 2
    X, Y = _net(7, T, N, D)
    monkeypatch.setenv('DLSM_PIPE_XBUDGET', '0')
    with eng.Chain(T, N, D, 'undirected', seed=1, chain_id=9) as other:
        other.upload_network(Y)
        ref, _ = _lsm_three_iterations(eng, X, Y, None, monkeypatch, SETTINGS[0])
        assert ref[4].sum() > 0
        for setting in SETTINGS[1:]:
            got, _ = _lsm_three_iterations(eng, X, Y, None, monkeypatch, setting)
            _same_bytes(got, ref, 'two chains %s' % (dict(zip(SWITCHES, setting)),))


def test_boundary_switches_hdp_lpcm(eng, monkeypatch):
    """the HDP-LPCM loop's sweeps (the same launches, the head possibly on the chain's second queue): the whole
    stored trace with the switches on and off"""
    T, N = 4, 520
    _, Y = _net(3, T, N, 2)
    res = []
    for setting in (SETTINGS[0], SETTINGS[-1]):
        _set(monkeypatch, setting)
        m = eng.DynamicNetworkHDPLPCM(n_iter=2, burn=1, tune=1, n_components=5, random_state=5, sweep_algo=4)
        m._prepare(Y); m._run(1, m._n_total - 1); m.chain_.synchronize()
        tr = m.chain_.hdp_trace_read(0, m._n_total)
        res.append([np.ascontiguousarray(tr[k]) for k in sorted(tr)])
        assert m.chain_.pipe_head_nodes() == _head_nodes(T, N, 2, spread=bool(setting[1]))
        m.chain_.close()            # (one chain alive at a time: the second run takes the same roles as the first)
    _same_bytes(res[1], res[0], 'HDP-LPCM')
    assert not np.array_equal(res[0][0][-1], res[0][0][0])
