"""The scaled-Dirichlet radii step of the directed and case-control device loops (kernels_dirloop.hpp:
philox_gamma, dir_radii_gamma_wg / _terms_wg / _finish_wg, tune_dirichlet, k_dir_tail's accept rule) in the
regimes the loop tests do not reach - concentrations below 1, rejected attempts, exact zeros and their
repair, a proposal that is 0 / 0, the tuning rule's factors, more nodes than k_dir_tail has threads - read
through dlsm_lsm_get_radii_step after every iteration, so that a rejected proposal is checked as well.

Inputs and the oracle's iterations come from tests/radii_ref.py; tests/test_radii_ref_cpu.py asserts, for
each of them, the conditions that make it reach its branch and that keep every decision clear of the
bounds below.  Needs an MI355X: -m gpu.

dir_q is held to the 60-digit value at the device's own proposal within c 2^-53 S (S: the sum of the
absolute values of its terms), c = 4 x the oracle's own largest ratio, at least 4 (radii_ref.device_q_factor).
Measured: the oracle's float64 expression reaches 1.31, so c = 5.24; the device
reaches 1.22 (MI355X).  Every case prints its ratios."""
import math

import numpy as np
import pytest

import radii_ref as rr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS = rr.EPS


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    from dynetlsm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, 'no HIP device: the engine has no CPU path'
    return dynetlsm_amd


def _open(eng, name, model, algo, step, n_total, tune=None):
    """a configured chain at the case's starting state, with an allocated trace"""
    inp = rr.case_inputs(name, model)
    N, T = inp['N'], inp['T']
    c = eng.Chain(T, N, 2, model, seed=rr.SEED, chain_id=rr.CHAIN)
    try:
        if model == 'case_control':
            cc = inp['cc']
            c.upload_edges(cc['in_edges'], cc['out_edges'], cc['degree'])
            c.set_controls(cc['control_nodes_in'], cc['control_nodes_out'])
        else:
            c.upload_network(inp['Yd'])
        c.set_positions(inp['X']); c.set_intercepts(rr.B0); c.set_radii(inp['radii'])
        c.set_prior_random_walk(rr.TAU_SQ, rr.SIGMA_SQ)
        x_step, x_tune = rr.x_sampler(name)
        c.set_samplers(eng.SamplerGrid(T, N, x_step, tune=x_tune, tune_interval=rr.X_TUNE_INTERVAL))
        _configure(c, algo, step, tune)
        lp0 = rr.make_loglik(inp)(inp['X'], rr.B0, inp['radii']) + orc.lsm_log_prior(
            inp['X'], rr.TAU_SQ, rr.SIGMA_SQ, rr.B0, rr.PRIOR_B, rr.VAR_B)
        c.trace_alloc(n_total, logp0=float(lp0))
    except Exception:
        c.close()
        raise
    return c


def _configure(c, algo, step, tune, state=None):
    c.lsm_configure(rr.PRIOR_B, rr.VAR_B, step_size_intercept=rr.I_STEP, tune=rr.I_TUNE,
                    tune_interval=rr.I_TUNE_INTERVAL, n_iter_procrustes=10 ** 6, sweep_algo=algo, state=state,
                    step_size_radii=step, radii_tune=tune[0] if tune else None,
                    radii_tune_interval=tune[1] if tune else 100)


def _check_iteration(tag, det, before, x, t, row, after, logp, step, seen):
    """one iteration of the device (proposal x, terms t, trace row, radii before / after) against the
    oracle's ``det``"""
    N = len(x)
    it = det['it']
    np.testing.assert_array_equal(after, row)
    if det['counts']['total'] == 0.0:
        # no proposal (0 / 0): the ratio is NaN and the step a rejection
        assert not (t['logu'] < (t['ll_proposal'] - t['ll_current']) + t['dir_q'])
        assert np.isnan((t['ll_proposal'] - t['ll_current']) + t['dir_q'])
        assert np.all(np.isfinite(row)) and np.array_equal(row, before)
        assert np.isfinite(logp)
        np.testing.assert_allclose(logp, det['logp'], rtol=rr.RTOL_LL)
        seen['nan'] += 1
        return
    # the proposal
    np.testing.assert_allclose(x, det['x'], rtol=rr.RTOL_RADII, atol=0)
    assert abs(math.fsum(x) - 1.0) <= N * EPS, (tag, it, math.fsum(x) - 1.0)
    if det['zero_repair']:
        assert x.min() > 0
        x0 = det['gammas'] * (1.0 / det['gammas'].sum())
        np.testing.assert_allclose(x, (x0 + 1e-5) / np.sum(x0 + 1e-5), rtol=rr.RTOL_RADII, atol=0)
        seen['repairs'] += 1
    # dir_q against the 60-digit value at the device's own proposal
    q_mp, S = rr.dir_q_mp(before, x, step)
    ratio_q = abs(t['dir_q'] - q_mp) / (EPS * S)
    seen['q_ratios'].append(ratio_q)
    print('%s it %d: device dir_q ratio %.3f (allowed %.3f), S %.3e' % (tag, it, ratio_q, rr.device_q_factor(), S))
    assert ratio_q <= rr.device_q_factor(), (tag, it, t['dir_q'], q_mp, S)
    # log u, the two log-likelihoods
    assert abs(t['logu'] - det['logu']) <= 4 * np.spacing(abs(det['logu'])), (tag, it, t['logu'], det['logu'])
    assert np.isfinite(t['ll_proposal']) and np.isfinite(t['ll_current'])
    np.testing.assert_allclose(t['ll_proposal'], det['ll_prop'], rtol=rr.RTOL_LL)
    np.testing.assert_allclose(t['ll_current'], det['ll_cur'], rtol=rr.RTOL_LL)
    # the decision: from the four values read back, in the trace, in the oracle
    accepted = not (t['logu'] >= (t['ll_proposal'] - t['ll_current']) + t['dir_q'])
    if accepted:
        np.testing.assert_array_equal(row, x)
    else:
        np.testing.assert_array_equal(row, before)
    assert accepted == bool(det['accepted']), (tag, it)
    np.testing.assert_allclose(after, det['radii_after'], rtol=rr.RTOL_RADII, atol=0)
    np.testing.assert_allclose(logp, det['logp'], rtol=rr.RTOL_LL)
    seen['accepted'] += int(accepted)


def _run_case(eng, name, model, algo):
    cs, inp, ref = rr.CASES[name], rr.case_inputs(name, model), rr.oracle_run(name, model)
    n_total = len(ref) + 1
    tag = '%s %s algo %d' % (name, model, algo)
    seen = dict(nan=0, repairs=0, accepted=0, q_ratios=[])
    c = _open(eng, name, model, algo, cs['phases'][0][0], n_total)
    with c:
        it = 0
        for pi, (step, count) in enumerate(cs['phases']):
            if pi > 0:      # the next phase's concentration; the intercepts' samplers go on where they are
                g = c.lsm_get_config()
                _configure(c, algo, step, None, state=[(g.i_step_size[k], g.i_n_accepted[k], g.i_n_steps[k],
                                                        g.i_steps_until_tune[k]) for k in range(2)])
            for k in range(count):
                it += 1
                if cs.get('starved'):
                    c.set_radii(inp['radii'])
                before = c.get_radii()
                c.lsm_run(it, 1)
                x, t = c.radii_step_read()
                row = c.trace_read_radii(it, 1)[0]
                logp = c.trace_read(it, 1, positions=False)[2][0]
                _check_iteration(tag, ref[it - 1], before, x, t, row, c.get_radii(), logp, step, seen)
                g = c.lsm_get_config()
                assert g.r_n_steps == k + 1 == ref[it - 1]['sampler'][2]
                assert g.r_n_accepted == ref[it - 1]['sampler'][1]
                assert g.r_step_size == step
        Xs = c.trace_read(0, n_total)[0]
    print('%s: largest device dir_q ratio %.3f, %d accepted, %d repaired, %d without a proposal'
          % (tag, max(seen['q_ratios'], default=0.0), seen['accepted'], seen['repairs'], seen['nan']))
    assert np.all(np.isfinite(Xs))
    return seen


def test_mixed_concentrations_take_both_forms_of_the_sampler(eng):
    """N = 513, a = 0.1 .. 2.3: Gamma(a + 1) U^(1 / a) beside the plain form in every workgroup, t <= 0
    rejections, variates accepted at a later attempt (counts: test_radii_ref_cpu.py)"""
    _run_case(eng, 'mixed', 'directed', 4)


def test_five_proposal_workgroups_and_the_tails_stride(eng):
    """N = 1025: five proposal workgroups, and node 1024 is the one k_dir_tail's 1024 threads reach in
    their second trip - the accepted row and the stored radii are the proposal there as everywhere"""
    seen = _run_case(eng, 'five_workgroups', 'directed', 4)
    assert seen['accepted'] >= 1


@pytest.mark.parametrize('model,algo', [('directed', 4), ('case_control', 4), ('case_control', 5)])
def test_zero_repair(eng, model, algo):
    """four starved nodes (0, 100, 255 in the first proposal workgroup of N = 257, 256 in the second) draw
    exact zeros in every iteration: the repair, its second normalisation over N > 256 and - case-control -
    the second write of the reciprocal radius into the gather records, which the likelihood at the proposal
    reads.  (The positions move by 1e-8 here: radii_ref.CASES says why.)"""
    seen = _run_case(eng, 'zero_repair', model, algo)
    assert seen['repairs'] == 6 and seen['accepted'] >= 1


@pytest.mark.parametrize('model,algo', [('directed', 1), ('case_control', 1)])
def test_tiny_radii_without_a_zero(eng, model, algo):
    """proposal entries down to 1e-94 and no zero: no repair, and the likelihood at the proposal is finite"""
    seen = _run_case(eng, 'tiny', model, algo)
    assert seen['repairs'] == 0


def test_a_proposal_without_a_total_is_rejected(eng):
    """every gamma variate underflows in some iterations: the proposal is 0 / 0, the ratio NaN - a rejection,
    finite rows and log-posterior, counted as a step and not as an acceptance (in the other iterations a
    single variate survives and the rest are repaired zeros)"""
    seen = _run_case(eng, 'all_zero', 'directed', 1)
    assert seen['nan'] >= 1


@pytest.mark.parametrize('name', ['tune_down', 'tune_up'])
def test_tuning_rule(eng, name):
    """80 iterations with a tuning every 5: between them the two runs apply 0.1, 0.5, 0.9, 1.1 and 10
    (test_radii_ref_cpu.py); one call per iteration against the oracle's sampler, then the same 80 in one
    call, bit for bit"""
    cs, ref = rr.CASES[name], rr.oracle_run(name, 'directed')
    step0, n = cs['phases'][0]
    out = []
    with _open(eng, name, 'directed', 1, step0, n + 1, tune=cs['tune']) as c:
        for it in range(1, n + 1):
            c.lsm_run(it, 1)
            g = c.lsm_get_config()
            st, na, ns, un = ref[it - 1]['sampler']
            np.testing.assert_allclose(g.r_step_size, st, rtol=1e-14)
            assert (g.r_n_accepted, g.r_n_steps, g.r_steps_until_tune) == (na, ns, un), it
        out.append(c.trace_read(0, n + 1) + (c.trace_read_radii(0, n + 1),) + (_counters(c),))
    np.testing.assert_allclose(out[0][3], np.array([rr.case_inputs(name, 'directed')['radii']] +
                                                   [d['radii_after'] for d in ref]), rtol=rr.RTOL_RADII, atol=0)
    with _open(eng, name, 'directed', 1, step0, n + 1, tune=cs['tune']) as c:
        c.lsm_run(1, n)
        out.append(c.trace_read(0, n + 1) + (c.trace_read_radii(0, n + 1),) + (_counters(c),))
    for a, b in zip(out[0][:4], out[1][:4]):
        np.testing.assert_array_equal(a, b)
    assert out[0][4] == out[1][4]


def _counters(c):
    g = c.lsm_get_config()
    return (g.r_step_size, g.r_n_accepted, g.r_n_steps, g.r_steps_until_tune,
            tuple(g.i_step_size), tuple(g.i_n_accepted), tuple(g.i_n_steps), tuple(g.i_steps_until_tune))


def test_radii_step_read_bad_arguments(eng):
    from dynetlsm_amd import _lib
    L = _lib.load()
    inp = rr.case_inputs('tiny', 'directed')
    N, T = inp['N'], inp['T']
    buf, terms = np.zeros(N), np.zeros(4)
    # an undirected chain has no radii step
    with eng.Chain(T, N, 2, 'undirected', seed=1) as c:
        with pytest.raises(eng.EngineError) as e:
            c.radii_step_read()
        assert e.value.code == -1
    with eng.Chain(T, N, 2, 'directed', seed=rr.SEED, chain_id=rr.CHAIN) as c:
        with pytest.raises(eng.EngineError) as e:       # not configured
            c.radii_step_read()
        assert e.value.code == -1
    with _open(eng, 'tiny', 'directed', 1, 1.5, 3) as c:
        with pytest.raises(eng.EngineError) as e:       # configured, no iteration yet
            c.radii_step_read()
        assert e.value.code == -1 and 'dlsm_lsm_run' in str(e.value)
        c.lsm_run(1, 0)
        with pytest.raises(eng.EngineError):            # ... and a run of no iteration is none
            c.radii_step_read()
        c.lsm_run(1, 1)
        x, t = c.radii_step_read()
        x2, t2 = c.radii_step_read()                    # read-only: twice the same
        assert np.array_equal(x, x2) and t == t2
        p = _lib.c_double_p
        assert L.dlsm_lsm_get_radii_step(c._h, None, terms.ctypes.data_as(p)) == -1
        assert L.dlsm_lsm_get_radii_step(c._h, buf.ctypes.data_as(p), None) == -1
        assert L.dlsm_lsm_get_radii_step(None, buf.ctypes.data_as(p), terms.ctypes.data_as(p)) == -1
        # a log-likelihood call reuses the step's buffers: nothing stale is handed out
        c.loglik_full_radii(c.get_radii())
        with pytest.raises(eng.EngineError) as e:
            c.radii_step_read()
        assert e.value.code == -1
        c.lsm_run(2, 1)
        assert len(c.radii_step_read()[0]) == N
