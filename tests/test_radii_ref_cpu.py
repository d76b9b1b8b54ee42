"""The references of the radii step (tests/radii_ref.py) against the oracle, and - for every input that
tests/test_gpu_radii_step.py uses - the conditions that make that input reach the branch it is there for.
A condition that does not hold shows here, without a device."""
import numpy as np
import pytest

import radii_ref as rr
from oracle import oracle as orc

STEP_RUNS = sorted({(n, m) for n, m, _ in rr.RUNS if n in rr.STEP_CASES})
ALL_RUNS = sorted({(n, m) for n, m, _ in rr.RUNS})


def _totals(run, key):
    return sum(det['counts'][key] for det in run)


# ------------------------------------------------------------------------------------------ the helpers
def test_dir_q_mp_symmetries():
    rng = np.random.RandomState(0)
    r, x = rng.dirichlet(np.full(7, 0.3)), rng.dirichlet(np.full(7, 2.0))
    q, S = rr.dir_q_mp(r, r, 12.5)
    assert q == 0.0 and S > 0
    q1, S1 = rr.dir_q_mp(r, x, 12.5)
    q2, S2 = rr.dir_q_mp(x, r, 12.5)
    assert q1 == -q2 and S1 == S2 and q1 != 0.0
    # a lower working precision gives the same float: 60 digits are plenty
    assert rr.dir_q_mp(r, x, 12.5, dps=50) == (q1, S1)
    # N = 2, step = 2: Dir(x | 2 r) by hand.  log B(a, b) = lgamma(a) + lgamma(b) - lgamma(a + b)
    import math
    r2, x2 = np.array([0.25, 0.75]), np.array([0.5, 0.5])

    def logpdf(v, a):
        return (math.lgamma(a.sum()) - sum(math.lgamma(t) for t in a) + sum((t - 1) * math.log(u) for t, u in zip(a, v)))
    np.testing.assert_allclose(rr.dir_q_mp(r2, x2, 2.0)[0], logpdf(r2, 2.0 * x2) - logpdf(x2, 2.0 * r2), rtol=1e-14)


@pytest.mark.parametrize('name,model', ALL_RUNS)
def test_gamma_counts_draws_what_the_oracle_draws(name, model):
    for det in rr.oracle_run(name, model):
        assert np.array_equal(det['counts']['gammas'], det['gammas'])
        assert det['counts']['zeros'] == int(np.sum(det['gammas'] == 0.0))


def test_oracle_q_in_double_against_mpmath():
    """the oracle's float64 dir_q misses the 60-digit value by a small multiple of 2^-53 S: a rounding per
    transcendental, per product and per level of numpy's pairwise sum, and the few ulp of sum(x) under the
    leading lgamma - 16 units hold all of that.  The largest ratio sets the device's allowance."""
    ratios = rr.oracle_q_ratios()
    for key in sorted(ratios):
        print('oracle dir_q ratio %-16s %-12s it %d: %.3f' % (key + (ratios[key],)))
    print('largest %.3f -> device factor %.3f' % (max(ratios.values()), rr.device_q_factor()))
    assert max(ratios.values()) <= 16.0
    assert rr.device_q_factor() >= 4.0
    # and the helper's float64 expression is the oracle's
    det = rr.oracle_run('mixed', 'directed')[0]
    assert rr.dir_q_double(det['radii0'], det['x'], det['step']) == det['q']


# ------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize('name,model', STEP_RUNS)
def test_no_decision_of_a_case_lies_inside_the_bounds(name, model):
    """|log u - ratio| is larger than everything device and oracle may differ by, in every iteration: the
    device must then take the oracle's decision, with no exemption"""
    for det in rr.oracle_run(name, model):
        if name == 'all_zero' and det['counts']['total'] == 0.0:
            continue                                    # no proposal: the device test asserts the rejection
        assert np.isfinite(det['ratio']) and np.isfinite(det['logu'])
        _, S, _ = rr.q_check(det)
        bound = rr.decision_bound(det, S)
        margin = abs(det['logu'] - det['ratio'])
        print('%s %s it %d: margin %.3e, bound %.3e, accepted %d' % (name, model, det['it'], margin, bound,
                                                                  det['accepted']))
        assert margin > 10 * bound


@pytest.mark.parametrize('name,model', STEP_RUNS)
def test_no_variate_of_a_case_is_subnormal(name, model):
    """a variate in the subnormal range has fewer than 53 bits: pow's last-place rounding there is a
    relative error that rtol = 1e-10 on the proposal does not cover"""
    assert _totals(rr.oracle_run(name, model), 'subnormal') == 0


def test_case_mixed_takes_both_forms_of_the_sampler():
    run = rr.oracle_run('mixed', 'directed')
    a = run[0]['step'] * run[0]['radii0']
    assert a.min() < 0.2 and a.max() > 2.0
    for wg in range(3):                                 # both forms in every workgroup of 256 nodes
        aw = a[wg * 256:(wg + 1) * 256]
        assert np.any(aw < 1.0) and (np.any(aw >= 1.0) or wg == 2)
    assert _totals(run, 'small') >= 1000
    assert _totals(run, 't_rejects') >= 1
    assert _totals(run, 'later') >= 20
    assert _totals(run, 'zeros') == 0 and not any(det['zero_repair'] for det in run)
    print('mixed: a < 1 %d, t <= 0 %d, later attempt %d' % (_totals(run, 'small'), _totals(run, 't_rejects'),
                                                            _totals(run, 'later')))


def test_case_five_workgroups_accepts():
    run = rr.oracle_run('five_workgroups', 'directed')
    assert len(run[0]['x']) == 1025 and (1025 + 255) // 256 == 5 and 1025 > 1024
    assert sum(det['accepted'] for det in run) >= 1
    assert sum(det['accepted'] for det in run[3:]) >= 1
    for det in run[3:]:             # at step 1e9 the proposal is the current radii to 1 / sqrt(1e9 / N) = 1e-3 or so
        np.testing.assert_allclose(det['x'], det['radii0'], rtol=0.02)
    assert _totals(run, 'zeros') == 0
    print('five_workgroups: accepted', [det['accepted'] for det in run])


@pytest.mark.parametrize('model', ['directed', 'case_control'])
def test_case_zero_repair_repairs_in_every_iteration(model):
    run = rr.oracle_run('zero_repair', model)
    nodes = set()
    for det in run:
        c = det['counts']
        assert c['zeros'] >= 1 and det['zero_repair']
        assert np.isfinite(c['total']) and c['total'] >= np.finfo(np.float64).tiny
        nodes |= set(c['zero_nodes'])
        x0 = det['gammas'] * (1.0 / det['gammas'].sum())
        np.testing.assert_allclose(det['x'], (x0 + 1e-5) / np.sum(x0 + 1e-5), rtol=1e-15)
        assert det['x'].min() > 0
        assert np.isfinite(det['ll_prop']) and np.isfinite(det['ll_cur'])
        assert np.array_equal(det['radii0'], rr.case_inputs('zero_repair', model)['radii'])
    assert nodes <= set(rr.STARVED)
    assert any(i < 256 for i in nodes) and any(i >= 256 for i in nodes)     # both workgroups
    # the starved nodes have ties: a reciprocal of an unrepaired zero in the records would show in the likelihood
    Yd = rr.case_inputs('zero_repair', model)['Yd']
    for i in rr.STARVED:
        assert Yd[:, i, :].sum() > 0 and Yd[:, :, i].sum() > 0
    print('zero_repair %s: %d zeros in %d iterations, nodes %s' % (model, _totals(run, 'zeros'), len(run),
                                                                  sorted(nodes)))


@pytest.mark.parametrize('model', ['directed', 'case_control'])
def test_case_tiny_has_no_zero_and_a_finite_likelihood(model):
    run = rr.oracle_run('tiny', model)
    assert _totals(run, 'zeros') == 0 and not any(det['zero_repair'] for det in run)
    assert all(np.isfinite(det['ll_prop']) for det in run)
    smallest = min(det['x'].min() for det in run)
    assert 0 < smallest < 1e-60          # far below anything the other cases propose
    print('tiny %s: smallest proposal entry %.3e' % (model, smallest))


def test_case_all_zero_is_rejected_by_the_oracle():
    """every gamma variate underflows: total 0, the proposal 0 / 0.  The ratio is NaN and the step a rejection"""
    run = rr.oracle_run('all_zero', 'directed')
    r0 = rr.case_inputs('all_zero', 'directed')['radii']
    n_nan = 0
    for det in run:
        if det['counts']['total'] == 0.0:
            n_nan += 1
            assert np.all(np.isnan(det['x'])) and np.isnan(det['ratio']) and not det['zero_repair']
            assert det['accepted'] == 0
        assert np.isfinite(det['logp'])
        if not det['accepted']:
            assert np.array_equal(det['radii_after'], det['radii0'])
        assert np.all(np.isfinite(det['radii_after']))
    assert n_nan >= 1
    assert run[-1]['sampler'][2] == len(run) and run[-1]['sampler'][1] == sum(det['accepted'] for det in run)
    if n_nan == len(run):
        assert np.array_equal(run[-1]['radii_after'], r0)
    print('all_zero: gamma total exactly 0 in %d of %d iterations' % (n_nan, len(run)))


class _NanDirichlet:
    def __init__(self):
        self.rs = np.random.RandomState(0)
        self.rand = self.rs.rand

    def dirichlet(self, alpha):
        return np.full(len(alpha), np.nan)


def test_step_dirichlet_rejects_a_proposal_that_is_not_finite():
    s = orc.ScalarMetropolis(1e-3, None, 100)
    x0 = np.array([0.2, 0.3, 0.5])
    with np.errstate(all='ignore'):
        x = s.step_dirichlet(x0, lambda v: -np.sum(v * v), _NanDirichlet())
    assert np.array_equal(x, x0) and s.n_steps == 1 and s.n_accepted == 0


def _factors(run, step0):
    steps = [step0] + [det['sampler'][0] for det in run]
    return sorted({round(b / a, 12) for a, b in zip(steps, steps[1:]) if b != a})


def test_case_tuning_applies_five_of_the_six_factors():
    down = _factors(rr.oracle_run('tune_down', 'directed'), 3e7)
    up = _factors(rr.oracle_run('tune_up', 'directed'), 30.)
    print('tune_down factors', down, 'tune_up factors', up)
    assert set(down) | set(up) >= {0.1, 0.5, 0.9, 1.1, 10.0}
    assert set(down) | set(up) <= {0.1, 0.5, 0.9, 1.1, 2.0, 10.0}
    for name in ('tune_down', 'tune_up'):
        run = rr.oracle_run(name, 'directed')
        assert len(run) == 80 and run[-1]['sampler'][2] == 80
        assert all(np.all(np.isfinite(det['radii_after'])) for det in run)
