"""References for the scaled-Dirichlet radii step of the directed loops (kernels_dirloop.hpp):

``dir_q_mp``      the proposal density ratio  log Dir(radii | step x) - log Dir(x | step radii)  of given
                  float64 (radii, x, step) in mpmath, with the scale S its rounding errors are measured in;
``gamma_counts``  a counting copy of the oracle's gamma sampler (oracle.philox_gamma): which of its branches
                  an input takes, and how often;
``CASES`` / ``oracle_run``  the inputs of tests/test_gpu_radii_step.py and the oracle's iterations on them,
                  computed once per process and shared by the CPU test (which asserts, for every input, the
                  conditions the GPU test relies on) and the GPU test (which compares the device against them).
"""
import functools

import numpy as np

from oracle import oracle as orc

EPS = 2.0 ** -53
RTOL_LL = 1e-10         # the project's log-likelihood tolerance (tests/test_gpu_parity.py)
RTOL_RADII = 1e-10      # ... and the radii's


# ------------------------------------------------------------------------------------------ q in mpmath
def dir_q_mp(radii, x, step, dps=60):
    """(q, S): q as a float rounded from ``dps`` digits, the float64 inputs taken as exact; S = the sum of
    the absolute values of every lgamma and every (.) log(.) term of q, in float"""
    import mpmath
    with mpmath.workdps(dps):
        mp = mpmath.mpf
        st = mp(float(step))
        r = [mp(float(v)) for v in radii]
        xx = [mp(float(v)) for v in x]
        terms = [mpmath.loggamma(st * mpmath.fsum(xx)), -mpmath.loggamma(st * mpmath.fsum(r))]
        for xi, ri in zip(xx, r):
            terms.append(-mpmath.loggamma(st * xi))
            terms.append((st * xi - 1) * mpmath.log(ri))
            terms.append(mpmath.loggamma(st * ri))
            terms.append(-(st * ri - 1) * mpmath.log(xi))
        q = mpmath.fsum(terms)
        S = mpmath.fsum([abs(t) for t in terms])
        return float(q), float(S)


def dir_q_double(radii, x, step):
    """the oracle's float64 expression (oracle.directed_coefficient_steps)"""
    from scipy.special import gammaln
    return ((gammaln(step * x.sum()) - gammaln(step * x).sum() + ((step * x - 1) * np.log(radii)).sum()) -
            (gammaln(step * radii.sum()) - gammaln(step * radii).sum() + ((step * radii - 1) * np.log(x)).sum()))


# ------------------------------------------------------------------------------------------ the sampler, counting
def gamma_counts(seed, chain, it, step, radii):
    """oracle.philox_gamma for every node of ``radii`` at concentration step * radii[i], with counters:
    small = draws at a < 1 (the Gamma(a + 1) U^(1 / a) form), t_rejects = attempts thrown away at t <= 0,
    later = variates accepted at an attempt after the first, zeros = variates that are exactly 0,
    subnormal = non-zero variates below the normal range, zero_nodes, total = their sum (numpy's), gammas"""
    sw = orc.stream_word(chain, orc.STREAM_RADII)
    out = dict(small=0, t_rejects=0, later=0, zeros=0, subnormal=0, zero_nodes=[])
    g = np.zeros(len(radii))
    for i, ri in enumerate(radii):
        a = step * ri
        aa = a + 1.0 if a < 1.0 else a
        d = aa - 1.0 / 3.0
        cc = 1.0 / np.sqrt(9.0 * d)
        out['small'] += int(a < 1.0)
        for att in range(4096):
            u0, u1 = orc.philox_uniform2(seed, i, 2 * att, it, sw)
            z0, _ = orc._box_muller(float(u0), float(u1))
            w0, w1 = orc.philox_uniform2(seed, i, 2 * att + 1, it, sw)
            w0, w1 = float(w0), float(w1)
            t = 1.0 + cc * z0
            if t <= 0.0:
                out['t_rejects'] += 1
                continue
            v = t * t * t
            x2 = z0 * z0
            if w0 < 1.0 - 0.0331 * x2 * x2 or np.log(w0) < 0.5 * x2 + d * (1.0 - v + np.log(v)):
                val = d * v
                if a < 1.0:
                    val *= w1 ** (1.0 / a)
                g[i] = val
                out['later'] += int(att > 0)
                break
        if g[i] == 0.0:
            out['zeros'] += 1
            out['zero_nodes'].append(i)
        elif g[i] < np.finfo(np.float64).tiny:
            out['subnormal'] += 1
    out['gammas'] = g
    out['total'] = float(g.sum())
    return out


# ------------------------------------------------------------------------------------------ the cases
SEED, CHAIN = 23, 2
B0 = np.array([0.4, 0.7])
PRIOR_B, VAR_B = np.array([0.3, 0.5]), 2.0
TAU_SQ, SIGMA_SQ = 1e-3, 1e-4
X_STEP, X_TUNE, X_TUNE_INTERVAL = 0.01, 6, 2        # the positions' sampler grid
I_STEP, I_TUNE, I_TUNE_INTERVAL = 0.1, 6, 2         # the intercepts' samplers
N_CONTROL, CONTROL_SEED = 8, 5
STARVED = (0, 100, 255, 256)

# name -> N, T, phases [(step_size_radii, iterations)], starved nodes, (radii_tune, radii_tune_interval),
# and the chains [(model, sweep_algo)] it runs on
CASES = {
    'mixed': dict(N=513, T=2, phases=[(0.6 * 513, 6)], chains=[('directed', 4)]),
    'five_workgroups': dict(N=1025, T=1, phases=[(0.6 * 1025, 3), (1e9, 3)], chains=[('directed', 4)]),
    # (x_step: the positions move by 1e-8, untuned.  A tie of a starved node has b / r = 4e8, so a move of 0.01
    # changes its term of a log-ratio by 1e6, and the pipelined sweeps - algo 4, both models - carry a node's
    # corrections for its batch's earlier acceptances as FACTORS e^delta (the H blocks), which leave the float64
    # range at |delta| > 700: with the other cases' step of 0.01 their decisions, and so the positions every
    # later value depends on, differ from the oracle's in the first iteration.  That is a limit of the sweep at
    # radii no chain keeps at a node with ties, not of the step under test, which reads
    # the positions and nothing else of the sweep.)
    'zero_repair': dict(N=257, T=2, phases=[(175000., 6)], starved=STARVED, x_step=1e-8, x_tune=None,
                        chains=[('directed', 4), ('case_control', 4), ('case_control', 5)]),
    'tiny': dict(N=30, T=2, phases=[(0.05 * 30, 6)], chains=[('directed', 1), ('case_control', 1)]),
    'all_zero': dict(N=30, T=2, phases=[(1e-3, 6)], chains=[('directed', 1)]),
    'tune_down': dict(N=30, T=2, phases=[(3e7, 80)], tune=(80, 5), chains=[('directed', 1)]),
    'tune_up': dict(N=30, T=2, phases=[(30., 80)], tune=(80, 5), chains=[('directed', 1)]),
}
# every per-iteration check applies (all_zero: in the iterations whose gamma total is not 0)
STEP_CASES = ['mixed', 'five_workgroups', 'zero_repair', 'tiny', 'all_zero']
RUNS = [(name, model, algo) for name in CASES for model, algo in CASES[name]['chains']]


def _rand_net(seed, T, N, D=2, density=0.2, scale=1.0):
    """tests/test_gpu_parity.py's generator (that module needs a device to be of use; this one does not)"""
    rng = np.random.RandomState(seed)
    X = rng.randn(T, N, D) * scale
    Yd = (rng.rand(T, N, N) < density).astype(np.float64)
    for t in range(T):
        np.fill_diagonal(Yd[t], 0)
    Yu = np.triu(Yd, 1)
    Yu = Yu + Yu.transpose(0, 2, 1)
    radii = rng.dirichlet(np.ones(N) * 5)
    return X, Yd, Yu, radii


def _cc_lists(Yd, n_control, seed):
    """tests/test_gpu_parity.py's: edge lists as the reference builds them + valid random controls"""
    T, N, _ = Yd.shape
    deg, ie, oe = orc.case_control_init(Yd)
    rng = np.random.RandomState(seed)
    ci = np.full((T, N, n_control), -1, dtype=np.int64)
    co = np.full((T, N, n_control), -1, dtype=np.int64)
    for t in range(T):
        for i in range(N):
            zo = np.setdiff1d(np.arange(N), np.append(oe[t, i, :deg[t, i, 1]], i))
            zi = np.setdiff1d(np.arange(N), np.append(ie[t, i, :deg[t, i, 0]], i))
            k = min(n_control, zo.size)
            co[t, i, :k] = rng.choice(zo, k, replace=False)
            k = min(n_control, zi.size)
            ci[t, i, :k] = rng.choice(zi, k, replace=False)
    return dict(in_edges=ie, out_edges=oe, degree=deg, control_nodes_in=ci, control_nodes_out=co)


@functools.lru_cache(maxsize=None)
def case_inputs(name, model):
    """the network, positions and radii of a case, as test_gpu_parity.directed_loop_case builds them"""
    cs = CASES[name]
    N, T = cs['N'], cs['T']
    X, Yd, _, radii = _rand_net(31 + N, T, N, 2, scale=0.05, density=0.1)
    if cs.get('starved'):
        radii = radii.copy()
        radii[list(cs['starved'])] = 1e-9 * radii.sum()     # (these nodes keep their ties)
        radii /= radii.sum()
    cc = _cc_lists(Yd, N_CONTROL, CONTROL_SEED) if model == 'case_control' else None
    return dict(X=X, Yd=Yd, radii=radii, cc=cc, N=N, T=T)


def x_sampler(name):
    """(step_size, tune) of the positions' sampler grid of a case"""
    cs = CASES[name]
    return cs.get('x_step', X_STEP), cs.get('x_tune', X_TUNE)


def make_loglik(inp):
    if inp['cc'] is not None:
        cc = inp['cc']

        def loglik(Xc, b, r):
            return orc.approx_directed_network_loglikelihood(Xc, r, cc['in_edges'], cc['out_edges'], cc['degree'],
                                                             cc['control_nodes_out'], b[0], b[1])
    else:
        Yd = inp['Yd']

        def loglik(Xc, b, r):
            return orc.dynamic_network_loglikelihood_directed(Yd, Xc, b[0], b[1], r)
    return loglik


@functools.lru_cache(maxsize=None)
def oracle_run(name, model):
    """The oracle's iterations of a case (the sweep algorithm does not enter: every algorithm of the device
    is held to the same oracle).  A list, one entry per iteration ``it`` = 1 .., of dicts: the radii step's
    intermediates (oracle.directed_coefficient_steps' ``details``), the sampler's branch counts
    (``gamma_counts``), radii_after, logp, and the radii sampler's (step_size, n_accepted, n_steps,
    steps_until_tune) after the iteration.  Read only: the tests share it."""
    cs, inp = CASES[name], case_inputs(name, model)
    N, T = inp['N'], inp['T']
    loglik = make_loglik(inp)
    kw = dict(case_control=inp['cc']) if model == 'case_control' else dict(Y=inp['Yd'])
    x_step, x_tune = x_sampler(name)
    og = orc.SamplerGrid(T, N, x_step, tune=x_tune, tune_interval=X_TUNE_INTERVAL)
    st = orc.ChainState(inp['X'], og, model=1 if model == 'directed' else 2, intercept=B0,
                        radii=inp['radii'].copy(), tau_sq=TAU_SQ, sigma_sq=SIGMA_SQ, seed=SEED, chain=CHAIN, **kw)
    isamp = [orc.ScalarMetropolis(I_STEP, I_TUNE, I_TUNE_INTERVAL) for _ in range(2)]
    tune = cs.get('tune')
    out, it = [], 0
    with np.errstate(all='ignore'):
        for step, count in cs['phases']:
            rsamp = (orc.ScalarMetropolis(step, tune[0], tune[1]) if tune else orc.ScalarMetropolis(step, None, 100))
            for _ in range(count):
                it += 1
                if cs.get('starved'):
                    st.radii[:] = inp['radii']
                det = {}
                counts = gamma_counts(SEED, CHAIN, it, rsamp.step_size, st.radii)
                lp = orc.lsm_iteration_directed(st, it, loglik, isamp, rsamp, PRIOR_B, VAR_B, details=det)
                det.update(counts=counts, radii_after=st.radii.copy(), logp=lp, it=it,
                           sampler=(rsamp.step_size, rsamp.n_accepted, rsamp.n_steps, rsamp.steps_until_tune))
                out.append(det)
    return out


def q_check(det):
    """(q in mpmath from the oracle's own x, S, the oracle's ratio |q_double - q_mp| / (2^-53 S))"""
    q_mp, S = dir_q_mp(det['radii0'], det['x'], det['step'])
    return q_mp, S, abs(det['q'] - q_mp) / (EPS * S)


@functools.lru_cache(maxsize=None)
def oracle_q_ratios():
    """{(case, model, it): ratio} over every iteration of STEP_CASES with a proposal (a gamma total > 0)"""
    out = {}
    for name, model, _ in RUNS:
        if name in STEP_CASES:
            for det in oracle_run(name, model):
                if det['counts']['total'] > 0:
                    out[(name, model, det['it'])] = q_check(det)[2]
    return out


def device_q_factor():
    """what the device's dir_q may miss the mpmath value by, in units of 2^-53 S: four times the oracle's own
    largest ratio and at least 4 - one device-library transcendental and one multiply per term against
    glibc's and scipy's, a block-tree sum against numpy's pairwise sum"""
    return 4.0 * max(1.0, max(oracle_q_ratios().values()))


def decision_bound(det, S):
    """the sum of what the accept test's sides may differ by between device and oracle: dir_q at the same x,
    dir_q's first-order change over a proposal that differs by RTOL_RADII in every entry, both
    log-likelihoods, log u (4 ulp)"""
    from scipy.special import digamma
    step, x, r = det['step'], det['x'], det['radii0']
    dq_dlnx = np.abs(step * x * digamma(step * x)) + np.abs(step * x * np.log(r)) + np.abs(step * r - 1.0)
    return (device_q_factor() * EPS * S + RTOL_RADII * (dq_dlnx.sum() + abs(step * digamma(step))) +
            RTOL_LL * (abs(det['ll_prop']) + abs(det['ll_cur'])) + 4 * np.spacing(abs(det['logu'])))
