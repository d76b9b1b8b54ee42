"""Pins tests/labels_ref.py (the long-double replica that tests/test_gpu_labels_shapes.py compares the label
kernels with) to the oracle, shows that every case reaches the kernel form it is listed for and that the
restated dispatch still uses the constants of the sources, and establishes the tie condition under which the
GPU test compares labels exactly: every draw of every case lies at least 1e-9 from a cumulative probability,
and the device's error in that probability is bounded by 1e-11 (derivation: labels_ref's docstring).  No GPU."""
import os
import re

import numpy as np
import pytest

import labels_ref as lr
from oracle import oracle as orc
from oracle.hdp_sums import NumpyLabelSums

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dynetlsm_amd', 'csrc')
MIN_MARGIN, MAX_BOUND = 1e-9, 1e-11


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    hits = re.findall(pattern, text)
    assert len(hits) == 1, (pattern, hits)
    return int(hits[0])


def test_constants_are_those_of_the_sources():
    hpp, capi, hdp = _source('kernels_labels.hpp'), _source('capi.hip'), _source('kernels_hdp.hpp')
    for name in ('LM_THREADS', 'LM_NODES', 'LM_MAX_KS', 'LAB_WAVES', 'LC_THREADS'):
        assert _one(r'constexpr int %s = (\d+);' % name, hpp) == getattr(lr, name), name
    assert _one(r'constexpr int WPRE = (\d+);', hpp) == lr.LM_WPRE
    counts = hpp[hpp.index('void k_label_counts('):]
    assert _one(r'constexpr int PRE = (\d+);', counts) == lr.LC_PRE
    assert _one(r'lm_lds_bytes\(h->T, h->K, h->D\) <= (\d+) \* 1024', capi) * 1024 == lr.MFMA_LDS_MAX
    assert _one(r'lds_tables > (\d+) \* 1024', capi) * 1024 == lr.WAVE_TABLES_MAX
    assert _one(r'lds_tables \+ lds_w <= (\d+) \* 1024', capi) * 1024 == lr.WAVE_W_LDS_MAX
    assert _one(r'h->K <= (\d+) \* LM_MAX_KS', capi) == 4
    assert _one(r'constexpr int HDP_THREADS = (\d+);', hdp) == lr.HDP_THREADS
    assert _one(r'constexpr int NU = (\d+);', hdp) == lr.HDP_NU


def test_every_case_reaches_the_form_it_is_listed_for():
    for case in lr.CASES + [lr.REFUSED]:
        T, N, D, K = case.dims
        assert lr.form(T, K, D) == case.want, case
    forms = {c.want for c in lr.CASES + [lr.REFUSED]}
    assert forms == {'mfma KS=%d' % ks for ks in range(1, 9)} | {'wave WLDS=1', 'wave WLDS=0', 'refused'}
    # each form's far-node case
    assert {c.want.split()[0] for c in lr.CASES if c.far} == {'mfma', 'wave'}
    assert len(set(lr.CASES)) == len(lr.CASES) == len({repr(c) for c in lr.CASES})


def test_the_cases_sit_on_the_switches_they_are_listed_for():
    by = {repr(c): c for c in lr.CASES}
    # every KS with three padded components and with none, on fewer than, exactly and more than 8 nodes
    ks_rows = lr.CASES[:16]
    assert [c.K for c in ks_rows] == [k for ks in range(1, 9) for k in (4 * ks - 3, 4 * ks)]
    assert {c.N for c in ks_rows} == {7, 8, 9, 23} and {c.D for c in ks_rows} == set(range(1, 9))
    assert {c.T for c in ks_rows} == {3, 4, 5}
    # the LDS limit of the matrix-core path: T = 13 is the largest at (K, D) = (32, 2)
    assert lr.lm_lds_bytes(13, 32, 2) <= lr.MFMA_LDS_MAX < lr.lm_lds_bytes(14, 32, 2)
    assert lr.form(13, 32, 2) == 'mfma KS=8' and lr.form(14, 32, 2) == 'wave WLDS=0'
    # staging of the transition matrices past the prefetched passes, and within the first
    assert 13 * 32 * lr.lm_wstride(32) > lr.LM_WPRE * lr.LM_THREADS
    assert all(c.T * c.K * lr.lm_wstride(c.K) < lr.LM_THREADS for c in ks_rows if c.K <= 5)
    # the wavefront kernel: passes of 64 uniforms, trips of 8 components, the largest table, its attribute
    assert by['129-10-1-3'].T > 2 * 64 and by['129-10-1-3'].K < 8
    assert 33 % 8 and 40 % 8 == 0
    tables, w = lr.wave_lds_bytes(20, 64)
    assert tables == lr.WAVE_TABLES_MAX > 64 * 1024 and lr.wave_lds_bytes(21, 64)[0] > lr.WAVE_TABLES_MAX
    assert lr.REFUSED.dims == (21, 11, 2, 64)
    # k_label_counts: a third pass; more counters than threads
    assert by['5-2100-2-3'].N > lr.LC_PRE * lr.LC_THREADS
    assert 64 * 64 + 64 > lr.LC_THREADS
    # the label sums: a second and a third trip
    assert [N > lr.HDP_NU * lr.HDP_THREADS for _, N, _, _ in lr.SUMS_CASES] == [True, True]
    assert lr.SUMS_CASES[1][1] > 2 * lr.HDP_NU * lr.HDP_THREADS


@pytest.mark.parametrize('case', lr.CASES, ids=repr)
def test_replica_draws_the_oracles_labels(case):
    (X, mu, sg, w), _ = lr.update(case)
    for it in lr.ITERS:
        ref = lr.reference(case, it)
        zo, no, nko = orc.sample_labels_block_philox(X, mu, sg, lr.LMBDA, w, lr.SEED, lr.CHAIN, it)
        np.testing.assert_array_equal(ref.z, zo)
        np.testing.assert_array_equal(ref.n, no)
        np.testing.assert_array_equal(ref.nk, nko)
        assert ref.nk.sum() == case.T * case.N and lr.update(case)[1].explain(zo, it) is None


@pytest.mark.parametrize('case', lr.CASES, ids=repr)
def test_replica_table_is_the_oracles(case):
    """to 1e-12 relative wherever the float64 table is a normal number with room to spare; below that both are
    below 1e-290"""
    (X, mu, sg, w), up = lr.update(case)
    L = np.exp(up.logL)
    for i in sorted({0, case.N // 2, case.N - 1} | set(case.far)):
        want = orc.compute_gaussian_likelihood(X[:, i], mu, sg, lr.LMBDA, normalize=False)
        big = want >= 1e-290
        np.testing.assert_allclose(L[:, i][big].astype(np.float64), want[big], rtol=1e-12, atol=0)
        assert (L[:, i][~big] < 1e-289).all()
        for normalize in (False, True):
            ref, bound = lr.table(X[:, i], mu, sg, lr.LMBDA, normalize)
            got = orc.compute_gaussian_likelihood(X[:, i], mu, sg, lr.LMBDA, normalize=normalize)
            assert (np.abs(got.astype(lr.LD) - ref) <= bound).all()     # the oracle makes the device's roundings


@pytest.mark.parametrize('case', lr.CASES, ids=repr)
def test_no_draw_is_a_tie_and_the_device_error_is_far_below_the_margin(case):
    worst_margin, worst_bound = np.inf, 0.0
    for it in lr.ITERS:
        ref = lr.reference(case, it)
        worst_margin = min(worst_margin, float(ref.margin.min()))
        worst_bound = max(worst_bound, float(ref.bound.max()))
    print('%r %s: %d draws, min margin %.3e, bound %.3e, max |log L| %.1f'
          % (case, case.want, 2 * case.T * case.N, worst_margin, worst_bound, ref.max_abs_logL))
    assert worst_margin >= MIN_MARGIN
    assert worst_bound <= MAX_BOUND


@pytest.mark.parametrize('case', [c for c in lr.CASES if c.far], ids=repr)
def test_far_nodes_sit_near_the_bottom_of_the_double_range(case):
    (X, mu, sg, w), _ = lr.update(case)
    with np.errstate(divide='ignore'):
        top = np.array([np.log(orc.compute_gaussian_likelihood(X[:, i], mu, sg, lr.LMBDA, normalize=False)).max(1)
                        for i in range(case.N)])
    assert top.min() <= lr.FAR_HIGH and top.min() >= lr.FAR_LOW, top.min()
    assert (top[list(case.far)].min(axis=1) <= lr.FAR_HIGH).all()


def test_the_other_cases_stay_in_the_middle_of_the_range():
    assert max(lr.reference(c, 1).max_abs_logL for c in lr.CASES if not c.far) < 700


def test_explain_names_the_first_draw_that_leaves_the_reference():
    case = lr.CASES[4]
    up = lr.update(case)[1]
    z = lr.reference(case, 1).z.copy()
    t, node = 1, 3
    z[t, node] = (z[t, node] + 1) % case.K
    got = up.explain(z, 1)
    assert got[:4] == (node, t, int(z[t, node]), int(lr.reference(case, 1).z[t, node]))
    assert got[4] == float(lr.reference(case, 1).margin[t, node]) and got[5] >= 1


@pytest.mark.parametrize('dims', lr.SUMS_CASES, ids=str)
@pytest.mark.parametrize('variant', ['random', 'empty', 'one'])
def test_label_sums_replica_is_the_oracles(dims, variant):
    T, N, D, K = dims
    X, z, mu, sigma, w = lr.sums_inputs(T, N, D, K, variant)
    lm, a, b = 0.83, 2.0, 1.3
    ref, sums = NumpyLabelSums(X, z, K), lr.LabelSums(X, z, K)
    want = [ref.mean(lm).reshape(T, K, D), ref.residual(mu, lm), ref.lam(mu, sigma), ref.logp(mu, sigma, lm, w, a, b)]
    got = [sums.stage(0, lmbda=lm), sums.stage(1, mu=mu, lmbda=lm), sums.stage(2, mu=mu, sigma=sigma),
           sums.stage(3, mu=mu, sigma=sigma, lmbda=lm, w=w, a=a, b=b)]
    for (g, bound), wnt in zip(got, want):
        np.testing.assert_allclose(g.astype(np.float64), wnt, rtol=1e-12, atol=1e-12)
        assert (bound >= 0).all() and (bound <= 1e-12 + 1e-12 * np.abs(g)).all()
        empty = np.zeros((T, K), dtype=bool)
        for t in range(T):
            empty[t] = np.bincount(z[t], minlength=K) == 0
        assert (g[empty] == 0).all() and (bound[empty] == 0).all()
    assert variant == 'random' or (np.bincount(z.ravel(), minlength=K) == 0).any()
