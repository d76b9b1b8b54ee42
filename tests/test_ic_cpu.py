"""Information criteria without a GPU: the host restatement (tests/ic_ref.py) against the C oracle's full
log-likelihood, the arithmetic of ICResult and compare_information_criteria against brute force, the
argument checks that come before any device call, the C-ABI declaration and its binding, and the code
object of the new kernels (no scratch memory in any instantiation)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import ic_ref  # noqa: E402
from conftest import LIK_TAGS  # noqa: E402

RTOL = 1e-12            # the golden tests' tolerance


def _oracle_loglik(Y, X, ic, radii, directed):
    from oracle import oracle as orc
    if directed:
        return orc.dynamic_network_loglikelihood_directed(Y, X, ic[0], ic[1], radii)
    return orc.dynamic_network_loglikelihood_undirected(Y, X, ic[0])


@pytest.mark.parametrize('tag', LIK_TAGS)
def test_reference_sample_loglik_equals_the_oracle_on_the_golden_inputs(golden_lik, tag):
    g = golden_lik
    X, Yd, Yu, radii = g[tag + '_X'], g[tag + '_Yd'], g[tag + '_Yu'], g[tag + '_radii']
    b, b_in, b_out = g[tag + '_b']
    # the oracle is pinned to the reference by these fixtures (test_oracle_golden.py)
    got = ic_ref.sample_loglik(Yu, X[None], np.array([[b, 0.0]]), None, False)
    want = _oracle_loglik(Yu, X, [b], None, False)
    assert abs(got.sum() - want) <= RTOL * abs(want), (got.sum(), want)
    got = ic_ref.sample_loglik(Yd, X[None], np.array([[b_in, b_out]]), radii[None], True)
    want = _oracle_loglik(Yd, X, [b_in, b_out], radii, True)
    assert abs(got.sum() - want) <= RTOL * abs(want), (got.sum(), want)


def _random_case(rng, S, T, N, D, directed, density=0.2):
    Xs = rng.randn(S, T, N, D) * (1.5 / np.sqrt(D))
    ic = np.stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    idx = np.arange(N)
    Y[:, idx, idx] = 0
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.transpose(0, 2, 1)
    return Y, Xs, ic, radii


@pytest.mark.parametrize('D', [1, 2, 5, 8])
@pytest.mark.parametrize('directed', [False, True])
def test_reference_sample_loglik_equals_the_oracle_on_random_inputs(D, directed):
    rng = np.random.RandomState(100 + D + 10 * directed)
    S, T, N = 3, 2, 23
    Y, Xs, ic, radii = _random_case(rng, S, T, N, D, directed)
    got = ic_ref.accumulate(Y, Xs, ic, radii, directed, rows=7)[1]
    for s in range(S):
        want = _oracle_loglik(Y, Xs[s], ic[s], radii[s] if directed else None, directed)
        assert abs(got[s].sum() - want) <= RTOL * abs(want), (s, got[s].sum(), want)
    # the time steps split the total
    one = _oracle_loglik(Y[:1], Xs[0][:1], ic[0], radii[0] if directed else None, directed)
    assert abs(got[0, 0] - one) <= RTOL * abs(one)


@pytest.mark.parametrize('directed', [False, True])
def test_result_arithmetic_against_brute_force(directed):
    from dynetlsm_amd.ic import ICResult
    rng = np.random.RandomState(7 + directed)
    S, T, N, D = 6, 3, 17, 2
    Y, Xs, ic, radii = _random_case(rng, S, T, N, D, directed)
    totals, sl, pw = ic_ref.accumulate(Y, Xs, ic, radii, directed)
    hat = ic_ref.accumulate(Y, Xs[:1], ic[:1], radii[:1] if directed else None, directed)[1][0]
    res = ICResult(np.arange(S), totals, sl, hat, directed, N, pw)
    want = ic_ref.criteria(pw, sl, hat, directed)
    assert res.n_dyads == want['n_dyads'] == T * (N * (N - 1) if directed else N * (N - 1) // 2)
    assert res.n_samples == S
    for name in ('lppd', 'p_waic', 'elpd_waic', 'waic', 'se_elpd', 'd_bar', 'd_hat', 'p_d', 'dic', 'p_v', 'dic_v'):
        np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-9, err_msg=name)
    for name in ('lppd_t', 'p_waic_t', 'elpd_waic_t', 'waic_t', 'se_elpd_t', 'd_bar_t', 'd_hat_t'):
        np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-9, err_msg=name)
    assert res.waic == -2 * res.elpd_waic and res.dic == res.d_bar + res.p_d
    for name in ('lppd', 'p_waic', 'elpd_waic', 'waic', 'd_bar', 'd_hat', 'p_d', 'dic'):
        np.testing.assert_allclose(getattr(res, name + '_t').sum(), getattr(res, name), rtol=1e-12, err_msg=name)
    assert res.n_dyads_t.sum() == res.n_dyads
    assert res.p_waic > 0 and res.se_elpd > 0
    np.testing.assert_array_equal(res.pointwise_lppd, pw[..., 0])
    np.testing.assert_array_equal(res.pointwise_p_waic, pw[..., 1])
    text = res.summary()
    assert 'waic' in text and 'dic' in text and repr(res) == text
    # one sample: no variance anywhere
    one = ICResult(np.arange(1), *ic_ref.accumulate(Y, Xs[:1], ic[:1], radii[:1] if directed else None,
                                                    directed)[:2], hat, directed, N)
    assert one.p_waic == 0.0 and one.p_v == 0.0 and one.pointwise_lppd is None
    np.testing.assert_allclose(one.lppd, one.sample_loglik.sum(), rtol=1e-12)


def test_compare_against_brute_force_and_its_errors():
    from dynetlsm_amd.ic import ICResult, compare_information_criteria
    rng = np.random.RandomState(11)
    S, T, N = 5, 2, 15
    Y, Xa, ica, _ = _random_case(rng, S, T, N, 2, False)
    _, Xb, icb, rb = _random_case(rng, S, T, N, 1, True)

    def result(Yn, Xs, ic, radii, directed, pointwise=True):
        totals, sl, pw = ic_ref.accumulate(Yn, Xs, ic, radii, directed)
        return ICResult(np.arange(S), totals, sl, sl[0], directed, Yn.shape[1], pw if pointwise else None), pw

    a, pwa = result(Y, Xa, ica, None, False)
    b, pwb = result(Y, Xb[..., :1] * 0.7, icb, None, False)
    diff, se = compare_information_criteria(a, b)
    wd, ws = ic_ref.compare(pwa, pwb, False)
    np.testing.assert_allclose([diff, se], [wd, ws], rtol=1e-10)
    np.testing.assert_allclose(diff, a.elpd_waic - b.elpd_waic, rtol=1e-9)
    back = compare_information_criteria(b, a)
    np.testing.assert_allclose([back[0], back[1]], [-diff, se], rtol=1e-12)
    assert se > 0
    with pytest.raises(ValueError, match='pointwise'):
        compare_information_criteria(a, result(Y, Xa, ica, None, False, pointwise=False)[0])
    with pytest.raises(ValueError, match='directed'):
        compare_information_criteria(a, result(Y, Xb, icb, rb, True)[0])
    Ys, Xs_, ics, _ = _random_case(rng, S, T, N - 1, 2, False)
    with pytest.raises(ValueError, match='different networks'):
        compare_information_criteria(a, result(Ys, Xs_, ics, None, False)[0])
    with pytest.raises(ValueError):
        compare_information_criteria(a, None)


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib

    def boom():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    with pytest.raises(ValueError, match='not fit'):
        da.information_criteria(da.DynamicNetworkLSM())

    class Fitted(object):                      # the attributes the function reads, nothing else
        is_directed = False
        thin = None
        n_burn_ = 4
        Y_fit_ = np.zeros((2, 5, 5))
        Xs_ = np.zeros((10, 2, 5, 2))
        intercepts_ = np.zeros((10, 1))
        X_ = np.zeros((2, 5, 2))
        intercept_ = np.zeros(1)
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.information_criteria(Fitted(), n_samples=bad)
    with pytest.raises(AssertionError, match='the library was loaded'):
        da.information_criteria(Fitted(), n_samples=6)


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    from dynetlsm_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_ic_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_ic_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 9 and args[0].startswith('dlsm_chain') and args[-1].endswith('pointwise')
    res, argtypes = _lib.SIGNATURES['dlsm_ic_accumulate']
    assert len(argtypes) == len(args)
    import ctypes
    from dynetlsm_amd.build import build
    assert hasattr(ctypes.CDLL(build()), 'dlsm_ic_accumulate')


def test_every_instantiation_of_the_kernels_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_ic_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    names += ['k_ic_reduce_totals', 'k_ic_reduce_samples']
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        # a 256-thread workgroup must fit a SIMD's 512 registers per lane
        assert md[name]['vgpr'] <= 512, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_ic_')) == sorted(names)
