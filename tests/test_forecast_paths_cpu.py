"""Multi-step forecasts without a GPU: the law of the numpy replica tests/forecast_paths_ref.py (what the
device test compares against), the counter layout, the argument checks of the facade and the code object of
the new kernels (no scratch memory in any instantiation)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import forecast_paths_ref as fpr  # noqa: E402


@pytest.fixture(scope='module')
def philox():
    from oracle import oracle as orc
    return orc.philox4x32


def test_label_frequencies_follow_the_transition_rows(philox):
    """20 000 nodes per starting label: the frequencies of the next label are within 5 standard errors of the
    normalised row (raw rows: they do not sum to 1)"""
    K, per = 4, 20000
    w = np.array([[3.0, 1.0, 0.0, 4.0], [0.2, 0.2, 0.2, 0.2], [0.0, 0.0, 5.0, 0.0], [1.0, 2.0, 3.0, 4.0]])
    z0 = np.repeat(np.arange(K), per)[None]
    N = K * per
    _, L = fpr.paths(philox, 77, 3, np.zeros((1, N, 1)), 2, z0=z0, trans=w[None], mu=np.zeros((1, K, 1)),
                     sigma=np.ones((1, K)), lmbda=np.array([0.5]))
    p = w / w.sum(axis=1, keepdims=True)
    for g in range(K):
        f = np.bincount(L[0, 0, z0[0] == g], minlength=K) / per
        se = np.sqrt(p[g] * (1 - p[g]) / per)
        assert (np.abs(f - p[g]) <= 5 * se + 1e-12).all(), (g, f, p[g])
        assert (f[p[g] == 0] == 0).all()
    # step 2 from the labels of step 1: the two-step law
    f2 = np.bincount(L[0, 1], minlength=K) / N
    want = (np.full(K, 0.25) @ p) @ p
    assert (np.abs(f2 - want) <= 5 * np.sqrt(want * (1 - want) / N) + 1e-12).all(), (f2, want)


def test_label_rule_edges():
    rows = np.array([[1.0, 1.0, 2.0], [0.0, 0.0, 3.0], [2.0, 0.0, 0.0]])
    # u = 1 is the largest uniform (u53 is in (0, 1]): the last component with weight
    assert fpr.draw_labels(np.array([1.0, 1.0, 1.0]), rows).tolist() == [2, 2, 0]
    assert fpr.draw_labels(np.array([2.0 ** -53] * 3), rows).tolist() == [0, 2, 0]
    assert fpr.draw_labels(np.array([0.25, 0.5, 0.50000001]), rows[[0, 0, 0]]).tolist() == [0, 1, 2]
    # K = 1
    assert fpr.draw_labels(np.array([0.3, 1.0]), np.array([[0.7], [0.1]])).tolist() == [0, 0]


def test_position_moments_follow_the_random_walk(philox):
    """x_H - x_0 is N(0, H sigma_sq) per coordinate, independent across coordinates and steps"""
    N, D, H, s2 = 40000, 3, 4, 0.3
    X0 = np.random.RandomState(0).randn(1, N, D)
    P, L = fpr.paths(philox, 5, 0, X0, H, sigma_sq=s2)
    assert L is None
    inc = np.diff(np.concatenate([X0[:, None], P], axis=1), axis=1)[0]       # (H, N, D)
    se = np.sqrt(s2 / N)
    assert (np.abs(inc.mean(axis=1)) <= 5 * se).all()
    assert (np.abs(inc.var(axis=1) - s2) <= 5 * s2 * np.sqrt(2.0 / N)).all()
    flat = inc.transpose(1, 0, 2).reshape(N, H * D)
    C = np.corrcoef(flat.T)
    assert (np.abs(C - np.eye(H * D)) <= 5 / np.sqrt(N)).all()


def test_position_moments_follow_the_mixture(philox):
    """one step from x_0 = 0 with one-hot rows: x_1 ~ N(lmbda mu_g, sigma_g) - sigma is a variance"""
    K, per, D, lm = 3, 30000, 2, 0.7
    mu = np.array([[1.0, -2.0], [0.0, 4.0], [-3.0, 0.5]])
    sigma = np.array([0.04, 1.0, 2.25])
    z0 = np.repeat(np.arange(K), per)[None]
    P, L = fpr.paths(philox, 9, 11, np.zeros((1, K * per, D)), 1, z0=z0, trans=np.eye(K)[None], mu=mu[None],
                     sigma=sigma[None], lmbda=np.array([lm]))
    assert np.array_equal(L[0, 0], z0[0])
    for g in range(K):
        x = P[0, 0, z0[0] == g]
        assert (np.abs(x.mean(axis=0) - lm * mu[g]) <= 5 * np.sqrt(sigma[g] / per)).all()
        assert (np.abs(x.var(axis=0) - sigma[g]) <= 5 * sigma[g] * np.sqrt(2.0 / per)).all()


def test_counters_never_collide():
    """(node, h, draw, sample) -> counter words is injective for D <= 8: h < 2^16 and draw <= 4 share word 1
    without overlap, the stream word is the new stream 9"""
    seen = set()
    hs = [1, 2, 255, 256, 65535]
    for i in (0, 1, 70000):
        for h in hs:
            for draw in range(0, 1 + 8 // 2):
                for q in (0, 1, 2 ** 32 - 1):
                    c = fpr.counter(i, h, draw, q)
                    assert c not in seen
                    seen.add(c)
                    assert c[1] & 0xFFFF == h and c[1] >> 16 == draw and c[3] == 9 and c[1] < 2 ** 32
    assert len(seen) == 3 * len(hs) * 5 * 3
    src = open(os.path.join(os.path.dirname(HERE), 'dynetlsm_amd', 'csrc', 'kernels_forecast_paths.hpp')).read()
    assert 'STREAM_FORECAST = 9' in src
    # streams 0..8 are taken by the other kernels
    import re
    csrc = os.path.join(os.path.dirname(HERE), 'dynetlsm_amd', 'csrc')
    taken = {}
    for name in os.listdir(csrc):
        for m in re.finditer(r'\b(STREAM_[A-Z_]+) = (\d+)', open(os.path.join(csrc, name), errors='replace').read()):
            taken[m.group(1)] = int(m.group(2))
    assert sorted(taken.values()) == list(range(10)) and taken['STREAM_FORECAST'] == 9


class Fitted(object):
    """the attributes of an undirected LSM fit that forecast() reads before any device call"""
    is_directed = False
    n_burn_ = 4
    random_state = 0
    sigma_sq = 0.1
    Y_fit_ = np.zeros((2, 5, 5))
    intercepts_ = np.zeros((10, 1))
    Xs_ = np.zeros((10, 2, 5, 2))
    X_ = np.zeros((2, 5, 2))
    intercept_ = np.zeros(1)


def test_the_facade_rejects_bad_arguments():
    import dynetlsm_amd as da
    for bad in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match='horizon'):
            da.forecast(Fitted(), horizon=bad)
    for est in (da.DynamicNetworkLSM(), da.DynamicNetworkHDPLPCM(), da.DynamicNetworkLPCM()):
        with pytest.raises(ValueError, match='not fit'):
            da.forecast(est)
        with pytest.raises(ValueError, match='not fit'):
            est.forecast(horizon=2)
    with pytest.raises(ValueError, match='estimate'):
        da.forecast(Fitted(), estimate='posterior_mean')
    with pytest.raises(ValueError, match='n_samples'):
        da.forecast(Fitted(), estimate='map')
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match='positive integer'):
            da.forecast(Fitted(), estimate='map', n_samples=bad)
        with pytest.raises(ValueError, match='positive integer'):
            da.forecast(Fitted(), n_samples=bad)
    with pytest.raises(ValueError, match='exceeds the 6 kept samples'):
        da.forecast(Fitted(), n_samples=7)


def test_score_needs_paths_and_a_network_of_the_forecast_shape():
    import dynetlsm_amd as da
    H, N, D, S = 3, 5, 2, 4
    bare = da.ForecastResult(np.zeros((H, N, N)), np.arange(S), False)
    assert bare.horizon == H and bare.n_nodes == N and bare.paths is None and bare.labels is None
    with pytest.raises(ValueError, match='keep_paths=True'):
        bare.score(np.zeros((H, N, N)))
    kept = da.ForecastResult(np.zeros((H, N, N)), np.arange(S), False, paths=np.zeros((S, H, N, D)),
                             intercepts=np.zeros((S, 2)))
    for shape in ((H + 1, N, N), (0, N, N), (H, N, N + 1), (N, N), (H, N + 1, N + 1)):
        with pytest.raises(ValueError, match='Y_future has shape'):
            kept.score(np.zeros(shape))
    text = bare.summary()
    assert 'horizon 3' in text and 'h=3' in text and '4 posterior samples' in text


def test_header_binding_and_library_agree_on_the_entry_point():
    import ctypes
    import re
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build
    root = os.path.dirname(HERE)
    src = open(os.path.join(root, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_forecast_paths\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_forecast_paths'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 19 and args[4].endswith('z0') and args[-3].endswith('probas') and args[-1].endswith('labels')
    assert len(_lib.SIGNATURES['dlsm_forecast_paths'][1]) == len(args)
    assert hasattr(ctypes.CDLL(build()), 'dlsm_forecast_paths')


def test_every_instantiation_of_the_kernels_is_free_of_scratch_memory():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'profiles'))
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_forecast_paths_draw<%d>' % d for d in range(1, 9)]
    names += ['k_forecast_paths_mean<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        # three 256-thread workgroups per CU at least: one wavefront of each per SIMD, 512 // 3 registers per lane
        assert md[name]['vgpr'] <= 170, (name, md[name])
        # ... and the LDS of each within a quarter of the CU's 160 KB
        assert md[name]['lds'] <= 40 * 1024, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_forecast_paths_')) == sorted(names)


def test_the_package_function_does_not_hide_the_one_step_module():
    """``da.forecast(...)`` is callable and ``from dynetlsm_amd import forecast as fc`` still reaches the one-step
    functions (tests/test_gpu_forecast.py imports them that way)"""
    import importlib
    import dynetlsm_amd as da
    from dynetlsm_amd import forecast as fc
    assert callable(da.forecast) and da.forecast is fc is importlib.import_module('dynetlsm_amd.forecast')
    for name in ('forecast_probas_map', 'forecast_probas_plugin', 'forecast_probas_marginalized', 'forecast_probas',
                 'forecast_probas_pp', 'lpcm_forecast_probas'):
        assert callable(getattr(fc, name)), name
    from dynetlsm_amd.forecast_paths import forecast
    with pytest.raises(ValueError, match='not fit'):
        forecast(da.DynamicNetworkLSM())
