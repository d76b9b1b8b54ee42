"""CPU-side checks of the missing-dyad sampling (csrc/kernels_missing.hpp, dynetlsm_amd/model_selection.py):
the held-out split, the validation that happens before any device call, the agreement of the header, the
integration document and the binding on the new entry points, and the code object of the new kernel."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

ENTRY_POINTS = {'dlsm_set_missing': 3, 'dlsm_impute_missing': 3, 'dlsm_missing_sampling': 3,
                'dlsm_get_missing': 4, 'dlsm_reset_missing_sums': 1}


def _network(T, N, seed, directed):
    rng = np.random.RandomState(seed)
    Y = (rng.rand(T, N, N) < 0.2).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    idx = np.arange(N)
    Y[:, idx, idx] = 0.0
    return Y


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('T,N,share', [(1, 7, 0.2), (3, 20, 0.1), (4, 33, 0.15)])
def test_train_test_split(T, N, share, directed):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.metrics import missing_index
    Y = _network(T, N, 5, directed)
    Yt, index = train_test_split(Y, test_size=share, random_state=11, is_directed=directed)
    n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
    per_slice = int(round(share * n_dyads))
    assert index.shape == (T * per_slice, 3) and index.dtype == np.int64
    assert np.array_equal(np.bincount(index[:, 0], minlength=T), np.full(T, per_slice))
    # the coded entries are exactly the listed dyads, the rest is untouched
    M = Yt == -1
    assert np.array_equal(missing_index(Yt, directed), index)
    assert M.sum() == index.shape[0] * (1 if directed else 2)
    assert np.array_equal(Yt[~M], Y[~M])
    d = np.arange(N)
    assert not M[:, d, d].any() and np.array_equal(Yt[:, d, d], Y[:, d, d])
    if directed:
        assert (index[:, 1] != index[:, 2]).all()
    else:
        assert np.array_equal(Yt, Yt.swapaxes(1, 2)) and (index[:, 1] < index[:, 2]).all()
    # reproducible by seed, different under another seed, and the caller's array is not written
    Yt2, index2 = train_test_split(Y, test_size=share, random_state=11, is_directed=directed)
    assert np.array_equal(Yt, Yt2) and np.array_equal(index, index2)
    _, index3 = train_test_split(Y, test_size=share, random_state=12, is_directed=directed)
    assert not np.array_equal(index, index3)
    assert not (Y == -1).any()
    with pytest.raises(ValueError, match='test_size'):
        train_test_split(Y, test_size=1.5)
    with pytest.raises(ValueError, match='shape'):
        train_test_split(Y[0])


def test_missing_list_is_checked_before_any_device_call():
    from dynetlsm_amd.engine import check_missing_index
    from dynetlsm_amd._lib import UNDIRECTED, DIRECTED, DIRECTED_CASE_CONTROL
    ok = np.array([[0, 1, 2], [1, 0, 4], [1, 3, 4]])
    got = check_missing_index(ok, 2, 5, UNDIRECTED)
    assert got.dtype == np.int32 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, ok)
    assert check_missing_index([], 2, 5, UNDIRECTED).shape == (0, 3)
    assert np.array_equal(check_missing_index([[0, 4, 1]], 2, 5, DIRECTED), [[0, 4, 1]])
    for bad, model, msg in (([[2, 0, 1]], UNDIRECTED, 'outside'), ([[0, 0, 5]], UNDIRECTED, 'outside'),
                            ([[0, -1, 2]], DIRECTED, 'outside'), ([[0, 3, 1]], UNDIRECTED, 'i < j'),
                            ([[0, 2, 2]], DIRECTED, 'diagonal'), ([[0, 1, 2], [0, 1, 2]], UNDIRECTED, 'twice'),
                            ([[0, 1, 2]], DIRECTED_CASE_CONTROL, 'case-control'),
                            ([0, 1, 2], UNDIRECTED, r'\(n, 3\)'), ([[0.0, 1.0, 2.0]], UNDIRECTED, 'integer')):
        with pytest.raises(ValueError, match=msg):
            check_missing_index(bad, 2, 5, model)


def test_facades_refuse_case_control_sampling_by_name_before_any_device_call():
    import dynetlsm_amd as da
    Y = _network(2, 8, 1, True)
    Y[0, 1, 2] = -1
    for est in (da.DynamicNetworkLSM(is_directed=True, n_control=3, sample_missing=True, n_iter=3, tune=None,
                                     burn=None),
                da.DynamicNetworkHDPLPCM(is_directed=True, n_control=3, sample_missing=True, n_iter=3, tune=None,
                                         burn=None),
                da.DynamicNetworkLPCM(is_directed=True, n_control=3, sample_missing=True, n_iter=3, tune=None,
                                      burn=None)):
        with pytest.raises(ValueError, match='sample_missing=True is not supported with n_control'):
            est.fit(Y)
    with pytest.raises(ValueError, match="hdp_loop='device'"):
        da.DynamicNetworkHDPLPCM(hdp_loop='device', sample_missing=True, n_iter=3, tune=None, burn=None).fit(Y)
    # the keyword defaults to off
    for cls in (da.DynamicNetworkLSM, da.DynamicNetworkHDPLPCM, da.DynamicNetworkLPCM):
        assert cls().sample_missing is False


def test_heldout_scores_on_a_stub():
    from dynetlsm_amd.metrics import heldout_scores

    class Fitted(object):
        missing_index_ = np.array([[0, 0, 1], [0, 1, 2], [1, 0, 2], [1, 1, 2]])
        missing_probas_ = np.array([0.9, 0.2, 0.6, 0.4])
    Y = np.zeros((2, 3, 3))
    Y[0, 0, 1] = Y[1, 0, 2] = 1
    s = heldout_scores(Fitted(), Y)
    assert s['n'] == 4 and s['auc'] == 1.0
    assert np.isclose(s['log_loss'], -np.mean(np.log([0.9, 0.8, 0.6, 0.6])))
    with pytest.raises(ValueError, match='sample_missing=True'):
        heldout_scores(object(), Y)
    Y[0, 1, 2] = -1
    with pytest.raises(ValueError, match='0 / 1'):
        heldout_scores(Fitted(), Y)


def test_replica_counter_layout():
    """A guard on the test helper only (the kernel is held to it in tests/test_gpu_missing.py): the replica's
    uniforms are a function of (seed, chain, iteration, t, unordered pair): both arcs of a pair share a counter
    and take its two halves; undirected pairs take the first"""
    from oracle import oracle as orc
    import missing_ref as mr
    idx = np.array([[300, 2, 9], [300, 9, 2], [0, 2, 9], [1, 2, 9]])
    u = mr.uniforms(orc.philox4x32, 77, 3, 5, idx, True)
    r = orc.philox4x32(77, 2 | ((300 & 255) << 24), 9 | ((300 >> 8) << 24), 5, (3 << 8) | 8)
    from gof_stats import u53
    assert u[0] == u53(r[0], r[1]) and u[1] == u53(r[2], r[3])
    assert len(set(u.tolist())) == 4
    uu = mr.uniforms(orc.philox4x32, 77, 3, 5, idx[[0, 2]], False)
    assert uu[0] == u[0] and uu[1] == u[2]
    assert mr.uniforms(orc.philox4x32, 77, 4, 5, idx[:1], False)[0] != u[0]
    assert mr.uniforms(orc.philox4x32, 77, 3, 6, idx[:1], False)[0] != u[0]


def _header():
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    return src, re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_header_document_and_binding_agree_on_the_entry_points():
    import ctypes
    from dynetlsm_amd import _lib
    raw, src = _header()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^;{]*?)\)\s*;' % name, src, flags=re.S)
        assert m, 'include/dynetlsm_hip.h does not declare %s' % name
        args = [a.strip() for a in m.group(1).split(',')]
        assert len(args) == arity and args[0].startswith('dlsm_chain')
        assert len(_lib.SIGNATURES[name][1]) == arity
        assert re.search(r'\b%s\(' % name, doc), 'INTEGRATION.md does not show %s' % name
    # each declaration follows a comment that cites the reference lines it stands for
    for name in ENTRY_POINTS:
        before = raw[:raw.index('int %s(' % name)]
        comment = before[before.rindex('/*'):]
        assert re.search(r'(lsm|hdp_lpcm|imputer)\.py:\d+', comment), name
    from dynetlsm_amd.build import build
    lib = ctypes.CDLL(build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    from dynetlsm_amd.engine import Chain
    for method in ('set_missing', 'impute_missing', 'missing_sampling', 'get_missing', 'reset_missing_sums'):
        assert callable(getattr(Chain, method))


def test_new_sources_hold_no_scalar_memory_write():
    words = ['s_' + w for w in ('store_dword', 'buffer_store', 'scratch_store', 'atomic_', 'buffer_atomic',
                                'dcache_wb', 'dcache_discard')]
    for f in ('kernels_missing.hpp', 'capi_missing.hpp'):
        txt = open(os.path.join(ROOT, 'dynetlsm_amd', 'csrc', f)).read().lower()
        for w in words:
            assert w not in txt, (f, w)
        assert 'asm' not in txt, f


def test_every_instantiation_of_the_kernel_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_impute_missing<%d>' % d for d in range(1, 9)]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_impute_missing')) == sorted(names)
