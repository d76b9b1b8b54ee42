"""PSIS-LOO without a GPU: the shared fit header (csrc/psis_tail.hpp, compiled into tests/cpp/check_psis_tail.cpp
as it is and under ASan / UBSan, a stand-alone program) against the host restatement tests/loo_ref.py, loo_ref
against a dyad worked out by hand, the arithmetic of LooResult and compare_loo against brute force, the C-ABI
declaration and its binding, and the code object of the new kernel (no scratch memory in any instantiation).

Tolerance of the header against loo_ref: 16 eps + 4 ulp, eps the reference's own error on that input - the larger
of max |float64 - longdouble| and max |ref(l) - ref(l')|, l' every value moved by +-4 ulp (the fit amplifies input
rounding).  A tail is left out of the value comparison only if the float64 and the longdouble evaluation of the
reference disagree on fitted / unfitted (at most 1 % of them)."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import loo_ref  # noqa: E402

CSRC = os.path.join(ROOT, 'dynetlsm_amd', 'csrc')
SOURCE = os.path.join(HERE, 'cpp', 'check_psis_tail.cpp')


def _compile(tmp_path, name, extra):
    if shutil.which('g++') is None:
        pytest.skip('g++ not installed')
    exe = str(tmp_path / name)
    b = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-I', CSRC] + extra + [SOURCE, '-o', exe, '-lm'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode()
    return exe


def _run(exe, args):
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert 'runtime error' not in out and 'Sanitizer' not in out, out
    return out


def _tails():
    """{M: (n, M + 1) sorted tails}: random ones at several spreads, constant ones, and ones with ties at the
    cutoff (zeros in x): one, up to q - 1 (xstar still positive) and beyond (xstar == 0: unfitted)"""
    rng = np.random.RandomState(11)
    out = {}
    for S, M in ((25, 5), (100, 20), (2000, 135)):
        assert loo_ref.tail_length(S) == M
        rows = []
        for scale in (0.05, 1.0, 3.0, 8.0):
            for _ in range(6):
                rows.append(np.sort(-np.abs(rng.standard_t(3, S)) * scale - rng.rand())[:M + 1])
        rows.append(np.full(M + 1, -0.7))                          # constant
        rows.append(np.full(M + 1, -812.25))
        base = np.sort(-rng.gamma(2.0, 1.0, S))[:M + 1]
        q = int(np.floor(M / 4 + 0.5))
        for ties in (1, max(1, q - 1), q, M - 1):                  # slots M - ties .. M - 1 equal the cutoff
            t = base.copy()
            t[M - ties:M] = t[M]
            rows.append(t)
        spread = base.copy()                                       # a spread below DBL_EPSILON / 100 at |l| of 1e-3
        spread[:] = -1e-3
        spread[1:] = np.nextafter(-1e-3, 0)
        rows.append(spread)
        out[M] = np.array(rows)
    return out


def _reference(tails):
    """(k, sigma, fitted, lw) of float64, longdouble and the perturbed tails"""
    rng = np.random.RandomState(5)
    pert = np.sort(tails + (rng.randint(0, 2, tails.shape) * 2 - 1) * 4 * np.spacing(np.abs(tails)), axis=1)
    return (loo_ref.fit_tails(tails.astype(np.float64)), loo_ref.fit_tails(tails.astype(np.longdouble)),
            loo_ref.fit_tails(pert))


def _tol(a64, ald, apert, pert_fitted):
    a64 = np.asarray(a64, dtype=np.float64)
    eps = max(float(np.max(np.abs(a64.astype(np.longdouble) - ald))),
              float(np.max(np.abs(a64 - apert)[pert_fitted])))
    return 16.0 * eps + 4.0 * np.spacing(np.abs(a64)), eps


def _check_program(exe, tmp_path):
    tails = _tails()
    path = str(tmp_path / 'tails.txt')
    with open(path, 'w') as f:
        f.write('%d\n' % sum(len(t) for t in tails.values()))
        for M, rows in tails.items():
            for r in rows:
                f.write('%d %s\n' % (M, ' '.join(float(v).hex() for v in r)))
    lines = _run(exe, [path]).strip().split('\n')
    assert len(lines) == sum(len(t) for t in tails.values())
    at = 0
    for M, rows in tails.items():
        got = np.array([[float.fromhex(w) for w in ln.split()] for ln in lines[at:at + len(rows)]])
        at += len(rows)
        r64, rld, rpt = _reference(rows)
        # the program reads the very bits the reference reads, so float64 and longdouble decide the class; the
        # perturbed evaluation (which breaks exact ties) enters the tolerance where it is fitted as well
        agree = r64[2] == rld[2]
        assert (~agree).sum() <= 0.01 * len(rows), (M, agree)
        fitted = got[:, 0] != 0
        np.testing.assert_array_equal(fitted[agree], r64[2][agree])
        # the constant tails, the xstar == 0 tails and the spread below the bound are unfitted, the rest fitted
        assert (~r64[2]).sum() >= 5 and r64[2].sum() >= 20, (M, r64[2])
        un = agree & ~r64[2]
        assert np.isinf(got[un, 1]).all() and (got[un, 1] > 0).all()
        np.testing.assert_array_equal(got[un, 3:], rows[un, :1] - rows[un][:, M - 1::-1])
        ok = agree & r64[2]
        for name, g, cols in (('k', got[ok, 1], 0), ('sigma', got[ok, 2], 1), ('lw', got[ok, 3:], 3)):
            tol, eps = _tol(r64[cols][ok], rld[cols][ok], rpt[cols][ok], rpt[2][ok])
            err = np.abs(g - r64[cols][ok])
            print('M=%-3d %-5s eps %.3e  max err %.3e  max err/tol %.3f' % (M, name, eps, err.max(), (err / tol).max()))
            assert np.isfinite(g).all() and (err <= tol).all(), (M, name, eps, float(err.max()))


def test_the_shared_header_against_the_reference(tmp_path):
    exe = _compile(tmp_path, 'check_psis_tail', [])
    _check_program(exe, tmp_path)
    for S in list(range(1, 60)) + [99, 100, 101, 399, 400, 401, 2000, 9152, 9153, 10 ** 6, 2 ** 31 - 1]:
        assert int(_run(exe, ['--tail-length', str(S)])) == loo_ref.tail_length(S), S


def test_the_shared_header_under_asan_and_ubsan(tmp_path):
    exe = _compile(tmp_path, 'check_psis_tail_san',
                   ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer'])
    _check_program(exe, tmp_path)


def test_reference_against_a_dyad_worked_out_by_hand():
    """S < 25: M < 5, so elpd_loo = -log mean_s exp(-l_s), k = inf; lppd = log mean_s exp(l_s)"""
    l = [-0.3, -2.5, -0.01, -1.75, -0.3, -4.0, -0.9]
    want = -math.log(sum(math.exp(-v) for v in l) / len(l))
    lppd = math.log(sum(math.exp(v) for v in l) / len(l))
    for dtype in (np.float64, np.longdouble):
        e, p, k, fitted = loo_ref.psis_dyads(np.array(l, dtype=dtype)[:, None])
        assert abs(float(e[0]) - want) <= 4 * np.spacing(abs(want)), (float(e[0]), want)
        assert abs(float(p[0]) - lppd) <= 4 * np.spacing(abs(lppd))
        assert np.isinf(k[0]) and k[0] > 0 and not fitted[0]
    for S in (1, 4, 24):
        assert loo_ref.tail_length(S) < 5
    assert loo_ref.tail_length(25) == 5 and loo_ref.tail_length(100) == 20 and loo_ref.tail_length(2000) == 135
    # 24 samples stay raw however heavy the tail, 25 are smoothed: a fitted dyad has a finite k and an elpd_loo
    # between the smallest l and lppd
    rng = np.random.RandomState(2)
    l = -np.abs(rng.standard_t(2, (25, 50)))
    e, p, k, fitted = loo_ref.psis_dyads(l)
    assert fitted.all() and np.isfinite(k).all()
    assert (e <= p).all() and (e >= l.min(axis=0)).all()
    e24, _, k24, f24 = loo_ref.psis_dyads(l[:24])
    assert not f24.any() and np.isinf(k24).all()
    np.testing.assert_allclose(e24, -np.log(np.mean(np.exp(-l[:24]), axis=0)), rtol=1e-13)


def _loo_module():
    import importlib
    return importlib.import_module('dynetlsm_amd.loo')       # da.loo is the function


def _synthetic_result(da, rng, T, N, directed, S=100):
    mask = loo_ref.ic_ref.dyad_mask(N, directed)
    pw = np.zeros((T, N, N, 2))
    pw[..., 0] = np.where(mask, -rng.gamma(2.0, 0.3, (T, N, N)), 0.0)
    k = rng.normal(0.3, 0.4, (T, N, N))
    k[rng.rand(T, N, N) < 0.05] = np.inf
    pw[..., 1] = np.where(mask, k, 0.0)
    lppd_t = pw[..., 0][:, mask].sum(axis=1) + rng.rand(T)
    e, kk = pw[..., 0][:, mask], pw[..., 1][:, mask]
    totals = np.stack([e.sum(1), (e * e).sum(1), lppd_t, np.full(T, mask.sum()), np.isinf(kk).sum(1)], axis=1)
    edges = _loo_module().k_edges(S)
    hist = np.stack([np.bincount(np.searchsorted(edges, kk[t], side='right'), minlength=edges.size + 1)
                     for t in range(T)]).astype(np.uint64)
    kfull = np.where(mask, pw[..., 1], -np.inf)
    node = np.maximum(kfull.max(axis=2), kfull.max(axis=1))
    res = da.LooResult(np.arange(S), S, totals, edges, hist, node, directed, N, pw)
    return res, pw, lppd_t, kk


def test_result_arithmetic_and_comparison_against_brute_force():
    import dynetlsm_amd as da
    rng = np.random.RandomState(4)
    for directed in (False, True):
        res, pw, lppd_t, kk = _synthetic_result(da, rng, 3, 12, directed)
        want = loo_ref.result(pw, lppd_t, directed)
        for name in ('elpd_loo', 'p_loo', 'looic', 'se_elpd_loo', 'lppd', 'max_k'):
            np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-12, err_msg=name)
        assert res.n_dyads == want['n_dyads'] and res.n_unfitted == want['n_unfitted']
        for name in ('elpd_loo', 'p_loo', 'looic', 'lppd', 'n_dyads', 'n_unfitted', 'n_bad'):
            np.testing.assert_allclose(getattr(res, name + '_t').sum(), getattr(res, name), rtol=1e-12)
        for t in range(3):
            e = pw[t, ..., 0][res.dyad_mask()]
            np.testing.assert_allclose(res.se_elpd_loo_t[t], np.sqrt(e.size * np.var(e, ddof=1)), rtol=1e-10)
        assert res.k_threshold == 0.5 and list(res.k_edges) == [0.5, 0.7, 1.0]          # S = 100
        assert res.n_bad == int((kk > res.k_threshold).sum()) and res.n_bad >= res.n_unfitted > 0
        np.testing.assert_array_equal(res.k_hist, res.k_hist_t.sum(axis=0))
        assert res.k_hist.sum() == res.n_dyads
        text = res.summary()
        assert 'elpd_loo' in text and 'n_bad' in text and 'p_loo' in text
        other, pw2, _, _ = _synthetic_result(da, rng, 3, 12, directed)
        diff, se = da.compare_loo(res, other)
        d = (pw[..., 0] - pw2[..., 0])[:, res.dyad_mask()].ravel()
        np.testing.assert_allclose(diff, d.sum(), rtol=1e-12)
        np.testing.assert_allclose(se, np.sqrt(d.size * np.var(d, ddof=1)), rtol=1e-12)
        np.testing.assert_allclose(diff, res.elpd_loo - other.elpd_loo, rtol=1e-9)
    # the edges: the threshold joins them unless it is one of them
    assert list(_loo_module().k_edges(10000)) == [0.5, 0.7, 1.0] and _loo_module().k_threshold(10000) == 0.7
    e25 = _loo_module().k_edges(25)
    assert len(e25) == 4 and e25[0] == _loo_module().k_threshold(25) == min(1 - 1 / np.log10(25), 0.7)
    assert list(e25) == sorted(e25)
    # mismatched inputs: the errors of compare_information_criteria
    a, _, _, _ = _synthetic_result(da, rng, 2, 8, False)
    b, _, _, _ = _synthetic_result(da, rng, 2, 9, False)
    c, _, _, _ = _synthetic_result(da, rng, 2, 8, True)
    with pytest.raises(ValueError, match='different networks'):
        da.compare_loo(a, b)
    with pytest.raises(ValueError, match='directed'):
        da.compare_loo(a, c)
    with pytest.raises(ValueError, match='LooResult'):
        da.compare_loo(a, object())
    a.pointwise_elpd_loo = None
    with pytest.raises(ValueError, match='pointwise'):
        da.compare_loo(a, a)


def test_facade_argument_checks_come_before_any_device_call():
    import dynetlsm_amd as da

    class Unfitted(object):
        pass

    with pytest.raises(ValueError, match='not fit'):
        da.loo(Unfitted())

    class Fitted(object):
        is_directed = False
        n_burn_ = 4
        Y_fit_ = np.zeros((2, 5, 5))
        Xs_ = np.zeros((10, 2, 5, 2))
        intercepts_ = np.zeros((10, 1))
    for bad in (0, -3, 2.5, 7):                # 6 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.loo(Fitted(), n_samples=bad)


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import ctypes
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_loo_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_loo_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert len(args) == 12 and args[0].startswith('dlsm_chain') and args[-1].endswith('pointwise')
    res, argtypes = _lib.SIGNATURES['dlsm_loo_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert hasattr(ctypes.CDLL(build()), 'dlsm_loo_accumulate')
    assert callable(da.loo) and callable(da.compare_loo) and callable(da.Chain.loo_accumulate)
    for name in ('loo', 'compare_loo', 'LooResult'):
        assert name in da.__all__
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dlsm_loo_accumulate(' in doc


def test_every_instantiation_of_the_kernel_is_free_of_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_loo_accumulate<%d,%s>' % (d, m) for d in range(1, 9) for m in ('false', 'true')]
    names += ['k_loo_decode_nodes']
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
        assert md[name]['vgpr'] <= 512, (name, md[name])
        # the static part leaves the 144 KB of the sorted buffers within the 160 KB of a workgroup
        assert md[name]['lds'] + (144 << 10) <= (160 << 10), (name, md[name])
    assert sorted(k for k in md if k.startswith('k_loo_')) == sorted(names)
