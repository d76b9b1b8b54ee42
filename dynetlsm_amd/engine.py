"""Python face of one device-resident MCMC chain (one ``dlsm_chain`` handle).

Thin: argument checking, dtype/contiguity normalisation and error mapping.
All arithmetic happens in the HIP library; nothing here computes a likelihood.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (EngineError, LsmConfig, HdpConfig, c_double_p, c_i32_p, c_i64_p,
                   UNDIRECTED, DIRECTED, DIRECTED_CASE_CONTROL)

__all__ = ['Chain', 'SamplerGrid', 'EngineError', 'MAX_FEATURES', 'check_n_features']

# The kernels take the latent dimension as a template parameter, instantiated for 1..8 (csrc/device_common.hpp
# DLSM_D_MAX; the reference takes any n_features, lsm.py:235,254; its examples and the paper use 2).
MAX_FEATURES = 8


def check_n_features(n_features):
    """ValueError naming the limit, before any device call (capi.hip's DISPATCH_D would answer
    DLSM_E_LIMIT from the first kernel launch only)"""
    d = int(n_features)
    if d != n_features or not 1 <= d <= MAX_FEATURES:
        raise ValueError('n_features=%r is not supported by the MI355X engine: its kernels are '
                         'compiled for 1 <= n_features <= %d latent dimensions' % (n_features, MAX_FEATURES))
    return d


def packed_row_words(N):
    """uint32 words of one bit-packed network row (capi.hip dlsm_create: a multiple of 4)"""
    return ((int(N) + 31) // 32 + 3) // 4 * 4


def pack_network(Y):
    """(T, N, N) 0/1 array -> (T, N, W) uint32 rows in the engine's layout: bit j % 32 of word
    j // 32 of row i is Y[t, i, j]; padding bits are zero"""
    Y = np.asarray(Y)
    T, N = Y.shape[0], Y.shape[1]
    W = packed_row_words(N)
    B = np.zeros((T, N, 32 * W), dtype=np.uint8)
    B[:, :, :N] = Y != 0
    bytes_ = np.packbits(B, axis=-1, bitorder='little')
    return np.ascontiguousarray(bytes_).view('<u4').astype(np.uint32).reshape(T, N, W)


def rank_candidates(index, value, k, largest=True):
    """The first ``k`` of the candidates of one time step as ``dlsm_topk_accumulate`` wrote them - ``index`` (n, 4)
    int32 rows (i, j, y, 0), ``value`` (n, 2) rows (proba, sd), in any order - by (proba descending - ascending
    unless ``largest`` -, then i, then j): the tuple (i, j, y, proba, sd) of arrays in rank order"""
    ij = index[:, 0].astype(np.int64) * (1 << 31) + index[:, 1]
    order = np.lexsort((ij, -value[:, 0] if largest else value[:, 0]))[:k]
    index, value = index[order].astype(np.int64), value[order]
    return (np.ascontiguousarray(index[:, 0]), np.ascontiguousarray(index[:, 1]), np.ascontiguousarray(index[:, 2]),
            np.ascontiguousarray(value[:, 0]), np.ascontiguousarray(value[:, 1]))


def check_node_ids(nodes, N, name='nodes'):
    """a non-empty one-dimensional array of integer node ids in 0..N-1 as int64 (ValueError, before any device
    call)"""
    ids = np.asarray(nodes)
    if ids.ndim != 1 or not ids.size or ids.dtype == bool or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError('%s must be a non-empty one-dimensional array of integer node ids, got %r' % (name, nodes))
    if (ids < 0).any() or (ids >= N).any():
        raise ValueError('%s must lie in 0..%d, got %r' % (name, N - 1, nodes))
    return ids.astype(np.int64)


def check_missing_index(index, T, N, model):
    """(n, 3) int32 rows (t, i, j) of missing dyads, validated as ``dlsm_set_missing`` validates them
    (ValueError, before any device call)"""
    idx = np.asarray(index)
    if idx.size == 0:
        return np.zeros((0, 3), dtype=np.int32)
    if idx.ndim != 2 or idx.shape[1] != 3 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError('missing dyads must be an (n, 3) integer array of (t, i, j) rows')
    if model == DIRECTED_CASE_CONTROL:
        raise ValueError('case-control chains hold edge lists: missing dyads cannot be sampled')
    t, i, j = idx[:, 0], idx[:, 1], idx[:, 2]
    if (t < 0).any() or (t >= T).any() or (idx[:, 1:] < 0).any() or (idx[:, 1:] >= N).any():
        raise ValueError('missing dyad outside T=%d, N=%d' % (T, N))
    if model == UNDIRECTED and (i >= j).any():
        raise ValueError('undirected missing dyads are listed with i < j')
    if (i == j).any():
        raise ValueError('the diagonal is not a dyad')
    key = (t.astype(np.int64) * N + i) * N + j
    if np.unique(key).shape[0] != key.shape[0]:
        raise ValueError('a missing dyad is listed twice')
    return np.ascontiguousarray(idx, dtype=np.int32)


def _f64(a, shape=None, name='array'):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError('%s has shape %s, expected %s' % (name, a.shape, shape))
    return a


def _i64(a, shape=None, name='array'):
    a = np.ascontiguousarray(a, dtype=np.int64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError('%s has shape %s, expected %s' % (name, a.shape, shape))
    return a


def _i32(a, shape=None, name='array'):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError('%s has shape %s, expected %s' % (name, a.shape, shape))
    return a


def _p(a):
    if a.dtype == np.float64:
        return a.ctypes.data_as(c_double_p)
    if a.dtype == np.int64:
        return a.ctypes.data_as(c_i64_p)
    if a.dtype == np.int32:
        return a.ctypes.data_as(c_i32_p)
    if a.dtype == np.uint32:
        return a.ctypes.data_as(_lib.c_u32_p)
    if a.dtype == np.uint64:
        return a.ctypes.data_as(_lib.c_u64_p)
    raise TypeError(a.dtype)


def _po(a):
    """``_p`` of an optional array: NULL for None and for an empty one"""
    return _p(a) if a is not None and a.size else None


class SamplerGrid(object):
    """State of the T x N random-walk Metropolis samplers (one per (t, node)),
    the struct-of-arrays form of the reference's ``latent_samplers`` list of
    ``Metropolis`` objects (metropolis.py:85-94, lsm.py:451-457)."""

    def __init__(self, T, N, step_size=0.1, tune=500, tune_interval=100):
        self.step_size = np.full((T, N), float(step_size))
        self.n_accepted = np.zeros((T, N), dtype=np.int32)
        self.n_steps = np.zeros((T, N), dtype=np.int32)
        self.steps_until_tune = np.full((T, N), tune_interval, dtype=np.int32)
        self.tune = tune
        self.tune_interval = tune_interval

    @classmethod
    def from_objects(cls, samplers):
        """Build from a list (T) of lists (N) of Metropolis-like objects."""
        T, N = len(samplers), len(samplers[0])
        s0 = samplers[0][0]
        g = cls(T, N, s0.step_size, s0.tune, s0.tune_interval)
        for t in range(T):
            for j in range(N):
                s = samplers[t][j]
                g.step_size[t, j] = s.step_size
                g.n_accepted[t, j] = s.n_accepted
                g.n_steps[t, j] = s.n_steps
                g.steps_until_tune[t, j] = s.steps_until_tune
        return g

    def to_objects(self, samplers):
        for t in range(len(samplers)):
            for j in range(len(samplers[0])):
                s = samplers[t][j]
                s.step_size = float(self.step_size[t, j])
                s.n_accepted = int(self.n_accepted[t, j])
                s.n_steps = int(self.n_steps[t, j])
                s.steps_until_tune = int(self.steps_until_tune[t, j])


class Chain(object):
    """One chain on one MI355X.

    Parameters mirror ``dlsm_create``: ``model`` is 'undirected', 'directed' or
    'case_control'; (seed, chain_id) key the Philox streams.
    """
    MODELS = {'undirected': UNDIRECTED, 'directed': DIRECTED,
              'case_control': DIRECTED_CASE_CONTROL}

    def __init__(self, T, N, D=2, model='undirected', seed=0, chain_id=0, device=0):
        check_n_features(D)
        self._L = _lib.load()
        self._h = _lib.handle_t()
        self.T, self.N, self.D = int(T), int(N), int(D)
        self.model = self.MODELS[model] if isinstance(model, str) else int(model)
        self.n_intercepts = 1 if self.model == UNDIRECTED else 2
        rc = self._L.dlsm_create(int(device), self.T, self.N, self.D, self.model,
                                 C.c_uint64(int(seed) & (2 ** 64 - 1)), int(chain_id),
                                 C.byref(self._h))
        if rc != 0:
            msg = self._L.dlsm_last_error(None)
            self._h = None
            raise EngineError(rc, msg.decode() if msg else 'dlsm_create failed')
        self.K = 0
        self.C = 0
        self.seed, self.chain_id = int(seed) & (2 ** 64 - 1), int(chain_id)    # the Philox key

    # -- plumbing ---------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            msg = self._L.dlsm_last_error(self._h)
            raise EngineError(rc, msg.decode() if msg else '?')

    def close(self):
        if getattr(self, '_h', None):
            self._L.dlsm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        self._ck(self._L.dlsm_synchronize(self._h))

    # -- network -----------------------------------------------------------
    def upload_network(self, Y):
        Y = _f64(Y, (self.T, self.N, self.N), 'Y')
        self._ck(self._L.dlsm_upload_network(self._h, _p(Y)))

    def network_packed_words(self):
        """uint32 words of the bit-packed network as the chain holds it"""
        n = C.c_int64(0)
        self._ck(self._L.dlsm_network_packed_words(self._h, C.byref(n)))
        return int(n.value)

    def get_network_packed(self, ptr, n_words):
        """copy the packed network into ``ptr`` (device or host address, e.g.
        ``tensor.data_ptr()`` of an int32 tensor of ``n_words`` elements)"""
        self._ck(self._L.dlsm_get_network_packed(self._h, C.c_void_p(int(ptr)), int(n_words)))

    def set_network_packed(self, ptr, n_words):
        """take the packed network from ``ptr`` (as written by ``get_network_packed`` of a
        chain of the same shape and model); the layout's invariants are checked"""
        self._ck(self._L.dlsm_set_network_packed(self._h, C.c_void_p(int(ptr)), int(n_words)))

    def upload_edges(self, in_edges, out_edges, degree):
        ie = _i64(in_edges); oe = _i64(out_edges)
        dg = _i64(degree, (self.T, self.N, 2), 'degree')
        if ie.shape[:2] != (self.T, self.N) or oe.shape[:2] != (self.T, self.N):
            raise ValueError('edge lists must be (T, N, max_degree)')
        self._ck(self._L.dlsm_upload_edges(self._h, _p(ie), ie.shape[2], _p(oe),
                                           oe.shape[2], _p(dg)))

    def upload_network_edges(self, net):
        """the network from a ``SparseNetwork``'s lists: the packed rows of an undirected / directed chain,
        the degree and edge tables of a case-control chain, built on the device"""
        if tuple(net.shape) != (self.T, self.N, self.N):
            raise ValueError('network has shape %s, expected %s' % (tuple(net.shape), (self.T, self.N, self.N)))
        offsets, src, dst = net.by_time()
        self._ck(self._L.dlsm_upload_network_edges(self._h, _p(offsets), _po(src), _po(dst)))

    def edge_table_widths(self):
        """(Din, Dout): the widths of a case-control chain's padded in / out edge tables"""
        din, dout = C.c_int(0), C.c_int(0)
        self._ck(self._L.dlsm_edge_table_widths(self._h, C.byref(din), C.byref(dout)))
        return int(din.value), int(dout.value)

    def get_edge_tables(self):
        """(in_edges (T, N, Din), out_edges (T, N, Dout), degree (T, N, 2)) int64, as a case-control
        chain holds them"""
        din, dout = self.edge_table_widths()
        ie = np.zeros((self.T, self.N, din), dtype=np.int64)
        oe = np.zeros((self.T, self.N, dout), dtype=np.int64)
        dg = np.zeros((self.T, self.N, 2), dtype=np.int64)
        # (an empty table still needs an address: the engine copies nothing into it)
        self._ck(self._L.dlsm_get_edges(self._h, _p(ie if ie.size else np.zeros(1, dtype=np.int64)),
                                        _p(oe if oe.size else np.zeros(1, dtype=np.int64)), _p(dg)))
        return ie, oe, dg

    def set_controls(self, control_nodes_in, control_nodes_out):
        ci = _i64(control_nodes_in); co = _i64(control_nodes_out)
        if ci.shape != co.shape or ci.shape[:2] != (self.T, self.N):
            raise ValueError('control node arrays must both be (T, N, n_control)')
        self.C = ci.shape[2]
        self._ck(self._L.dlsm_set_controls(self._h, _p(ci), _p(co), self.C))

    def get_controls(self):
        ci = np.zeros((self.T, self.N, self.C), dtype=np.int64)
        co = np.zeros_like(ci)
        self._ck(self._L.dlsm_get_controls(self._h, _p(ci), _p(co)))
        return ci, co

    def resample_controls(self, it, n_control):
        self._ck(self._L.dlsm_resample_controls(self._h, int(it), int(n_control)))
        self.C = int(n_control)

    # -- missing dyads -------------------------------------------------------
    def set_missing(self, index):
        """the missing dyads as (n, 3) rows (t, i, j): i < j for the undirected model, i != j for the
        directed one; an empty list clears them.  Checked here, before any device call, and again by
        the engine."""
        idx = check_missing_index(index, self.T, self.N, self.model)
        self._ck(self._L.dlsm_set_missing(self._h, _p(idx) if idx.shape[0] else None, idx.shape[0]))
        self.n_missing = int(idx.shape[0])

    def set_missing_edges(self, net, allow_ties=False):
        """the missing dyads from the missing lists of a ``SparseNetwork``: pairs in any order, duplicates
        allowed, either orientation for the undirected model.  The tables are built on the device and are those
        of ``set_missing`` for the distinct dyads in row-major order (``get_missing_index``).
        ``allow_ties=False``: a listed dyad that is a tie of the uploaded network is an error."""
        if tuple(net.shape) != (self.T, self.N, self.N):
            raise ValueError('network has shape %s, expected %s' % (tuple(net.shape), (self.T, self.N, self.N)))
        offsets, src, dst = net.missing_by_time()
        self.n_missing = 0
        self._ck(self._L.dlsm_set_missing_edges(self._h, _p(offsets), _po(src), _po(dst), int(bool(allow_ties))))
        n = C.c_int64(0)
        self._ck(self._L.dlsm_missing_count(self._h, C.byref(n)))
        self.n_missing = int(n.value)

    def get_missing_index(self):
        """(n, 3) int64 rows (t, i, j) in the order of the accumulators: row-major after ``set_missing_edges``,
        the caller's own list after ``set_missing``"""
        n = C.c_int64(0)
        self._ck(self._L.dlsm_missing_count(self._h, C.byref(n)))
        tij = np.zeros((int(n.value), 3), dtype=np.int32)
        if tij.shape[0]:
            self._ck(self._L.dlsm_get_missing_index(self._h, _p(tij)))
        return tij.astype(np.int64)

    def impute_missing(self, it, accumulate=False):
        """draw every missing dyad from its conditional at the current state (the draws of iteration
        ``it``) into the chain's network; asynchronous"""
        self._ck(self._L.dlsm_impute_missing(self._h, int(it), int(bool(accumulate))))

    def missing_sampling(self, on=True, accumulate_after=0):
        """``lsm_run`` ends every iteration with the step; it accumulates when it > accumulate_after"""
        self._ck(self._L.dlsm_missing_sampling(self._h, int(bool(on)), int(accumulate_after)))

    def get_missing(self):
        """(p_sum (n,), ones (n,) uint32, n_accumulated) in the order of ``set_missing``'s list"""
        n = getattr(self, 'n_missing', 0)
        ps = np.zeros(n)
        ones = np.zeros(n, dtype=np.uint32)
        k = C.c_int64(0)
        self._ck(self._L.dlsm_get_missing(self._h, _p(ps), ones.ctypes.data_as(_lib.c_u32_p), C.byref(k)))
        return ps, ones, int(k.value)

    def reset_missing_sums(self):
        self._ck(self._L.dlsm_reset_missing_sums(self._h))

    # -- state -------------------------------------------------------------
    def set_positions(self, X):
        X = _f64(X, (self.T, self.N, self.D), 'X')
        self._ck(self._L.dlsm_set_positions(self._h, _p(X)))

    def get_positions(self):
        X = np.zeros((self.T, self.N, self.D))
        self._ck(self._L.dlsm_get_positions(self._h, _p(X)))
        return X

    def set_intercepts(self, b):
        b = _f64(np.atleast_1d(b).ravel(), (self.n_intercepts,), 'intercept')
        self._ck(self._L.dlsm_set_intercepts(self._h, _p(b), self.n_intercepts))

    def get_intercepts(self):
        b = np.zeros(self.n_intercepts)
        self._ck(self._L.dlsm_get_intercepts(self._h, _p(b), self.n_intercepts))
        return b

    def set_radii(self, radii):
        r = _f64(radii, (self.N,), 'radii')
        self._ck(self._L.dlsm_set_radii(self._h, _p(r)))

    def get_radii(self):
        r = np.zeros(self.N)
        self._ck(self._L.dlsm_get_radii(self._h, _p(r)))
        return r

    def set_squared(self, squared):
        self._ck(self._L.dlsm_set_squared(self._h, int(bool(squared))))

    def set_samplers(self, grid):
        sh = (self.T, self.N)
        st = _f64(grid.step_size, sh, 'step_size')
        na = _i32(grid.n_accepted, sh); ns = _i32(grid.n_steps, sh)
        un = _i32(grid.steps_until_tune, sh)
        tune = -1 if grid.tune is None else int(grid.tune)
        self._ck(self._L.dlsm_set_samplers(self._h, _p(st), _p(na), _p(ns), _p(un),
                                           tune, int(grid.tune_interval)))

    def get_samplers(self, grid):
        """read the device's sampler state back into ``grid`` (in place)"""
        sh = (self.T, self.N)
        st = np.zeros(sh); na = np.zeros(sh, dtype=np.int32)
        ns = np.zeros(sh, dtype=np.int32); un = np.zeros(sh, dtype=np.int32)
        self._ck(self._L.dlsm_get_samplers(self._h, _p(st), _p(na), _p(ns), _p(un)))
        grid.step_size[...] = st; grid.n_accepted[...] = na
        grid.n_steps[...] = ns; grid.steps_until_tune[...] = un
        return grid

    def set_prior_random_walk(self, tau_sq, sigma_sq):
        self._ck(self._L.dlsm_set_prior_random_walk(self._h, float(tau_sq),
                                                    float(sigma_sq)))

    def set_prior_mixture(self, mu, sigma, lmbda, z):
        """``z=None`` keeps the labels the device already holds (those of the last
        ``sample_labels`` or ``set_prior_mixture``)."""
        sigma = _f64(sigma)
        K = sigma.shape[0]
        mu = _f64(mu, (K, self.D), 'mu')
        zp = None if z is None else _p(_i64(z, (self.T, self.N), 'z'))
        lm = float(np.asarray(lmbda).ravel()[0])
        self._ck(self._L.dlsm_set_prior_mixture(self._h, _p(mu), _p(sigma), lm, zp, K))
        self.K = K

    # -- kernels -----------------------------------------------------------
    def loglik_full(self, intercepts=None):
        """network log-likelihood at the current X; ``intercepts`` (m, n_ic)
        evaluates m candidates in fused passes, None the current intercept."""
        if intercepts is None:
            out = np.zeros(1)
            self._ck(self._L.dlsm_loglik_full(self._h, 1, None, _p(out)))
            return float(out[0])
        ic = _f64(np.atleast_2d(intercepts))
        if ic.shape[1] != self.n_intercepts:
            raise ValueError('intercepts must be (m, %d)' % self.n_intercepts)
        out = np.zeros(ic.shape[0])
        self._ck(self._L.dlsm_loglik_full(self._h, ic.shape[0], _p(ic), _p(out)))
        return out

    def loglik_full_radii(self, radii_alt):
        r = _f64(radii_alt, (self.N,), 'radii_alt')
        out = np.zeros(2)
        self._ck(self._L.dlsm_loglik_full_radii(self._h, _p(r), _p(out)))
        return out

    def loglik_partial(self, t, j, x=None, with_prior=False):
        out = np.zeros(1)
        xp = None
        if x is not None:
            x = _f64(x, (self.D,), 'x')
            xp = _p(x)
        self._ck(self._L.dlsm_loglik_partial(self._h, int(t), int(j), xp,
                                             int(with_prior), _p(out)))
        return float(out[0])

    def loglik_partial_all(self, with_prior=False):
        out = np.zeros((self.T, self.N))
        self._ck(self._L.dlsm_loglik_partial_all(self._h, int(with_prior), _p(out)))
        return out

    def sweep_positions(self, it, algo=0):
        self._ck(self._L.dlsm_sweep_positions(self._h, int(it), int(algo)))

    def resolve_sweep_algo(self, algo=0):
        """the sweep algorithm ``algo`` resolves to on this chain (0 = auto)"""
        rc = self._L.dlsm_resolve_sweep_algo(self._h, int(algo))
        if rc < 0:
            self._ck(rc)
        return rc

    def pipe_head_nodes(self):
        """nodes per evaluator workgroup of the last pipelined sweep's head launch: 16, or 8 when it was
        spread over twice the workgroups; 0 before the first such sweep"""
        q = C.c_int(0)
        self._ck(self._L.dlsm_pipe_head_nodes(self._h, C.byref(q)))
        return int(q.value)

    def center(self):
        self._ck(self._L.dlsm_center(self._h))

    def procrustes(self, X_ref):
        X_ref = _f64(X_ref, (self.T, self.N, self.D), 'X_ref')
        R = np.zeros((self.D, self.D))
        self._ck(self._L.dlsm_procrustes(self._h, _p(X_ref), _p(R)))
        return R

    def gaussian_likelihood(self, node, normalize=True):
        out = np.zeros((self.T, self.K))
        self._ck(self._L.dlsm_gaussian_likelihood(self._h, int(node), int(normalize),
                                                  _p(out)))
        return out

    def sample_labels(self, it, w):
        K = self.K
        w = _f64(w, (self.T, K, K), 'w')
        z = np.zeros((self.T, self.N), dtype=np.int64)
        n = np.zeros((self.T, K, K))
        nk = np.zeros((self.T, K), dtype=np.int64)
        self._ck(self._L.dlsm_sample_labels(self._h, int(it), _p(w), _p(z), _p(n), _p(nk)))
        return z, n, nk

    # -- device-resident LSM loop -------------------------------------------
    def hdp_label_sums(self, stage, mu=None, sigma=None, lmbda=0.0, w=None, a=0.0, b=0.0):
        """Label-wise sums of the HDP-LPCM conjugate updates on the device (stage 0 means,
        1 residuals, 2 lambda, 3 log-posterior node terms); see ``dlsm_hdp_label_sums``."""
        K = self.K
        nv = self.D if stage == 0 else (2 if stage == 2 else 1)
        out = np.empty((self.T, K, nv) if nv > 1 else (self.T, K))
        mu = None if mu is None else _f64(mu, (K, self.D), 'mu')
        sigma = None if sigma is None else _f64(sigma, (K,), 'sigma')
        w = None if w is None else _f64(w, (self.T, K, K), 'w')
        self._ck(self._L.dlsm_hdp_label_sums(
            self._h, int(stage), None if mu is None else _p(mu),
            None if sigma is None else _p(sigma), float(np.ravel(lmbda)[0]),
            None if w is None else _p(w), float(a), float(b), _p(out)))
        return out

    def lsm_configure(self, intercept_prior, intercept_variance_prior,
                      step_size_intercept=0.1, tune=None, tune_interval=100,
                      n_iter_procrustes=0, sweep_algo=0, state=None, step_size_radii=175000.,
                      radii_tune=None, radii_tune_interval=100):
        cfg = LsmConfig()
        ip = np.atleast_1d(np.asarray(intercept_prior, dtype=np.float64)).ravel()
        for k in range(2):
            cfg.intercept_prior[k] = ip[k] if k < ip.size else 0.0
            cfg.i_step_size[k] = float(step_size_intercept)
            cfg.i_n_accepted[k] = 0
            cfg.i_n_steps[k] = 0
            cfg.i_steps_until_tune[k] = int(tune_interval)
        if state is not None:       # (step, n_accepted, n_steps, until) per sampler
            for k, s in enumerate(state):
                cfg.i_step_size[k], cfg.i_n_accepted[k] = s[0], s[1]
                cfg.i_n_steps[k], cfg.i_steps_until_tune[k] = s[2], s[3]
        cfg.intercept_variance_prior = float(intercept_variance_prior)
        cfg.i_tune = -1 if tune is None else int(tune)
        cfg.i_tune_interval = int(tune_interval)
        cfg.n_iter_procrustes = int(n_iter_procrustes)
        cfg.sweep_algo = int(sweep_algo)
        cfg.r_step_size = float(step_size_radii)
        cfg.r_n_accepted, cfg.r_n_steps = 0, 0
        cfg.r_steps_until_tune = int(radii_tune_interval)
        cfg.r_tune = -1 if radii_tune is None else int(radii_tune)
        cfg.r_tune_interval = int(radii_tune_interval)
        self._ck(self._L.dlsm_lsm_configure(self._h, C.byref(cfg)))

    def lsm_get_config(self):
        cfg = LsmConfig()
        self._ck(self._L.dlsm_lsm_get_config(self._h, C.byref(cfg)))
        return cfg

    def trace_alloc(self, n_total, logp0=0.0):
        self._ck(self._L.dlsm_trace_alloc(self._h, int(n_total), float(logp0)))
        self._trace_n = int(n_total)

    def lsm_run(self, first, count, procrustes_ref=-1):
        """enqueue iterations first..first+count-1 (asynchronous)"""
        self._ck(self._L.dlsm_lsm_run(self._h, int(first), int(count),
                                      int(procrustes_ref)))

    def trace_read(self, first, count, positions=True):
        Xs = np.zeros((count, self.T, self.N, self.D)) if positions else None
        ics = np.zeros((count, 2))
        lps = np.zeros(count)
        self._ck(self._L.dlsm_trace_read(self._h, int(first), int(count),
                                         _p(Xs) if positions else None, _p(ics),
                                         _p(lps)))
        return Xs, ics[:, :self.n_intercepts], lps

    # -- device-resident HDP-LPCM loop -------------------------
    def hdp_configure(self, hp, beta, weights, intercept_prior, intercept_variance_prior,
                      step_size_intercept=0.1, tune=None, tune_interval=100, sweep_algo=0,
                      state=None, step_size_radii=175000., radii_tune=None, radii_tune_interval=100):
        """``hp``: an object with the HDP-LPCM's hyper-parameters as attributes (gamma,
        alpha_init, alpha, kappa, mean_variance_prior, b, a, a0, b0, c0, d0 - None switches an
        update off -, lambda_prior, lambda_variance_prior, *_prior_shape / *_rate); beta (K,),
        weights (T, K, K).  The mixture prior (mu, sigma, lmbda, z) must be set."""
        K = self.K
        cfg = HdpConfig()
        for name in ('gamma', 'alpha_init', 'alpha', 'kappa', 'mean_variance_prior', 'b', 'a',
                     'lambda_prior', 'lambda_variance_prior', 'gamma_prior_shape',
                     'gamma_prior_rate', 'alpha_init_shape', 'alpha_init_rate',
                     'alpha_kappa_shape', 'alpha_kappa_rate'):
            setattr(cfg, name, float(np.ravel(getattr(hp, name))[0]))
        cfg.has_a0 = int(hp.a0 is not None)
        cfg.has_c0 = int(hp.c0 is not None)
        cfg.a0, cfg.b0 = (float(hp.a0), float(hp.b0)) if hp.a0 is not None else (0.0, 0.0)
        cfg.c0, cfg.d0 = (float(hp.c0), float(hp.d0)) if hp.c0 is not None else (0.0, 0.0)
        cfg.intercept_prior = float(np.ravel(intercept_prior)[0])
        cfg.intercept_variance_prior = float(intercept_variance_prior)
        cfg.i_step_size = float(step_size_intercept)
        cfg.i_n_accepted, cfg.i_n_steps = 0, 0
        cfg.i_steps_until_tune = int(tune_interval)
        if state is not None:       # (step, n_accepted, n_steps, until)
            cfg.i_step_size, cfg.i_n_accepted = float(state[0]), int(state[1])
            cfg.i_n_steps, cfg.i_steps_until_tune = int(state[2]), int(state[3])
        cfg.i_tune = -1 if tune is None else int(tune)
        cfg.i_tune_interval = int(tune_interval)
        cfg.sweep_algo = int(sweep_algo)
        if self.model != UNDIRECTED:        # intercept_out and the radii sampler (hdp_lpcm.py:731-747)
            ip = np.ravel(np.asarray(intercept_prior, dtype=np.float64))
            cfg.intercept_prior_out = float(ip[1] if ip.size > 1 else ip[0])
            cfg.i_step_size_out = float(step_size_intercept)
            cfg.i_n_accepted_out, cfg.i_n_steps_out = 0, 0
            cfg.i_steps_until_tune_out = int(tune_interval)
            cfg.r_step_size = float(step_size_radii)
            cfg.r_n_accepted, cfg.r_n_steps = 0, 0
            cfg.r_steps_until_tune = int(radii_tune_interval)
            cfg.r_tune = -1 if radii_tune is None else int(radii_tune)
            cfg.r_tune_interval = int(radii_tune_interval)
        beta = _f64(beta, (K,), 'beta')
        weights = _f64(weights, (self.T, K, K), 'weights')
        self._ck(self._L.dlsm_hdp_configure(self._h, C.byref(cfg), _p(beta), _p(weights)))

    def hdp_get_config(self):
        cfg = HdpConfig()
        self._ck(self._L.dlsm_hdp_get_config(self._h, C.byref(cfg)))
        return cfg

    def hdp_trace_alloc(self, n_total, logp0=0.0):
        self._ck(self._L.dlsm_hdp_trace_alloc(self._h, int(n_total), float(logp0)))

    def hdp_run(self, first, count):
        """enqueue Gibbs iterations first..first+count-1 of the HDP-LPCM (asynchronous)"""
        self._ck(self._L.dlsm_hdp_run(self._h, int(first), int(count)))

    def hdp_trace_read(self, first, count, positions=True, labels=True, weights=True, small=True):
        """dict of the stored samples first..first+count-1: ``Xs`` (positions), ``zs`` (labels),
        ``weights`` - the three large arrays, each optional - and the small ones (``small``)"""
        T, N, D, K = self.T, self.N, self.D, self.K
        out = {}
        if small:
            out.update(intercepts=np.zeros((count, 2)), logps=np.zeros(count),
                       mus=np.zeros((count, K, D)), sigmas=np.zeros((count, K)),
                       betas=np.zeros((count, K)), lambdas=np.zeros((count, 1)),
                       hypers=np.zeros((count, 6)))
        if weights:
            out['weights'] = np.zeros((count, T, K, K))
        if positions:
            out['Xs'] = np.zeros((count, T, N, D))
        if labels:
            out['zs'] = np.zeros((count, T, N), dtype=np.int64)

        def ptr(name):
            return _p(out[name]) if name in out else None
        self._ck(self._L.dlsm_hdp_trace_read(
            self._h, int(first), int(count), ptr('Xs'), ptr('intercepts'), ptr('logps'), ptr('mus'),
            ptr('sigmas'), ptr('zs'), ptr('betas'), ptr('weights'), ptr('lambdas'), ptr('hypers')))
        if small and self.model == UNDIRECTED:
            # (undirected device loop: the second slot carries the network log-likelihood of the
            # stored state, NaN where it is not known)
            out['logliks'] = out['intercepts'][:, 1].copy()
            out['intercepts'] = out['intercepts'][:, :1]
        elif small:
            out['logliks'] = np.full(count, np.nan)
        return out

    def hdp_trace_write(self, first, Xs=None, intercepts=None, logps=None, mus=None, sigmas=None,
                        zs=None, betas=None, weights=None, lambdas=None):
        """rows first .. of the device-resident trace from host arrays (the mirror of
        ``hdp_trace_read``); every given array has the same leading length"""
        T, N, D, K = self.T, self.N, self.D, self.K
        given = [a for a in (Xs, intercepts, logps, mus, sigmas, zs, betas, weights, lambdas)
                 if a is not None]
        count = int(np.shape(given[0])[0])

        def f(a, shape):
            return None if a is None else _p(_f64(np.reshape(a, (count,) + shape), (count,) + shape))
        zz = None if zs is None else _i64(zs, (count, T, N), 'zs')
        self._ck(self._L.dlsm_hdp_trace_write(
            self._h, int(first), count, f(Xs, (T, N, D)),
            None if intercepts is None else _p(_f64(
                np.reshape(intercepts, (count, -1))[:, :self.n_intercepts].copy())),
            f(logps, ()), f(mus, (K, D)), f(sigmas, (K,)), None if zz is None else _p(zz),
            f(betas, (K,)), f(weights, (T, K, K)), f(lambdas, ())))

    def hdp_queues(self):
        """queues the last ``hdp_run`` used: 2 when the intercept's likelihood pass ran beside the
        label update and the conjugate draws (undirected model, the process's only live chain)"""
        q = C.c_int(0)
        self._ck(self._L.dlsm_hdp_queues(self._h, C.byref(q)))
        return int(q.value)

    def hdp_get_aux(self):
        """auxiliary variables of the last iteration: m, m_bar, w_over, n, nk"""
        T, K = self.T, self.K
        m = np.zeros((T, K, K), dtype=np.int64); mb = np.zeros(K)
        wo = np.zeros((max(T - 1, 0), K), dtype=np.int64)
        n = np.zeros((T, K, K), dtype=np.int64); nk = np.zeros((T, K), dtype=np.int64)
        self._ck(self._L.dlsm_hdp_get_aux(self._h, _p(m), _p(mb), _p(wo), _p(n), _p(nk)))
        return dict(m=m, m_bar=mb, w_over=wo, n=n, nk=nk)

    def trace_read_radii(self, first, count):
        out = np.zeros((count, self.N))
        self._ck(self._L.dlsm_trace_read_radii(self._h, int(first), int(count), _p(out)))
        return out

    def radii_step_read(self):
        """the radii step of the last iteration ``lsm_run`` ran, accepted or not: (proposal (N,),
        dict(dir_q, logu, ll_proposal, ll_current)); accepted iff logu < ll_proposal - ll_current + dir_q"""
        x = np.zeros(self.N)
        t = np.zeros(4)
        self._ck(self._L.dlsm_lsm_get_radii_step(self._h, _p(x), _p(t)))
        return x, dict(dir_q=t[0], logu=t[1], ll_proposal=t[2], ll_current=t[3])

    # -- starting values -----------------------------------
    def init_shortest_paths(self):
        self._ck(self._L.dlsm_init_shortest_paths(self._h))

    def init_get_dissimilarity(self, t):
        out = np.empty((self.N, self.N))
        self._ck(self._L.dlsm_init_get_dissimilarity(self._h, int(t), _p(out)))
        return out

    def init_smacof(self, t, X0, max_iter=300, eps=1e-6):
        """SMACOF runs from the starting configurations ``X0`` (n_init, N, D);
        returns (X[n_init, N, D], stress[n_init], n_iter[n_init])."""
        X0 = np.ascontiguousarray(X0, dtype=np.float64)
        if X0.ndim == 2:
            X0 = X0[None]
        X0 = _f64(X0, (X0.shape[0], self.N, self.D), 'X0')
        n_init = X0.shape[0]
        X = np.empty_like(X0)
        stress = np.empty(n_init)
        n_iter = np.empty(n_init, dtype=np.int32)
        self._ck(self._L.dlsm_init_smacof(self._h, int(t), n_init, _p(X0), int(max_iter),
                                          float(eps), _p(X), _p(stress), _p(n_iter)))
        return X, stress, n_iter

    def init_gmds_step(self, t, X_prev, lmbda=10.0, max_lanczos=256, tol=1e-12):
        """One Sarkar-Moore step; returns (X_t, evals[D], info) with info =
        {'n_lanczos', 'residual'}."""
        X_prev = _f64(X_prev, (self.N, self.D), 'X_prev')
        X = np.empty_like(X_prev)
        evals = np.empty(self.D)
        nl = np.zeros(1, dtype=np.int32)
        res = np.zeros(1)
        self._ck(self._L.dlsm_init_gmds_step(self._h, int(t), _p(X_prev), float(lmbda),
                                             int(max_lanczos), float(tol), _p(X), _p(evals),
                                             _p(nl), _p(res)))
        return X, evals, {'n_lanczos': int(nl[0]), 'residual': float(res[0])}

    def init_mle_sums(self, p0, p1):
        out = np.empty(3)
        self._ck(self._L.dlsm_init_mle_sums(self._h, float(p0), float(p1), _p(out)))
        return out

    def init_release(self):
        self._ck(self._L.dlsm_init_release(self._h))

    # -- post-loop processing ---------------------------------
    def init_kmeans_lloyd(self, Xc, centers_init, max_iter=300, tol=0.0):
        """scikit-learn's Lloyd loop on the centred (N, F) matrix from the given seeding; returns
        (centers, labels, n_iter) or None when a cluster emptied (the caller finishes on the host)"""
        Xc = _f64(Xc)
        N, F = Xc.shape
        K = int(np.shape(centers_init)[0])
        c0 = _f64(centers_init, (K, F), 'centers_init')
        cen = np.empty((K, F)); lab = np.empty(N, dtype=np.int32)
        nit = np.zeros(1, dtype=np.int32); empty = np.zeros(1, dtype=np.int32)
        self._ck(self._L.dlsm_init_kmeans_lloyd(self._h, _p(Xc), N, F, K, _p(c0), int(max_iter),
                                                float(tol), _p(cen), _p(lab), _p(nit), _p(empty)))
        if empty[0]:
            return None
        return cen, lab, int(nit[0])

    def post_cooccurrence(self, zs, K, want_matrix=True):
        """co-occurrence probabilities of the kept samples ``zs`` (S, T, N); returns the
        (T, N, N) matrices (or None) and keeps them on the device for the VI sums"""
        zs = _i64(zs, (np.shape(zs)[0], self.T, self.N), 'zs')
        out = np.empty((self.T, self.N, self.N)) if want_matrix else None
        self._ck(self._L.dlsm_post_cooccurrence(self._h, _p(zs), zs.shape[0], int(K),
                                                None if out is None else _p(out)))
        self._post_S = zs.shape[0]
        return out

    def post_expected_vi_sums(self):
        out = np.empty((self.T, self._post_S))
        self._ck(self._L.dlsm_post_expected_vi_sums(self._h, _p(out)))
        return out

    def post_release(self):
        self._ck(self._L.dlsm_post_release(self._h))

    # the same on the device-resident trace of hdp_run (rows first .. first + count - 1)
    def post_trace_label_counts(self, first, count):
        """(count, T, K) int32: nodes per label, time and stored sample"""
        nk = np.empty((count, self.T, self.K), dtype=np.int32)
        self._ck(self._L.dlsm_post_trace_label_counts(self._h, int(first), int(count),
                                                      nk.ctypes.data_as(c_i32_p)))
        return nk

    def post_trace_cooccurrence(self, first, count, want_matrix=False):
        """co-occurrence probabilities of the stored samples: returns (matrix or None, row sums
        (T, N)); the matrices stay on the device for the VI sums / ``post_get_cooccurrence``"""
        out = np.empty((self.T, self.N, self.N)) if want_matrix else None
        rs = np.empty((self.T, self.N))
        self._ck(self._L.dlsm_post_trace_cooccurrence(self._h, int(first), int(count),
                                                      None if out is None else _p(out), _p(rs)))
        self._post_S = int(count)
        return out, rs

    def post_get_cooccurrence(self):
        out = np.empty((self.T, self.N, self.N))
        self._ck(self._L.dlsm_post_get_cooccurrence(self._h, _p(out)))
        return out

    def post_trace_align(self, first, count, ref_row):
        """rotate the stored positions and cluster means of the rows onto row ``ref_row``"""
        self._ck(self._L.dlsm_post_trace_align(self._h, int(first), int(count), int(ref_row)))

    def post_trace_mean(self, first, count):
        out = np.empty((self.T, self.N, self.D))
        self._ck(self._L.dlsm_post_trace_mean(self._h, int(first), int(count), _p(out)))
        return out

    def post_latent_marginal_loglik(self, init_w, trans_w, mu, sigma, lmbda, row=-1):
        """approx_bic.py:54-76 at trace row ``row`` (-1: the chain's current positions)"""
        Ka = int(np.shape(sigma)[0])
        init_w = _f64(init_w, (Ka,), 'init_w')
        trans_w = _f64(trans_w, (self.T, Ka, Ka), 'trans_w')
        mu = _f64(mu, (Ka, self.D), 'mu')
        sigma = _f64(sigma, (Ka,), 'sigma')
        out = np.zeros(1)
        self._ck(self._L.dlsm_post_latent_marginal_loglik(
            self._h, int(row), _p(init_w), _p(trans_w), _p(mu), _p(sigma),
            float(np.ravel(lmbda)[0]), Ka, _p(out)))
        return float(out[0])

    # -- one-step-ahead forecasts ------------------------------
    def forecast_mean_probas(self, Xs, intercepts, zero_diag=False):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        S = Xs.shape[0]
        Xs = _f64(Xs, (S, self.N, self.D), 'Xs')
        b = _f64(np.broadcast_to(np.ravel(intercepts), (S,)) if np.size(intercepts) == 1
                 else np.ravel(intercepts), (S,), 'intercepts')
        out = np.empty((self.N, self.N))
        self._ck(self._L.dlsm_forecast_mean_probas(self._h, _p(Xs), _p(b), S, int(zero_diag),
                                                   _p(out)))
        return out

    def forecast_marginal(self, x, W, intercepts):
        W = np.ascontiguousarray(W, dtype=np.float64)
        S = W.shape[0]
        x = _f64(x, (self.N, self.D), 'x')
        W = _f64(W, (S, self.N), 'W')
        b = _f64(np.ravel(intercepts), (S,), 'intercepts')
        out = np.empty((self.N, self.N))
        self._ck(self._L.dlsm_forecast_marginal(self._h, _p(x), _p(W), _p(b), S, _p(out)))
        return out

    # -- the arguments the passes over posterior samples share -------------------------------
    def _samples(self, Xs, lead_shape, name, min_samples=1):
        """``Xs`` as contiguous float64 (S,) + ``lead_shape``, and S"""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        S = Xs.shape[0]
        if S < min_samples:
            raise ValueError('needs at least one sample')
        return _f64(Xs, (S,) + tuple(lead_shape), name), S

    def _intercepts_radii(self, intercepts, radii, S):
        """``intercepts`` (S,) (undirected chains) or (S, 2) as (S, 2); ``radii`` (S, N), which directed
        chains need (None for undirected ones)"""
        b = np.asarray(intercepts, dtype=np.float64)
        if b.ndim == 1 and self.model == UNDIRECTED:
            b = np.stack([b, np.zeros_like(b)], axis=1)
        b = _f64(b, (S, 2), 'intercepts')
        if self.model == UNDIRECTED:
            return b, None
        if radii is None:
            raise ValueError('directed models need radii')
        return b, _f64(radii, (S, self.N), 'radii')

    def _sample_args(self, Xs, intercepts, radii, min_samples=1):
        """(Xs (S, T, N, D), intercepts (S, 2), radii (S, N) or None, S) of S posterior samples"""
        Xs, S = self._samples(Xs, (self.T, self.N, self.D), 'Xs', min_samples)
        return (Xs,) + self._intercepts_radii(intercepts, radii, S) + (S,)

    def _packed(self, bits, name):
        """a packed network (``pack_network``) as contiguous uint32 (T, N, W)"""
        shape = (self.T, self.N, packed_row_words(self.N))
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        if bits.shape != shape:
            raise ValueError('%s has shape %s, expected %s' % (name, bits.shape, shape))
        return bits

    # -- posterior predictive goodness of fit (no reference counterpart) ----------------------
    def gof_record_length(self):
        """int64 entries of one statistics record: edges, mutual, deg_out[N], deg_in[N], esp[N]"""
        return 2 + 3 * self.N

    def gof_simulate(self, Xs, intercepts, radii=None, seed=0, first_index=0, batch=0, want_bits=False):
        """Networks drawn at the S posterior samples ``Xs`` (S, T, N, D), ``intercepts`` (S,) or (S, 2),
        ``radii`` (S, N) (directed and case-control chains), and their statistics (S, T, R) int64.
        Sample s uses RNG index ``first_index + s``: results do not depend on how the samples are split
        across calls or on ``batch`` (samples per device batch, 0: automatic).  ``want_bits``: also the
        drawn rows (S, T, N, W) uint32, bit j % 32 of word j // 32 of row i = Y[t, i, j]."""
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii, min_samples=0)
        stats = np.zeros((S, self.T, self.gof_record_length()), dtype=np.int64)
        W = packed_row_words(self.N)
        bits = np.zeros((S, self.T, self.N, W), dtype=np.uint32) if want_bits else None
        self._ck(self._L.dlsm_gof_simulate(
            self._h, _p(Xs), _p(b), _p(r) if r is not None else None, int(S),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(first_index)), int(batch), _p(stats),
            bits.ctypes.data_as(_lib.c_u32_p) if want_bits else None))
        return (stats, bits) if want_bits else stats

    def gof_observed(self, bits):
        """statistics (T, R) int64 of the packed network ``bits`` (T, N, W) uint32 (``pack_network``)"""
        bits = self._packed(bits, 'bits')
        stats = np.zeros((self.T, self.gof_record_length()), dtype=np.int64)
        self._ck(self._L.dlsm_gof_observed(self._h, bits.ctypes.data_as(_lib.c_u32_p), _p(stats)))
        return stats

    def _gof_dynamic_records(self, lead, temporal, geodesic):
        if not (temporal or geodesic):
            raise ValueError('at least one of temporal and geodesic must be requested')
        ov = np.zeros(lead + (self.T, self.T), dtype=np.int64) if temporal else None
        st = np.zeros(lead + (self.T - 1, 2 * self.N), dtype=np.int64) if temporal else None
        geo = np.zeros(lead + (self.T, self.N), dtype=np.int64) if geodesic else None
        return ov, st, geo

    def gof_dynamic_simulate(self, Xs, intercepts, radii=None, seed=0, first_index=0, batch=0, temporal=True,
                             geodesic=True, want_bits=False):
        """The statistics over time of the networks ``gof_simulate`` draws for the same arguments, ``seed``
        and ``first_index``: ``overlap`` (S, T, T), ``steps`` (S, T - 1, 2N) - persist_degree[N] and
        formed_sp[N] per step t -> t+1 - and ``geodesic`` (S, T, N) int64 (csrc/kernels_gof_dynamic.hpp;
        layouts in include/dynetlsm_hip.h).  ``temporal=False`` leaves out overlap and steps,
        ``geodesic=False`` the geodesic distances: those entries are None.  ``want_bits``: also the drawn
        rows (S, T, N, W) uint32.  Returns (overlap, steps, geodesic[, bits])."""
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii, min_samples=0)
        ov, st, geo = self._gof_dynamic_records((S,), temporal, geodesic)
        W = packed_row_words(self.N)
        bits = np.zeros((S, self.T, self.N, W), dtype=np.uint32) if want_bits else None
        self._ck(self._L.dlsm_gof_dynamic_simulate(
            self._h, _p(Xs), _p(b), _p(r) if r is not None else None, int(S),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(first_index)), int(batch),
            _p(ov) if temporal else None, _p(st) if temporal else None, _p(geo) if geodesic else None,
            bits.ctypes.data_as(_lib.c_u32_p) if want_bits else None))
        return (ov, st, geo, bits) if want_bits else (ov, st, geo)

    def gof_dynamic_observed(self, bits, temporal=True, geodesic=True):
        """(overlap (T, T), steps (T - 1, 2N), geodesic (T, N)) int64 of the packed network ``bits``
        (T, N, W) uint32 (``pack_network``); a family that is switched off is None"""
        bits = self._packed(bits, 'bits')
        ov, st, geo = self._gof_dynamic_records((), temporal, geodesic)
        self._ck(self._L.dlsm_gof_dynamic_observed(
            self._h, bits.ctypes.data_as(_lib.c_u32_p), _p(ov) if temporal else None,
            _p(st) if temporal else None, _p(geo) if geodesic else None))
        return ov, st, geo

    TRIAD_RECORD_LENGTH = 51

    def gof_triads_simulate(self, Xs, intercepts, radii=None, seed=0, first_index=0, batch=0, want_bits=False):
        """The triad records (S, T, 51) int64 of the networks ``gof_simulate`` draws for the same arguments,
        ``seed`` and ``first_index`` (csrc/kernels_gof_triads.hpp; layout in include/dynetlsm_hip.h:
        [(c - 1) * 16 + a * 4 + b] over the connected pairs of dyad code c, then the three pair counts).
        ``want_bits``: also the drawn rows (S, T, N, W) uint32."""
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii, min_samples=0)
        triads = np.zeros((S, self.T, self.TRIAD_RECORD_LENGTH), dtype=np.int64)
        W = packed_row_words(self.N)
        bits = np.zeros((S, self.T, self.N, W), dtype=np.uint32) if want_bits else None
        self._ck(self._L.dlsm_gof_triads_simulate(
            self._h, _p(Xs), _p(b), _p(r) if r is not None else None, int(S),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(first_index)), int(batch), _p(triads),
            bits.ctypes.data_as(_lib.c_u32_p) if want_bits else None))
        return (triads, bits) if want_bits else triads

    def gof_triads_observed(self, bits):
        """triad records (T, 51) int64 of the packed network ``bits`` (T, N, W) uint32 (``pack_network``)"""
        bits = self._packed(bits, 'bits')
        triads = np.zeros((self.T, self.TRIAD_RECORD_LENGTH), dtype=np.int64)
        self._ck(self._L.dlsm_gof_triads_observed(self._h, bits.ctypes.data_as(_lib.c_u32_p), _p(triads)))
        return triads

    # -- information criteria (no reference counterpart) ---------------------------------------
    def ic_accumulate(self, bits, Xs, intercepts, radii=None, want_pointwise=False):
        """Pointwise log-likelihood of the packed network ``bits`` (T, N, W) uint32 (``pack_network``)
        over the S posterior samples ``Xs`` (S, T, N, D), ``intercepts`` (S,) or (S, 2), ``radii`` (S, N)
        (directed and case-control chains), reduced on the device (csrc/kernels_ic.hpp; the pass over the
        samples: csrc/kernels_dyad_pass.hpp).  Returns ``totals`` (T, 5) - per time step sum lppd, sum var,
        sum mean, sum (lppd - var)^2, dyads - and ``sample_loglik`` (S, T), the network log-likelihood of
        each sample; ``want_pointwise``: also (T, N, N, 2), (lppd, var) per dyad (undirected: i < j filled,
        the rest 0)."""
        bits = self._packed(bits, 'bits')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        totals = np.zeros((self.T, 5))
        sample_loglik = np.zeros((S, self.T))
        pw = np.zeros((self.T, self.N, self.N, 2)) if want_pointwise else None
        self._ck(self._L.dlsm_ic_accumulate(self._h, _p(bits), _p(Xs), _p(b), _po(r), int(S), _p(totals),
                                            _p(sample_loglik), _po(pw)))
        return (totals, sample_loglik, pw) if want_pointwise else (totals, sample_loglik)

    # -- in-sample scores (no reference counterpart) --------------------------------------------
    def score_accumulate(self, bits, Xs, intercepts, radii=None, mask=None):
        """Rank statistics and log-loss of the posterior-mean edge probability of the packed network
        ``bits`` over the S samples (arguments as ``ic_accumulate``), computed on the device without
        sorting (csrc/kernels_score.hpp).  ``mask``: packed like ``bits``, a set bit excludes the dyad
        (undirected chains: either of (i, j), (j, i)).  Returns ``counts`` (T + 1, 4) uint64 - per time
        step and, in row T, pooled: n_pos, n_neg, u2, ties - and ``logloss_sum`` (T,);
        ``scores.scores_from_counts`` turns them into AUC, its bound and the mean log-loss."""
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        counts = np.zeros((self.T + 1, 4), dtype=np.uint64)
        logloss_sum = np.zeros(self.T)
        self._ck(self._L.dlsm_score_accumulate(self._h, _p(bits), _po(mask), _p(Xs), _p(b), _po(r), int(S),
                                               _p(counts), _p(logloss_sum)))
        return counts, logloss_sum

    # -- convergence of every dyad (no reference counterpart) -----------------------------------
    def convergence_accumulate(self, Xs, intercepts, radii=None, n_segments=2, seg_len=None, batch_len=None,
                               rhat_edges=(), ess_edges=(), want_pointwise=False):
        """Split R-hat and batch-means ESS of the linear predictor of every dyad over the S =
        ``n_segments * seg_len`` samples ``Xs`` (S, T, N, D), ``intercepts`` (S,) or (S, 2), ``radii``
        (S, N) (directed and case-control chains): the halves of the chains, segment after segment
        (csrc/kernels_conv.hpp).  ``batch_len`` defaults to floor(sqrt(seg_len)).  Returns ``hist_rhat``
        (T, len(rhat_edges) + 1) and ``hist_ess`` (T, len(ess_edges) + 1) uint64 - the bin of a value is
        the number of edges <= it -, ``node_rhat_max`` (T, N) and ``node_ess_min`` (T, N) over the dyads
        of each node; ``want_pointwise``: also (T, N, N, 2), (rhat, ess) per dyad (undirected: i < j
        filled, the rest 0)."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        S = Xs.shape[0]
        n_segments = int(n_segments)
        if seg_len is None:
            seg_len = S // max(1, n_segments)
        seg_len = int(seg_len)
        if n_segments < 2 or n_segments % 2 or seg_len < 2 or n_segments * seg_len != S:
            raise ValueError('S=%d samples are not n_segments=%d (even, >= 2) segments of seg_len=%d (>= 2)'
                             % (S, n_segments, seg_len))
        if batch_len is None:
            batch_len = int(np.floor(np.sqrt(seg_len)))
        batch_len = int(batch_len)
        if not 1 <= batch_len <= seg_len // 2:
            raise ValueError('batch_len=%d is not between 1 and seg_len // 2 = %d' % (batch_len, seg_len // 2))
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        re_ = np.ascontiguousarray(np.ravel(rhat_edges), dtype=np.float64)
        ee = np.ascontiguousarray(np.ravel(ess_edges), dtype=np.float64)
        if re_.size > 16 or ee.size > 16:
            raise ValueError('at most 16 edges per histogram')
        hist_rhat = np.zeros((self.T, re_.size + 1), dtype=np.uint64)
        hist_ess = np.zeros((self.T, ee.size + 1), dtype=np.uint64)
        node_rhat = np.zeros((self.T, self.N))
        node_ess = np.zeros((self.T, self.N))
        pw = np.zeros((self.T, self.N, self.N, 2)) if want_pointwise else None
        self._ck(self._L.dlsm_convergence_accumulate(
            self._h, _p(Xs), _p(b), _po(r), n_segments, seg_len, batch_len, _po(re_), int(re_.size), _po(ee),
            int(ee.size), _p(hist_rhat), _p(hist_ess), _p(node_rhat), _p(node_ess), _po(pw)))
        out = (hist_rhat, hist_ess, node_rhat, node_ess)
        return out + (pw,) if want_pointwise else out

    # -- PSIS-LOO (no reference counterpart) -----------------------------------------------------
    def loo_accumulate(self, bits, Xs, intercepts, radii=None, k_edges=(), want_pointwise=False):
        """Pareto-smoothed importance-sampling leave-one-out of every dyad of the packed network ``bits``
        over the S samples (arguments as ``ic_accumulate``), in one pass on the device
        (csrc/kernels_loo.hpp; the fit: csrc/psis_tail.hpp; the definition: include/dynetlsm_hip.h).
        Returns ``totals`` (T, 5) - per time step sum elpd_loo, sum elpd_loo^2, sum lppd, dyads, unfitted
        dyads -, ``hist_k`` (T, len(k_edges) + 1) uint64 - the bin of a Pareto shape k is the number of
        edges <= it, unfitted dyads (k = +inf) fall into the last one - and ``node_k_max`` (T, N), the
        largest k over the dyads of each node; ``want_pointwise``: also (T, N, N, 2), (elpd_loo, k) per
        dyad (undirected: i < j filled, the rest 0)."""
        bits = self._packed(bits, 'bits')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        ke = np.ascontiguousarray(np.ravel(k_edges), dtype=np.float64)
        if ke.size > 16:
            raise ValueError('at most 16 edges per histogram')
        totals = np.zeros((self.T, 5))
        hist_k = np.zeros((self.T, ke.size + 1), dtype=np.uint64)
        node_k = np.zeros((self.T, self.N))
        pw = np.zeros((self.T, self.N, self.N, 2)) if want_pointwise else None
        self._ck(self._L.dlsm_loo_accumulate(self._h, _p(bits), _p(Xs), _p(b), _po(r), int(S), _po(ke), int(ke.size),
                                             _p(totals), _p(hist_k), _p(node_k), _po(pw)))
        return (totals, hist_k, node_k, pw) if want_pointwise else (totals, hist_k, node_k)

    # -- posterior edge probabilities (no reference counterpart) ----------------------------------
    def proba_accumulate(self, bits, Xs, intercepts, radii, level, mask=None, n_bins=20,
                         width_edges=(0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5), pointwise=False):
        """Mean, standard deviation (ddof 1) and the equal-tailed credible interval at ``level`` of the edge
        probability of every dyad over the S >= 2 samples (arguments as ``score_accumulate``; ``radii`` None
        for undirected chains), and the calibration of the posterior mean against the packed network ``bits``
        over the dyads that ``mask`` does not exclude, in one pass on the device (csrc/kernels_proba.hpp; the
        definition: include/dynetlsm_hip.h).  Returns uint64 tables - ``calib`` (T, n_bins, 3): scored dyads,
        those with y = 1 and the sum of the mean in units of 2^-32 per bin of the mean; ``brier`` (T,):
        sum (y - mean)^2 in the same units; ``node_sums`` (T, N, 2): the mean of dyad (i, j) added to slot 0
        of i and slot 1 of j; ``hist_width`` (T, len(width_edges) + 1): the bin of upper - lower is the
        number of edges <= it - and, with ``pointwise``, (T, N, N, 4) = (mean, sd, lower, upper) of every
        dyad (undirected: i < j filled, the rest 0), else None."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError('level must lie in (0, 1), got %r' % (level,))
        n_bins = int(n_bins)
        if not 1 <= n_bins <= 64:
            raise ValueError('n_bins must be between 1 and 64, got %d' % n_bins)
        we = np.ascontiguousarray(np.ravel(width_edges), dtype=np.float64)
        if we.size > 16:
            raise ValueError('at most 16 edges per histogram')
        if not np.all(np.isfinite(we)) or np.any(np.diff(we) <= 0):
            raise ValueError('width_edges must be finite and ascending')
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        if np.shape(Xs)[0] < 2:
            raise ValueError('needs at least two samples (the standard deviation has ddof = 1)')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        calib = np.zeros((self.T, n_bins, 3), dtype=np.uint64)
        brier = np.zeros(self.T, dtype=np.uint64)
        node_sums = np.zeros((self.T, self.N, 2), dtype=np.uint64)
        hist_width = np.zeros((self.T, we.size + 1), dtype=np.uint64)
        pw = np.zeros((self.T, self.N, self.N, 4)) if pointwise else None
        self._ck(self._L.dlsm_proba_accumulate(
            self._h, _p(bits), _po(mask), _p(Xs), _p(b), _po(r), int(S), C.c_double(level), n_bins, _po(we),
            int(we.size), _p(calib), _p(brier), _p(node_sums), _p(hist_width), _po(pw)))
        return calib, brier, node_sums, hist_width, pw

    # -- link prediction (no reference counterpart) ------------------------------------------------
    TOPK_AMONG = ('non_ties', 'ties', 'observed', 'missing', 'all')

    def topk_accumulate(self, bits, Xs, intercepts, radii, k, among='non_ties', largest=True, mask=None,
                        max_candidates=None):
        """Per time step the ``k`` eligible dyads that come first by the posterior-mean edge probability over the
        S >= 2 samples (arguments as ``proba_accumulate``): probability descending, then i, then j; ``largest=False``:
        ascending, then i, then j.  Selected on the device without a (T, N, N) array or a sort of it
        (csrc/kernels_topk.hpp; the definition: include/dynetlsm_hip.h).  ``among``: ``'non_ties'`` - dyads that
        ``mask`` does not exclude with y = 0 in ``bits`` -, ``'ties'`` - not excluded, y = 1 -, ``'observed'`` - not
        excluded -, ``'missing'`` - the dyads that ``mask`` excludes - or ``'all'``.  The device returns every dyad
        that shares the rank key of the k-th or lies beyond it, at most ``max_candidates`` (default ``k + 2**20``)
        per time step, else ``EngineError`` with code -5; they are sorted here and cut to k.  Returns ``steps``, per
        time step a tuple (i, j, y, proba, sd) of arrays of min(k, eligible) entries in rank order, and ``diag``, a
        dict of (T,) int64 arrays: ``eligible``, ``n_beyond`` and ``n_at`` (dyads beyond and at the k-th key),
        ``key`` (-1: nothing eligible), ``tiles_revisited`` (tiles of the second pass), and ``n_tiles``, the tiles of
        a time step."""
        if among not in self.TOPK_AMONG:
            raise ValueError('among must be one of %s, got %r' % (', '.join(map(repr, self.TOPK_AMONG)), among))
        if int(k) != k or int(k) < 1:
            raise ValueError('k must be a positive integer, got %r' % (k,))
        k = int(k)
        if max_candidates is None:
            max_candidates = k + 2 ** 20
        if int(max_candidates) != max_candidates or int(max_candidates) < k:
            raise ValueError('max_candidates must be an integer >= k=%d, got %r' % (k, max_candidates))
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        elif among == 'missing':
            raise ValueError("among='missing' needs the mask of the missing dyads")
        if np.shape(Xs)[0] < 2:
            raise ValueError('needs at least two samples (the standard deviation has ddof = 1)')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        T, N = self.T, self.N
        dyads = N * (N - 1) // (1 if self.model != UNDIRECTED else 2)
        # no time step has more candidates than dyads: room beyond that (and beyond k) is never used
        room = min(int(max_candidates), max(k, dyads))
        index = np.zeros((T, room, 4), dtype=np.int32)
        value = np.zeros((T, room, 2))
        n_cand = np.zeros(T, dtype=np.int32)
        diag = np.zeros((T, 5), dtype=np.int64)
        self._ck(self._L.dlsm_topk_accumulate(
            self._h, _p(bits), _po(mask), _p(Xs), _p(b), _po(r), int(S), self.TOPK_AMONG.index(among),
            int(bool(largest)), C.c_int64(k), C.c_int64(room), _p(index), _p(value), _p(n_cand), _p(diag)))
        steps = [rank_candidates(index[t, :int(n_cand[t])], value[t, :int(n_cand[t])], k, largest) for t in range(T)]
        tile_rows = 32 if self.D <= 4 else 16
        n_rb, n_cb = -(-N // tile_rows), -(-N // 64)
        if self.model != UNDIRECTED:
            n_tiles = n_rb * n_cb
        else:
            n_tiles = sum(1 for bi in range(n_rb) for bj in range(n_cb) if bi * tile_rows < min(N, (bj + 1) * 64) - 1)
        return steps, dict(eligible=diag[:, 0].copy(), n_beyond=diag[:, 1].copy(), n_at=diag[:, 2].copy(),
                           key=diag[:, 3].copy(), tiles_revisited=diag[:, 4].copy(), n_tiles=n_tiles)

    # -- per-node link prediction (no reference counterpart) ----------------------------------------
    PARTNERS_K_MAX = 64

    def partners_accumulate(self, bits, Xs, intercepts, radii, k, among='non_ties', largest=True, mask=None,
                            rows=None):
        """For every time step and every node i the ``k`` <= 64 eligible partners j != i that come first by the
        posterior-mean edge probability of the dyad (i, j) over the S >= 2 samples (arguments and ``among`` as
        ``topk_accumulate``): probability descending - ``largest=False``: ascending -, then j.  Directed chains rank
        the receivers j of sender i; undirected chains read the network and the mask of {i, j} as ``topk_accumulate``
        does.  Each row's list is kept on the device while its columns stream by (csrc/kernels_partners.hpp; the
        definition: include/dynetlsm_hip.h): no (T, N, N) array is formed.  ``rows``: node ids; only the row blocks
        that hold them are computed, and every row that was not asked for comes back as padding.  Returns ``partner``
        (T, N, k) int64, padded with -1, ``proba`` and ``sd`` (T, N, k), padded with NaN, ``y`` (T, N, k) int64, the
        partners' bits of the network, padded with -1, and ``eligible`` (T, N) int64, the eligible partners of each
        row: -1 for the rows of blocks that were not computed."""
        if among not in self.TOPK_AMONG:
            raise ValueError('among must be one of %s, got %r' % (', '.join(map(repr, self.TOPK_AMONG)), among))
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= self.PARTNERS_K_MAX:
            raise ValueError('k must be an integer in 1..%d, the entries of a node\'s list, got %r'
                             % (self.PARTNERS_K_MAX, k))
        k = int(k)
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        elif among == 'missing':
            raise ValueError("among='missing' needs the mask of the missing dyads")
        if np.shape(Xs)[0] < 2:
            raise ValueError('needs at least two samples (the standard deviation has ddof = 1)')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        T, N = self.T, self.N
        blocks = None
        if rows is not None:
            rows = np.unique(check_node_ids(rows, N, 'rows'))
            blocks = np.ascontiguousarray(np.unique(rows // (32 if self.D <= 4 else 16)), dtype=np.int32)
        partner = np.zeros((T, N, k), dtype=np.int32)
        value = np.zeros((T, N, k, 2))
        y = np.zeros((T, N, k), dtype=np.int32)
        eligible = np.zeros((T, N), dtype=np.int32)
        self._ck(self._L.dlsm_partners_accumulate(
            self._h, _p(bits), _po(mask), _p(Xs), _p(b), _po(r), int(S), self.TOPK_AMONG.index(among),
            int(bool(largest)), k, _po(blocks), 0 if blocks is None else int(blocks.size), _p(partner), _p(value),
            _p(y), _p(eligible)))
        if rows is not None:
            # rows that share a block with an asked row were computed: they are padding all the same
            drop = np.ones(N, dtype=bool)
            drop[rows] = False
            partner[:, drop], y[:, drop], value[:, drop] = -1, -1, np.nan
            eligible[:, drop] = -1
        return (partner.astype(np.int64), np.ascontiguousarray(value[..., 0]), np.ascontiguousarray(value[..., 1]),
                y.astype(np.int64), eligible.astype(np.int64))

    # -- tie dynamics (no reference counterpart) ---------------------------------------------------
    def dynamics_accumulate(self, bits, Xs, intercepts, radii, min_count, mask=None, n_bins=20, pointwise=False):
        """The posterior change of the edge probability of every dyad between consecutive time steps over the
        S >= 2 samples (arguments as ``proba_accumulate``; the chain has T >= 2), in one pass on the device
        (csrc/kernels_dynamics.hpp; the definition: include/dynetlsm_hip.h).  A step u = t -> t + 1 of a dyad is
        scored when ``mask`` excludes it neither at t nor at t + 1.  Returns uint64 tables over the scored steps -
        ``transitions`` (T - 1, 4, 4): per observed class 2 y_t + y_{t+1} the dyads and the sums of the mean
        probability at t, at t + 1 and of the mean of their product, in units of 2^-32; ``hist_up`` (T - 1,
        n_bins): dyads per bin min(up * n_bins // S, n_bins - 1) of the number of samples in which the linear
        predictor rose; ``node_changes`` (T - 1, N, 4): dyad (i, j) that rose in at least ``min_count`` (1..S)
        samples adds 1 to slot 0 of i and slot 1 of j, one that fell in as many to slots 2 and 3;
        ``node_turnover`` (T - 1, N, 2): |mean change| in units of 2^-32 to slot 0 of i and slot 1 of j - and, with
        ``pointwise``, (T - 1, N, N, 4) = (delta_mean, delta_sd, prob_up, prob_down) of every dyad (undirected:
        i < j filled, the rest 0), else None."""
        if self.T < 2:
            raise ValueError('a step needs two time steps, the chain has T=%d' % self.T)
        n_bins = int(n_bins)
        if not 1 <= n_bins <= 64:
            raise ValueError('n_bins must be between 1 and 64, got %d' % n_bins)
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        if np.shape(Xs)[0] < 2:
            raise ValueError('needs at least two samples (the standard deviation has ddof = 1)')
        Xs, b, r, S = self._sample_args(Xs, intercepts, radii)
        if int(min_count) != min_count or not 1 <= int(min_count) <= S:
            raise ValueError('min_count must be an integer between 1 and S=%d, got %r' % (S, min_count))
        U = self.T - 1
        transitions = np.zeros((U, 4, 4), dtype=np.uint64)
        hist_up = np.zeros((U, n_bins), dtype=np.uint64)
        node_changes = np.zeros((U, self.N, 4), dtype=np.uint64)
        node_turnover = np.zeros((U, self.N, 2), dtype=np.uint64)
        pw = np.zeros((U, self.N, self.N, 4)) if pointwise else None
        self._ck(self._L.dlsm_dynamics_accumulate(
            self._h, _p(bits), _po(mask), _p(Xs), _p(b), _po(r), int(S), int(min_count), n_bins, _p(transitions),
            _p(hist_up), _p(node_changes), _p(node_turnover), _po(pw)))
        return transitions, hist_up, node_changes, node_turnover, pw

    # -- community structure of stored labellings (the reference: modularity of one labelling on the host) ----
    def community_accumulate(self, bits, zs, K, mask=None, batch=0, want_blocks=False):
        """Counts of the labellings ``zs`` (S, T, N), integers in [0, K), 1 <= K <= 256, against the packed network
        ``bits`` (``pack_network``; undirected chains: symmetric) without the excluded dyads ``mask`` (packed alike;
        undirected chains: either orientation excludes the dyad), in one pass on the device
        (csrc/kernels_community.hpp; the definition: include/dynetlsm_hip.h).  Every count is of ordered pairs.
        Returns int64 tables: ``clusters`` (S, T, K, 5) - per labelling and cluster its nodes, the ties inside it,
        its out-volume, its in-volume and the excluded ordered dyads inside it; ``node_within`` (T, N) - over the
        samples, a node's ties into its own cluster; ``node_switch`` (T - 1, N) - the samples in which the node's
        label changed; ``moved`` (S, T - 1) - the nodes whose label changed; and, with ``want_blocks``, ``blocks``
        (S, T, K, K, 2) - ties and excluded ordered dyads from cluster a to cluster b - else None.  The labels are
        staged ``batch`` samples at a time (0: automatic); no table depends on it."""
        K, batch = int(K), int(batch)
        if np.ndim(zs) != 3:
            raise ValueError('zs must be (S, T, N), got %d dimensions' % np.ndim(zs))
        zs = _i64(zs, (np.shape(zs)[0], self.T, self.N), 'zs')
        S = zs.shape[0]
        if S < 1:
            raise ValueError('needs at least one sample')
        if not 1 <= K <= 256:
            raise ValueError('n_components must be in 1..256 (labels are kept as bytes), got %d' % K)
        if batch < 0:
            raise ValueError('batch must not be negative, got %d' % batch)
        bits = self._packed(bits, 'bits')
        if mask is not None:
            mask = self._packed(mask, 'mask')
        U = self.T - 1
        clusters = np.zeros((S, self.T, K, 5), dtype=np.int64)
        node_within = np.zeros((self.T, self.N), dtype=np.int64)
        node_switch = np.zeros((U, self.N), dtype=np.int64)
        moved = np.zeros((S, U), dtype=np.int64)
        blocks = np.zeros((S, self.T, K, K, 2), dtype=np.int64) if want_blocks else None
        self._ck(self._L.dlsm_community_accumulate(
            self._h, _p(bits), _po(mask), _p(zs), S, K, batch, _p(clusters), _p(node_within), _po(node_switch),
            _po(moved), _po(blocks)))
        return clusters, node_within, node_switch, moved, blocks

    # -- multi-step posterior predictive forecasts (the reference: one step, undirected, on the host) ----
    def forecast_paths(self, X0, intercepts, radii=None, z0=None, trans=None, mu=None, sigma=None, lmbda=None,
                       sigma_sq=0.0, horizon=1, seed=0, first_index=0, batch=0, want_paths=False,
                       want_labels=False):
        """One trajectory of ``horizon`` future time steps per posterior sample, drawn and averaged on the
        device (csrc/kernels_forecast_paths.hpp).  ``X0`` (S, N, D): the samples' last time step;
        ``intercepts`` (S,) or (S, 2); ``radii`` (S, N) (directed and case-control chains).  With ``z0``
        (S, N) the mixture dynamics: ``trans`` (S, K, K) raw transition rows, ``mu`` (S, K, D), ``sigma``
        (S, K) variances, ``lmbda`` (S,); without it the random walk of variance ``sigma_sq``.  Sample s
        uses RNG index ``first_index + s``: results do not depend on how the samples are split across calls
        or on ``batch`` (samples per device batch, 0: automatic).  Returns ``(probas, paths, labels)``:
        (H, N, N) mean edge probabilities over the S samples, (S, H, N, D) positions if ``want_paths`` and
        (S, H, N) int32 labels if ``want_labels`` (mixture only), else None."""
        X0, S = self._samples(X0, (self.N, self.D), 'X0')
        H = int(horizon)
        if H != horizon or H < 1:
            raise ValueError('horizon must be a positive integer, got %r' % (horizon,))
        b, r = self._intercepts_radii(intercepts, radii, S)
        if z0 is None:
            if want_labels:
                raise ValueError('the random walk has no labels')
            K, z, w, m, sg, lm = 0, None, None, None, None, None
        else:
            if trans is None or mu is None or sigma is None or lmbda is None:
                raise ValueError('the mixture needs trans, mu, sigma and lmbda')
            w = np.ascontiguousarray(trans, dtype=np.float64)
            K = int(w.shape[-1])
            z = _i32(z0, (S, self.N), 'z0')
            w = _f64(w, (S, K, K), 'trans')
            m = _f64(mu, (S, K, self.D), 'mu')
            sg = _f64(sigma, (S, K), 'sigma')
            lm = _f64(np.ravel(lmbda), (S,), 'lmbda')
        probas = np.zeros((H, self.N, self.N))
        paths = np.zeros((S, H, self.N, self.D)) if want_paths else None
        labels = np.zeros((S, H, self.N), dtype=np.int32) if want_labels else None

        def ptr(a):
            return _p(a) if a is not None else None

        self._ck(self._L.dlsm_forecast_paths(
            self._h, _p(X0), _p(b), ptr(r), ptr(z), ptr(w), ptr(m), ptr(sg), ptr(lm), K, float(sigma_sq), H, int(S),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint32(int(first_index)), int(batch), _p(probas),
            ptr(paths), ptr(labels)))
        return probas, paths, labels

    def profile_enable(self, on=True):
        self._ck(self._L.dlsm_profile_enable(self._h, int(on)))

    def profile_read(self, kernel):
        ms = C.c_double(0.0)
        n = C.c_int(0)
        self._ck(self._L.dlsm_profile_read(self._h, int(kernel), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_read_eval_stamps(self):
        """(mean in-kernel duration in us, launches) of k_spec_eval while profiling"""
        us = C.c_double(0.0)
        n = C.c_int(0)
        self._ck(self._L.dlsm_profile_read_eval_stamps(self._h, C.byref(us), C.byref(n)))
        return us.value, n.value

    def timer_start(self):
        self._ck(self._L.dlsm_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_double(0.0)
        self._ck(self._L.dlsm_timer_stop(self._h, C.byref(ms)))
        return ms.value
