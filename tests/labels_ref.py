"""Host restatement of the label block update (sample_labels.py:134-190 as oracle/dynetlsm_oracle.c:
orc_sample_labels states it) in np.longdouble, vectorised over the nodes, with the engine's own Philox
uniforms (oracle.philox_uniform2, pure numpy); a Python restatement of the dispatch of capi.hip:
launch_sample_labels, which names the kernel form a shape reaches; the cases of
tests/test_gpu_labels_shapes.py; and long-double restatements of the T x K table (k_gauss_table) and of
oracle/hdp_sums.py with the rounding bounds those two comparisons use.  Written from the oracle's
statement of the update and independently of dynetlsm_amd/csrc/kernels_labels.hpp, whose constants
tests/test_labels_ref_cpu.py reads out of the sources and compares with the ones below.

TEST INFRASTRUCTURE ONLY.

Why labels are compared exactly
-------------------------------
A draw is the number of k with u total > cdf_k, i.e. with u > c_k = cdf_k / total.  ``margin`` is
min_k |u - c_k| over k < K - 1 (the last comparison, u total > total, is false for every u <= 1) in long
double.  The device's c_k differs from the exact one by at most ``bound`` (below); where margin > bound the
device and the reference draw the same label.  tests/test_labels_ref_cpu.py asserts margin >= 1e-9 and
bound <= 1e-11 for every draw of every case, so a label that differs is a kernel's mistake, not a tie.

The bound on the device's error in c_k, to first order in u = 2^-53.  Every quantity of the update is a
sum of products of non-negative numbers, so relative errors add and nothing cancels.

  * table.  log L[t][k] = lognorm_k - ss hiv_k with lognorm_k = -d/2 log(2 pi var_k), hiv_k = 0.5 (1 / var_k),
    ss = sum_j d_j^2, d_j = x_j - (lm m_j + (1 - lm) xp_j) (t = 0: x_j - m_j).  The mean of t > 0 carries
    u (2 |lm m_j| + 3 |(1 - lm) xp_j|) =: u B_j (the roundings of 1 - lm, of the two products and of the
    add), d_j that and u |d_j|; the square adds u d_j^2 and the d - 1 adds (d - 1) u ss:
        |delta(ss hiv)| <= u hiv (2 sum_j |d_j| B_j + (d + 2) ss) + 2 u ss hiv
    (the last term: the division and the product).  lognorm: one rounding in the logarithm's argument (u
    absolute, times d/2), the logarithm's ulp and the product: <= u (d + 3 |lognorm|).  The subtraction:
    u |log L|.  The exponential turns the argument's absolute error into a relative one and adds its own
    error, 1 ulp by the ROCm device-library's table, taken as 2 u:
        eL[t][k] = |delta arg| + 2 u.
    A fused multiply-add in place of a product and an add only removes roundings.  An entry below 2^-969 is
    subnormal on the device or close to it: eL = 1 (nothing is assumed of it; its weight below is < 1e-13).
  * backward step.  pm[t][k] = L[t][k] bm[t][k] (one rounding), bm[t-1][r] = sum_k w[t][r][k] pm[t][k] up to a
    factor common to all r (the wavefront kernel divides by the row's sum, the matrix-core kernel scales by a
    power of two: either cancels in c_k).  K products and adds in whatever order (a chain, or four at a time
    inside v_mfma_f64_16x16x4_f64) cost at most (K + 1) u relative; K + 6 is used, which leaves room for the
    division by the row's sum.  With H[t][k] the bound of pm[t][k] and G[t][r] that of bm[t][r]:
        H[t][k] = eL[t][k] + G[t][k] + u,   G[T-1] = 0,
        G[t-1][r] = sum_k w[t][r][k] pm[t][k] H[t][k] / sum_k w[t][r][k] pm[t][k] + (K + 6) u
    - the error of a sum of non-negative terms is the terms' errors weighted by the terms.
  * draw.  p_k = w[t][z_{t-1}][k] pm[t][k] (one rounding), cdf and total K - 1 adds each, u total one product:
        |delta c_k| <= sum_k p_k (H[t][k] + u) / total + 2 (K + 4) u = bound[t][node].
    (c_k = sum_{j <= k} p_j / total; with p_j (1 + e_j) in place of p_j it moves by
    (1 - c_k) sum_{j <= k} p_j e_j / total - c_k sum_{j > k} p_j e_j / total, at most sum_j p_j |e_j| / total.)

For the shapes here this is roughly ((T - 1)(K + 6) + K + 4 + 2 sum_t E|log L[t][z_t]|) u: 1e-14 to 1e-12.

The table of one node (k_gauss_table, ``table_bound``)
------------------------------------------------------
out[t][k] = exp(log L[t][k]) or, normalised, exp(log L[t][k] - max_k log L[t][k]).  The relative error is
|delta arg| + 2 u with delta arg as above; normalised, the maximum's own delta arg and the subtraction's
u |log L - max| come on top.  An entry may be subnormal in double, where the exponential's result is rounded a
second time when it is scaled down: 2^-1073, two of the smallest subnormal, is added.

The label sums (hdp_label_sums_wg, ``LabelSums``)
-------------------------------------------------
A thread adds the members among its ceil(N / 256) nodes in ascending order, block_sum_all adds the 64 lanes
of a wavefront in six levels and the four wavefronts in a chain of four: an element passes through at most
ceil(N / 256) + 10 adds, so |err| <= (ceil(N / 256) + 10) u sum_i |v_i| + sum_i |delta v_i|, v_i the node's
term and delta v_i its own rounding:
  stage 0  v = x - (1 - lm) xp:          u (2 |(1 - lm) xp| + |v|)
  stage 1  v = ss = sum_j r_j^2, r_j = x_j - (1 - lm) xp_j - lm mk_j:
           delta r_j = u (2 |(1 - lm) xp_j| + |x_j - (1 - lm) xp_j| + |lm mk_j| + |r_j|),
           delta ss = 2 sum_j |r_j| delta r_j + d u ss
  stage 2  v = sum_j dm_j dx_j / sk (and dm_j dm_j), dm = mk - xp, dx = x - xp:  (d + 3) u sum_j |dm_j dx_j| / sk
  stage 3  five summands (log w, two multiples of log sk, ss / sk / 2, b / sk / 2), each within 4 u of its
           value but for the share of delta ss, and four adds:  8 u sum |summand| + delta ss / (2 sk)
and never looser than the 1e-12 + 1e-12 |ref| of test_gpu_parity.py::test_hdp_label_sums_match_oracle.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as orc

LD = np.longdouble
assert np.finfo(LD).machep <= -63, 'np.longdouble has no 64-bit mantissa on this platform'
U = LD(2.0) ** -53
PI = LD(3.14159265358979323846)          # the double the kernels and the oracle multiply by

# ---- the dispatch (capi.hip: launch_sample_labels; kernels_labels.hpp) ----------------------------------------
LM_THREADS = 1024
LM_NODES = 8
LM_MAX_KS = 8
LM_WPRE = 6                              # passes of LM_THREADS transition-matrix entries requested up front
LAB_WAVES = 8
LC_THREADS = 1024
LC_PRE = 2                               # passes of LC_THREADS labels k_label_counts requests up front
MFMA_LDS_MAX = 150 * 1024
WAVE_TABLES_MAX = 160 * 1024
WAVE_W_LDS_MAX = 80 * 1024
HDP_THREADS = 256
HDP_NU = 4                               # nodes per thread and trip of hdp_label_sums_wg


def lm_ksteps(K):
    return (K + 3) // 4


def lm_wstride(K):
    return (4 * lm_ksteps(K)) | 1


def lm_stride(K):
    return 16 * ((lm_ksteps(K) + 3) // 4) + 1


def lm_lds_bytes(T, K, D):
    words = T * K * lm_wstride(K) + (T + 1) * LM_NODES * lm_stride(K) + LM_NODES * T + 2 * K
    return 8 * (words + (T * LM_NODES + K) * D)


def wave_lds_bytes(T, K):
    """(the nodes' tables, the padded transition matrices) of the wavefront-per-node kernel"""
    return LAB_WAVES * 2 * T * K * 8, T * K * (K | 1) * 8


def form(T, K, D):
    """the kernel a shape reaches: 'mfma KS=n', 'wave WLDS=1', 'wave WLDS=0' or 'refused'"""
    if K <= 4 * LM_MAX_KS and lm_lds_bytes(T, K, D) <= MFMA_LDS_MAX:
        return 'mfma KS=%d' % min(lm_ksteps(K), LM_MAX_KS)
    tables, w = wave_lds_bytes(T, K)
    if tables > WAVE_TABLES_MAX:
        return 'refused'
    return 'wave WLDS=%d' % (tables + w <= WAVE_W_LDS_MAX)


# ---- the cases ---------------------------------------------------------------------------------------------
SEED, CHAIN, LMBDA, ITERS = 11, 2, 0.7, (1, 2)


class Case(object):
    """a shape, the form it is listed for and the nodes moved far from every mean; ``seed`` draws the inputs"""

    def __init__(self, T, N, D, K, want, far=(), seed=None):
        self.T, self.N, self.D, self.K, self.want, self.far = T, N, D, K, want, tuple(far)
        self.seed = T * 131 + K if seed is None else seed

    @property
    def dims(self):
        return self.T, self.N, self.D, self.K

    def __repr__(self):
        return '%d-%d-%d-%d%s' % (self.T, self.N, self.D, self.K, '-far' if self.far else '')


def _ks_rows():
    """KS = 1..8 with three padded components and with none; T = 3..5; fewer than, exactly and more than one
    workgroup of 8 nodes; n_features walking 1..8"""
    rows = []
    for i, K in enumerate(k for ks in range(1, 9) for k in (4 * ks - 3, 4 * ks)):
        rows.append(Case(3 + i % 3, (7, 8, 9, 23)[i % 4], 1 + i % 8, K, 'mfma KS=%d' % lm_ksteps(K)))
    return rows


CASES = _ks_rows() + [
    Case(1, 9, 2, 16, 'mfma KS=4'),           # T = 1: no backward pass; one full column tile
    Case(2, 17, 2, 31, 'mfma KS=8'),          # T = 2: one step, nothing requested ahead; K = 31
    Case(13, 12, 2, 32, 'mfma KS=8'),         # the largest T at K = 32; staging past WPRE x 1024 doubles
    Case(14, 12, 2, 32, 'wave WLDS=0'),       # the other side of the matrix-core path's LDS limit
    Case(64, 10, 1, 3, 'mfma KS=1'),
    Case(65, 10, 1, 3, 'mfma KS=1'),
    Case(129, 10, 1, 3, 'wave WLDS=1'),       # uniforms in three passes of 64; one trip of clamped reads
    Case(3, 20, 2, 33, 'wave WLDS=1'),        # trips of 8: K not a multiple
    Case(3, 20, 3, 40, 'wave WLDS=1'),        # a multiple
    Case(3, 20, 2, 63, 'wave WLDS=0'),
    Case(20, 11, 2, 64, 'wave WLDS=0'),       # the largest T K; K K + K > 1024 counters
    Case(5, 2100, 2, 3, 'mfma KS=1'),         # k_label_counts past its two prefetched passes
    Case(4, 12, 2, 7, 'mfma KS=2', far=(0, 5, 11)),
    Case(3, 12, 2, 40, 'wave WLDS=1', far=(0, 5, 11), seed=7001),
]
REFUSED = Case(21, 11, 2, 64, 'refused')
FAR_LOW, FAR_HIGH = -650.0, -500.0         # every (t, node): max_k log L >= FAR_LOW; some: <= FAR_HIGH


def _log_table64(X, mu, sigma, lmbda):
    """float64 log L (T, N, K), for placing the far nodes"""
    mean = np.broadcast_to(mu[None, None], X.shape[:2] + mu.shape).copy()
    mean[1:] = lmbda * mu[None, None] + (1 - lmbda) * X[:-1, :, None, :]
    ss = ((X[:, :, None, :] - mean) ** 2).sum(-1)
    return -0.5 * X.shape[2] * np.log(2 * np.pi * sigma) - ss * (0.5 / sigma)


def inputs(case):
    """X, mu, sigma, w drawn as the label tests of test_gpu_parity.py draw them; the far nodes sit at one point
    at every time, on the diagonal, at the smallest distance (steps of 1/4) where max_k log L[0] <= -560"""
    T, N, D, K = case.dims
    rng = np.random.RandomState(case.seed)
    mu = rng.randn(K, D) * 2
    sg = rng.uniform(0.2, 1.0, K)
    X = mu[rng.randint(0, K, size=(T, N))] + 0.5 * rng.randn(T, N, D)
    w = rng.dirichlet(np.ones(K), size=(T, K))
    for q, i in enumerate(case.far):
        e = np.ones(D) / np.sqrt(D) * (1 if q % 2 == 0 else -1)
        for r in np.arange(20.0, 120.0, 0.25):
            X[:, i] = r * e
            if _log_table64(X[:1, i:i + 1], mu, sg, LMBDA).max() <= -560.0:
                break
    return X, mu, sg, w


# ---- the table ---------------------------------------------------------------------------------------------
def log_table(X, mu, sigma, lmbda):
    """log L (T, N, K) in long double, the expression of gaussian_likelihood_fast.pyx:17-49, and the bound
    |delta arg| (in units of 1) on the error of the device's double evaluation of it (module docstring)"""
    X, mu, sigma, lm = LD(X), LD(mu), LD(sigma), LD(lmbda)
    T, N, D = X.shape
    mean = np.empty((T, N, sigma.shape[0], D), dtype=LD)
    mean[0] = mu[None]
    mean[1:] = lm * mu[None, None] + (1 - lm) * X[:-1, :, None, :]
    B = np.zeros_like(mean)
    B[1:] = 2 * np.abs(lm * mu[None, None]) + 3 * np.abs((1 - lm) * X[:-1, :, None, :])
    d = X[:, :, None, :] - mean
    ss = np.zeros(d.shape[:3], dtype=LD)
    for j in range(D):
        ss += d[..., j] * d[..., j]
    hiv = 0.5 * (1 / sigma)
    lognorm = -0.5 * D * np.log(2 * PI * sigma)
    logL = lognorm - ss * hiv
    darg = U * (hiv * (2 * (np.abs(d) * B).sum(-1) + (D + 2) * ss) + 2 * ss * hiv + D + 3 * np.abs(lognorm)
                + np.abs(logL))
    return logL, darg


def table(X_node, mu, sigma, lmbda, normalize):
    """the T x K table of one node (X_node (T, D)) as Chain.gaussian_likelihood returns it, in long double, and
    the per-entry absolute bound of the module docstring"""
    logL, darg = log_table(np.asarray(X_node)[:, None, :], mu, sigma, lmbda)
    logL, darg = logL[:, 0], darg[:, 0]
    rel = darg + 2 * U
    if normalize:
        top = logL.argmax(axis=1)[:, None]
        m = np.take_along_axis(logL, top, 1)
        rel = rel + np.take_along_axis(darg, top, 1) + U * np.abs(logL - m)
        logL = logL - m
    ref = np.exp(logL)
    return ref, rel * ref + LD(2.0) ** -1073


# ---- the block update ----------------------------------------------------------------------------------------
def uniforms(T, N, it, seed=SEED, chain=CHAIN):
    """(T, N): the engine's uniform of (node, t) at iteration ``it``"""
    u = orc.philox_uniform2(seed, np.arange(N)[None, :], np.arange(T)[:, None], it,
                            orc.stream_word(chain, orc.STREAM_LABELS))[0]
    return LD(u)


class Update(object):
    """The block update of one case: the table and the backward messages once (they do not depend on the
    iteration), the draws per iteration."""

    def __init__(self, X, mu, sigma, lmbda, w):
        self.T, self.N, self.D = X.shape
        self.K = K = sigma.shape[0]
        self.w = w = LD(w)
        T, N = self.T, self.N
        logL, darg = log_table(X, mu, sigma, lmbda)
        self.logL = logL
        L = np.exp(logL)
        eL = np.where(L < LD(2.0) ** -969, LD(1.0), darg + 2 * U)
        self.pm = pm = np.empty((T, N, K), dtype=LD)
        self.H = H = np.empty((T, N, K), dtype=LD)
        bm = np.ones((N, K), dtype=LD)
        G = np.zeros((N, K), dtype=LD)
        for t in range(T - 1, 0, -1):
            pm[t] = L[t] * bm
            H[t] = eL[t] + G + U
            wpm = w[t][None, :, :] * pm[t][:, None, :]            # [node][r][k]
            s = wpm.sum(axis=2)
            G = (wpm * H[t][:, None, :]).sum(axis=2) / s + (K + 6) * U
            bm = s / s.sum(axis=1, keepdims=True)
        pm[0] = L[0] * bm
        H[0] = eL[0] + G + U

    def _step(self, t, zprev, u):
        """labels, margins and bounds of time t given the labels of t - 1"""
        K = self.K
        wrow = self.w[0, 0][None, :] if t == 0 else self.w[t][zprev]
        p = wrow * self.pm[t]
        cdf = np.cumsum(p, axis=1)
        total = cdf[:, -1]
        z = (u[:, None] * total[:, None] > cdf).sum(axis=1)
        if K > 1:
            margin = np.abs(u[:, None] - cdf[:, :-1] / total[:, None]).min(axis=1)
        else:
            margin = np.ones(self.N, dtype=LD)
        bound = (p * (self.H[t] + U)).sum(axis=1) / total + 2 * (K + 4) * U
        return z, margin, bound

    def draw(self, it, seed=SEED, chain=CHAIN):
        T, N, K = self.T, self.N, self.K
        u = uniforms(T, N, it, seed, chain)
        z = np.zeros((T, N), dtype=np.int64)
        margin = np.empty((T, N), dtype=LD)
        bound = np.empty((T, N), dtype=LD)
        for t in range(T):
            z[t], margin[t], bound[t] = self._step(t, z[t - 1] if t else None, u[t])
        n, nk = counts(z, K)
        return SimpleNamespace(z=z, n=n, nk=nk, margin=margin, bound=bound, u=u,
                               max_abs_logL=float(np.abs(self.logL).max()))

    def explain(self, z_dev, it, seed=SEED, chain=CHAIN):
        """Teacher-forced: at every (t, node) the label the reference draws given the device's label of t - 1.
        Returns None when the device's labels are those, else (node, t, device label, reference label, margin,
        number of draws that differ) for the first node that leaves the reference and its first such time."""
        T, N = self.T, self.N
        u = uniforms(T, N, it, seed, chain)
        z_dev = np.asarray(z_dev)
        want = np.empty((T, N), dtype=np.int64)
        margin = np.empty((T, N), dtype=LD)
        for t in range(T):
            zprev = np.clip(z_dev[t - 1], 0, self.K - 1) if t else None
            want[t], margin[t], _ = self._step(t, zprev, u[t])
        bad = want != z_dev
        if not bad.any():
            return None
        node = int(np.flatnonzero(bad.any(axis=0))[0])
        t = int(np.flatnonzero(bad[:, node])[0])
        return node, t, int(z_dev[t, node]), int(want[t, node]), float(margin[t, node]), int(bad.sum())


def counts(z, K):
    """n[0][0][k] initial labels, n[t][j][k] transitions j -> k into time t, nk[t][k] labels in use"""
    T = z.shape[0]
    n = np.zeros((T, K, K))
    nk = np.zeros((T, K), dtype=np.int64)
    np.add.at(n[0, 0], z[0], 1)
    for t in range(1, T):
        np.add.at(n[t], (z[t - 1], z[t]), 1)
    for t in range(T):
        nk[t] = np.bincount(z[t], minlength=K)
    return n, nk


@functools.lru_cache(maxsize=None)
def update(case):
    """(inputs, Update) of a case, computed once and shared by the tests; read only"""
    X, mu, sg, w = inputs(case)
    for a in (X, mu, sg, w):
        a.setflags(write=False)
    return (X, mu, sg, w), Update(X, mu, sg, LMBDA, w)


@functools.lru_cache(maxsize=None)
def reference(case, it):
    return update(case)[1].draw(it)


# ---- the label sums (oracle/hdp_sums.py in long double) --------------------------------------------------------
class LabelSums(object):
    """``stage(s, ...)`` returns (sums, bound): the sums over the members of label k at time t of the node terms
    of oracle/hdp_sums.py (mean, residual, lam, logp) and the rounding bound of the module docstring"""

    def __init__(self, X, z, K):
        self.X, self.z, self.K = LD(X), np.asarray(z), int(K)
        self.T, self.N, self.D = self.X.shape

    def _by_label(self, V, dV):
        T, K, N = self.T, self.K, self.N
        member = self.z[:, :, None] == np.arange(K)[None, None, :]          # [t][i][k]
        shape = (T, N, K) + (1,) * (V.ndim - 2)
        m = member.reshape(shape)
        Vk, dVk = V[:, :, None], dV[:, :, None]
        ref = np.where(m, Vk, LD(0)).sum(axis=1)
        adds = -(-N // HDP_THREADS) + 10
        bound = adds * U * np.where(m, np.abs(Vk), LD(0)).sum(axis=1) + np.where(m, dVk, LD(0)).sum(axis=1)
        return ref, np.minimum(bound, LD(1e-12) + LD(1e-12) * np.abs(ref))

    def _residual(self, mu, lm):
        """r (T, N, D), ss (T, N) and delta ss"""
        X, z = self.X, self.z
        mz = mu[z]
        r = X - mz
        dr = U * np.abs(r)
        a = X[1:] - (1 - lm) * X[:-1]
        r[1:] = a - lm * mz[1:]
        dr[1:] = U * (2 * np.abs((1 - lm) * X[:-1]) + np.abs(a) + np.abs(lm * mz[1:]) + np.abs(r[1:]))
        ss = (r * r).sum(axis=2)
        return r, ss, 2 * (np.abs(r) * dr).sum(axis=2) + self.D * U * ss

    def stage(self, s, mu=None, sigma=None, lmbda=0.0, w=None, a=0.0, b=0.0):
        X, z, D = self.X, self.z, self.D
        lm = LD(lmbda)
        mu = None if mu is None else LD(mu)
        sigma = None if sigma is None else LD(sigma)
        if s == 0:
            V = X.copy()
            V[1:] = X[1:] - (1 - lm) * X[:-1]
            dV = U * np.abs(V)
            dV[1:] += 2 * U * np.abs((1 - lm) * X[:-1])
            out, bound = self._by_label(V, dV)
            return (out, bound) if D > 1 else (out[..., 0], bound[..., 0])
        if s == 1:
            _, ss, dss = self._residual(mu, lm)
            return self._by_label(ss, dss)
        if s == 2:
            V = np.zeros((self.T, self.N, 2), dtype=LD)
            dV = np.zeros_like(V)
            dm = mu[z[1:]] - X[:-1]
            dx = X[1:] - X[:-1]
            sz = sigma[z[1:]]
            V[1:, :, 0] = (dm * dx).sum(axis=2) / sz
            V[1:, :, 1] = (dm * dm).sum(axis=2) / sz
            dV[1:, :, 0] = (D + 3) * U * np.abs(dm * dx).sum(axis=2) / sz
            dV[1:, :, 1] = (D + 3) * U * (dm * dm).sum(axis=2) / sz
            return self._by_label(V, dV)
        w = LD(w)
        _, ss, dss = self._residual(mu, lm)
        sz = sigma[z]
        lw = np.empty(z.shape, dtype=LD)
        lw[0] = np.log(w[0, 0, z[0]])
        if self.T > 1:
            lw[1:] = np.log(w[np.arange(1, self.T)[:, None], z[:-1], z[1:]])
        parts = [lw, -0.5 * np.log(sz), -0.5 * ss / sz, -(0.5 * LD(a) + 1) * np.log(sz), -0.5 * LD(b) / sz]
        V = sum(parts[1:], parts[0])
        dV = 8 * U * sum(np.abs(p) for p in parts) + 0.5 * dss / sz
        return self._by_label(V, dV)


SUMS_CASES = [(2, 1030, 3, 5), (2, 2100, 2, 3)]       # past one trip of HDP_NU x HDP_THREADS nodes; past two


def sums_inputs(T, N, D, K, variant):
    """X, z, mu, sigma, w of a label-sums case; ``variant``: 'random' (every label has members), 'empty' (label
    K - 1 has none), 'one' (every node on label 1)"""
    rng = np.random.RandomState(T * 1000 + N)
    X = rng.randn(T, N, D)
    z = rng.randint(0, K, size=(T, N)).astype(np.int64)
    mu, sigma = rng.randn(K, D), rng.gamma(2.0, 1.0, size=K) + 0.1
    w = rng.dirichlet(np.ones(K), size=(T, K))
    if variant == 'empty':
        z = z % (K - 1)
    elif variant == 'one':
        z[:] = 1
    return X, z, mu, sigma, w
