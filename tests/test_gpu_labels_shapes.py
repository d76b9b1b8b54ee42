"""The label kernels (csrc/kernels_labels.hpp, csrc/kernels_hdp.hpp, the counts role of
csrc/kernels_hdploop.hpp) through ``Chain.sample_labels``, ``gaussian_likelihood``, ``hdp_label_sums`` and the
device-resident loop at the smallest shapes that cross each of their structural switches, draw for draw
against the long-double replica tests/labels_ref.py.  tests/test_labels_ref_cpu.py pins that replica to the
oracle, shows that each case reaches the form it is listed for, and establishes why labels are compared
exactly: every draw of every case lies >= 1e-9 from a cumulative probability and the device's error there is
<= 1e-11 (derived in labels_ref's docstring), so no draw is a tie.  Needs an MI355X: -m gpu.

Cases are (T, N, D, K); the form is decided by capi.hip: launch_sample_labels from the shape alone.

  switch                                                     crossed by
  ---------------------------------------------------------  --------------------------------------------------
  k_sample_labels_mfma<KS>, KS = 1..8, with three padded     K = 4 KS - 3 and K = 4 KS: K = 1, 4, 5, 8, ..., 29,
  components and with none                                   32; T = 3..5; N = 7, 8, 9, 23 (fewer than, exactly
                                                             and more than one workgroup of 8 nodes, a ragged
                                                             last one); D walking 1..8
  the second column tile's first column; the j < K guard of  K = 16, 17 above and (1, 9, 2, 16); (2, 17, 2, 31)
  the B operand
  T = 1 (no backward pass), T = 2 (one step, nothing         (1, 9, 2, 16), (2, 17, 2, 31)
  requested ahead) on the matrix cores
  the transition matrices staged past the WPRE x 1024        (13, 12, 2, 32): T K WS = 13728; the K <= 5 rows
  prefetched doubles, and within the first 1024
  the LDS limit of the matrix-core path, both sides          (13, 12, 2, 32): mfma KS=8 at 141 KB, the largest T
                                                             that does; (14, 12, 2, 32): wave WLDS=0
  long series on the matrix cores; the wavefront kernel's    (64, 10, 1, 3), (65, 10, 1, 3): mfma;
  uniforms in three passes of 64, K < 8: one trip of         (129, 10, 1, 3): wave WLDS=1
  clamped reads
  the wavefront kernel's trips of 8 at K not a multiple of   (3, 20, 2, 33), (3, 20, 3, 40): WLDS=1;
  8, a multiple, 63 and 64; WLDS both ways; the largest      (3, 20, 2, 63), (20, 11, 2, 64): WLDS=0, 160 KB of
  T K, LDS attribute above 64 KB                             tables
  the refusal above it                                       (21, 11, 2, 64): EngineError, no labels written
  k_label_counts past its two prefetched passes of 1024;     (5, 2100, 2, 3); (20, 11, 2, 64)
  K K + K > 1024 counters
  likelihoods near the bottom of the double range: some      (4, 12, 2, 7) far: mfma KS=2; (3, 12, 2, 40) far:
  (t, node) with max_k log L <= -500, all >= -650            wave WLDS=1 (three nodes 30 to 40 away from every mean)
  k_gauss_table at K = 1, K = 64, T = 1; first, last and a   test_table_of_one_node
  far node (entries that underflow); both normalisations
  hdp_label_sums_wg past one trip of 4 x 256 nodes, and      (2, 1030, 3, 5), (2, 2100, 2, 3): every label in use,
  past two                                                   a label without members, all nodes on one label
  hdp_counts_tables_wg past one trip of 8 x 256 labels, a    test_device_loop_past_2048_nodes
  trace row split over its groups

Labels and counts are compared with assert_array_equal, every draw of both iterations.  The table and the label
sums are held to the rounding bounds derived in labels_ref's docstring; the largest err / bound seen on an
MI355X: table 0.385 (unnormalised), 0.342 (normalised), both at (20, 11, 2, 64); label sums 0.018 (stage 0),
0.044 (stage 1), 0.053 (stage 2), 0.097 (stage 3).  The whole file takes 4 s.
"""
import numpy as np
import pytest

import labels_ref as lr
from test_gpu_hdp_loop import _run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import dynetlsm_amd
    return dynetlsm_amd


def _chain(eng, case, X, mu, sg):
    T, N, D, K = case.dims
    c = eng.Chain(T, N, D, 'undirected', seed=lr.SEED, chain_id=lr.CHAIN)
    c.set_positions(X)
    c.set_prior_mixture(mu, sg, lr.LMBDA, np.zeros((T, N), dtype=np.int64))
    return c


def _assert_labels(case, up, it, z, n, nk):
    ref = lr.reference(case, it)
    if not np.array_equal(z, ref.z):
        node, t, got, want, margin, n_bad = up.explain(z, it)
        pytest.fail('%r (%s) iteration %d: node %d at t = %d drew %d, the reference %d; |u - cdf / total| = %.3e '
                    'there (a tie needs < 1e-11); %d draws leave the reference given the device\'s previous label, '
                    '%d labels differ' % (case, case.want, it, node, t, got, want, margin, n_bad,
                                          int((z != ref.z).sum())))
    np.testing.assert_array_equal(z, ref.z)
    np.testing.assert_array_equal(n, ref.n)
    np.testing.assert_array_equal(nk, ref.nk)


@pytest.mark.parametrize('case', lr.CASES, ids=repr)
def test_labels_and_counts_draw_for_draw(eng, case):
    (X, mu, sg, w), up = lr.update(case)
    with _chain(eng, case, X, mu, sg) as c:
        first = {}
        for it in lr.ITERS:
            z, n, nk = first[it] = c.sample_labels(it, w)
            _assert_labels(case, up, it, z, n, nk)
        # the same iteration again: the same bits, whatever was drawn in between
        for a, b in zip(c.sample_labels(lr.ITERS[0], w), first[lr.ITERS[0]]):
            np.testing.assert_array_equal(a, b)


def test_refused_above_the_largest_table(eng):
    case = lr.REFUSED
    T, N, D, K = case.dims
    X, mu, sg, w = lr.inputs(case)
    z0 = np.random.RandomState(3).randint(0, K, size=(T, N)).astype(np.int64)
    # the labels the chain holds decide the mixture prior of a node: they are what they were after the refusal
    with eng.Chain(T, N, D, 'undirected', seed=lr.SEED, chain_id=lr.CHAIN) as c:
        c.upload_network(np.zeros((T, N, N))); c.set_positions(X); c.set_intercepts([0.0])
        c.set_prior_mixture(mu, sg, lr.LMBDA, z0)
        before = [c.loglik_partial(t, i, with_prior=True) for t, i in ((0, 0), (T - 1, N - 1), (7, 4))]
        with pytest.raises(eng.EngineError) as e:
            c.sample_labels(1, w)
        assert e.value.code == -5                   # DLSM_E_LIMIT
        after = [c.loglik_partial(t, i, with_prior=True) for t, i in ((0, 0), (T - 1, N - 1), (7, 4))]
        assert before == after
        z1 = z0.copy()
        z1[7, 4] = (z1[7, 4] + 1) % K
        c.set_prior_mixture(mu, sg, lr.LMBDA, z1)
        assert c.loglik_partial(7, 4, with_prior=True) != before[2]      # (the probe does see a label change)


TABLE_CASES = [lr.CASES[0], next(c for c in lr.CASES if c.K == 64), next(c for c in lr.CASES if c.T == 1)]


@pytest.mark.parametrize('case', TABLE_CASES, ids=repr)
def test_table_of_one_node(eng, case):
    """k_gauss_table against the long-double table within the per-entry bound of labels_ref's docstring; the far
    node sits 60 away from the origin in every coordinate: entries that are 0 in double are below 2^-1022"""
    assert TABLE_CASES[0].K == 1
    T, N, D, K = case.dims
    X, mu, sg, w = lr.inputs(case)
    far = N // 2
    X[:, far] = 60.0
    worst = {False: 0.0, True: 0.0}
    zeros = 0
    with _chain(eng, case, X, mu, sg) as c:
        for node in (0, far, N - 1):
            for normalize in (False, True):
                got = c.gaussian_likelihood(node, normalize)
                ref, bound = lr.table(X[:, node], mu, sg, lr.LMBDA, normalize)
                err = np.abs(got.astype(lr.LD) - ref)
                worst[normalize] = max(worst[normalize], float((err / bound).max()))
                assert (err <= bound).all(), (node, normalize, float((err / bound).max()))
                assert (ref[got == 0] < lr.LD(2.0) ** -1022).all()
                zeros += int((got == 0).sum())
                if normalize:
                    assert (got.max(axis=1) == 1.0).all()
    print('%r table: max err / bound %.3f (unnormalised) %.3f (normalised); %d entries underflow'
          % (case, worst[False], worst[True], zeros))
    assert zeros > 0


@pytest.mark.parametrize('variant', ['random', 'empty', 'one'])
@pytest.mark.parametrize('dims', lr.SUMS_CASES, ids=str)
def test_label_sums_past_one_trip(eng, dims, variant):
    T, N, D, K = dims
    X, z, mu, sigma, w = lr.sums_inputs(T, N, D, K, variant)
    lm, a, b = 0.83, 2.0, 1.3
    sums = lr.LabelSums(X, z, K)
    empty = np.stack([np.bincount(z[t], minlength=K) == 0 for t in range(T)])
    assert empty.any() == (variant != 'random')
    with eng.Chain(T, N, D, 'undirected') as c:
        c.set_positions(X)
        c.set_prior_mixture(mu, sigma, lm, z)
        got = [c.hdp_label_sums(0, lmbda=lm), c.hdp_label_sums(1, mu=mu, lmbda=lm),
               c.hdp_label_sums(2, mu=mu, sigma=sigma),
               c.hdp_label_sums(3, mu=mu, sigma=sigma, lmbda=lm, w=w, a=a, b=b)]
    want = [sums.stage(0, lmbda=lm), sums.stage(1, mu=mu, lmbda=lm), sums.stage(2, mu=mu, sigma=sigma),
            sums.stage(3, mu=mu, sigma=sigma, lmbda=lm, w=w, a=a, b=b)]
    ratios = []
    for stage, (g, (ref, bound)) in enumerate(zip(got, want)):
        assert g.shape == ref.shape
        assert (g[empty] == 0).all(), stage                 # a label without members: exactly 0
        err = np.abs(g.astype(lr.LD) - ref)
        live = bound > 0
        assert (err[~live] == 0).all(), stage
        ratios.append(float((err[live] / bound[live]).max()))
        assert (err <= bound).all(), (stage, ratios[-1])
    print('label sums %s %s: max err / bound by stage %s' % (dims, variant, ' '.join('%.3f' % r for r in ratios)))


def test_device_loop_past_2048_nodes(eng):
    """hdp_counts_tables_wg takes its second trip of 8 x 256 labels and files a trace row split over its groups;
    hdp_label_sums_wg its third of 4 x 256 nodes: labels, counts, tables and the trace iteration by iteration
    against the oracle (test_gpu_hdp_loop._run_both)"""
    _run_both(eng, 2, 2100, 3, 31, n_it=2)
