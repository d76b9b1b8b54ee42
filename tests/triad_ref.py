"""numpy references of the triad census, written from the definitions (Holland and Leinhardt's MAN classes
in the convention of sna and networkx) and not from dynetlsm_amd/gof.py: a brute-force census over all
i < j < k, and a replica of the engine's (c, a, b) records (include/dynetlsm_hip.h,
dlsm_gof_triads_simulate), for tests."""
import functools
import itertools

import numpy as np

NAMES = ('003', '012', '102', '021D', '021U', '021C', '111D', '111U', '030T', '030C', '201', '120D', '120U',
         '120C', '210', '300')
R = 51


def classify(A):
    """the MAN class name of the 3 x 3 boolean adjacency matrix ``A``, from the definitions: the counts of
    mutual, asymmetric and null dyads, then the letter by the shape of the asymmetric arcs"""
    pairs = ((0, 1), (0, 2), (1, 2))
    m = sum(1 for x, y in pairs if A[x, y] and A[y, x])
    a = sum(1 for x, y in pairs if A[x, y] != A[y, x])
    n = 3 - m - a
    man = '%d%d%d' % (m, a, n)
    asym = [(x, y) for x in range(3) for y in range(3) if x != y and A[x, y] and not A[y, x]]
    out_a = [sum(1 for x, _ in asym if x == v) for v in range(3)]      # asymmetric arcs sent by v
    in_a = [sum(1 for _, y in asym if y == v) for v in range(3)]       # ... received by v
    if man == '021':
        # two arcs: Down from one node, Up into one node, or a Chain
        return man + ('D' if max(out_a) == 2 else 'U' if max(in_a) == 2 else 'C')
    if man == '111':
        # a mutual pair and one arc between the third node and one of the pair.  D: the arc points into
        # the pair (A <-> B <- C), U: it points out of it (A <-> B -> C)
        (x, y), = asym
        mutual = [v for v in range(3) if any(A[v, u] and A[u, v] for u in range(3) if u != v)]
        return man + ('D' if y in mutual else 'U')
    if man == '030':
        return man + ('C' if max(out_a) == 1 and max(in_a) == 1 else 'T')
    if man == '120':
        # a mutual pair and two arcs at the third node: both from it (Down), both into it (Up), or a Chain
        return man + ('D' if max(out_a) == 2 else 'U' if max(in_a) == 2 else 'C')
    return man


def _class_of_code():
    """class index of every labelled triad, by its six arc bits in the order (0,1) (1,0) (0,2) (2,0) (1,2) (2,1)"""
    arcs = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))
    out = np.zeros(64, dtype=np.int64)
    for code in range(64):
        A = np.zeros((3, 3), dtype=bool)
        for bit, (x, y) in enumerate(arcs):
            A[x, y] = (code >> bit) & 1
        out[code] = NAMES.index(classify(A))
    return out


CLASS_OF_CODE = _class_of_code()


@functools.lru_cache(maxsize=4)
def _triples(N):
    return np.array(list(itertools.combinations(range(N), 3)), dtype=np.int64).T


def census(Y):
    """(T, N, N) 0/1 -> (T, 16) int64: the class of every triple i < j < k, one by one (vectorised over the
    triples; O(N^3) memory, fine up to N of about 200)"""
    Y = (np.asarray(Y) != 0)
    T, N, _ = Y.shape
    out = np.zeros((T, 16), dtype=np.int64)
    if N < 3:
        return out
    i, j, k = _triples(N)
    for t in range(T):
        A = Y[t].astype(np.int64)
        code = (A[i, j] | A[j, i] << 1 | A[i, k] << 2 | A[k, i] << 3 | A[j, k] << 4 | A[k, j] << 5)
        out[t] = np.bincount(CLASS_OF_CODE[code], minlength=16)
    return out


def records(Y):
    """(T, N, N) 0/1 -> (T, 51) int64, the engine's records: over the pairs i < j with an arc between them,
    of dyad code c = Y[i,j] + 2 Y[j,i], the number of third nodes k in state a = Y[i,k] + 2 Y[k,i],
    b = Y[j,k] + 2 Y[k,j] at [(c - 1) * 16 + a * 4 + b], and the number of pairs of code c at [48 + c - 1]"""
    Y = (np.asarray(Y) != 0)
    T, N, _ = Y.shape
    out = np.zeros((T, R), dtype=np.int64)
    for t in range(T):
        A = Y[t].astype(np.int64)
        code = A + 2 * A.T                                 # code[i, k] = Y[i,k] + 2 Y[k,i]
        for i, j in zip(*np.nonzero(np.triu(code, 1))):
            c = code[i, j]
            third = np.ones(N, dtype=bool)
            third[[i, j]] = False
            out[t, (c - 1) * 16:c * 16] += np.bincount(code[i, third] * 4 + code[j, third], minlength=16)
            out[t, 48 + c - 1] += 1
    return out


def random_network(rng, T, N, directed, density):
    Y = rng.rand(T, N, N) < density
    idx = np.arange(N)
    Y[:, idx, idx] = False
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y | Y.swapaxes(1, 2)
    return Y
