"""Record the reference's own ``modularity(Y, z, is_directed)`` (network_statistics.py:31-61) for two small
networks into tests/golden/community_modularity.npz: inputs and outputs only.

Usage:  python tests/golden/make_community_golden.py PATH_TO_THE_REFERENCE_CHECKOUT
The reference needs scikit-learn and ``np.int`` (aliased here, as make_golden.py does)."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    import sklearn.preprocessing  # noqa  (before the alias)
    import scipy.sparse  # noqa
    np.int = int
    pkg = types.ModuleType('dynetlsm_ref')
    pkg.__path__ = [os.path.join(ref, 'dynetlsm')]               # the two modules alone, not the package's __init__
    sys.modules['dynetlsm_ref'] = pkg
    stats = importlib.import_module('dynetlsm_ref.network_statistics')
    rng = np.random.RandomState(20)
    out = {}
    for tag, directed, T, N, K, p in (('u', False, 3, 12, 3, 0.3), ('d', True, 2, 15, 4, 0.2)):
        Y = (rng.rand(T, N, N) < p).astype(np.float64)
        if not directed:
            Y = np.triu(Y, 1) + np.triu(Y, 1).transpose(0, 2, 1)
        Y[:, np.arange(N), np.arange(N)] = 0
        z = rng.randint(0, K, size=(T, N))
        z[0][z[0] == 1] = 0                                      # a label that no node carries at t = 0
        out[tag + '_Y'], out[tag + '_z'] = Y, z
        out[tag + '_modularity'] = np.float64(stats.modularity(Y, z, is_directed=directed))
        out[tag + '_modularity_t'] = np.array([stats.static_modularity(Y[t], z[t], is_directed=directed)
                                               for t in range(T)])
    np.savez(os.path.join(HERE, 'community_modularity.npz'), **out)
    print({k: v for k, v in out.items() if 'modularity' in k})


if __name__ == '__main__':
    main(sys.argv[1])
