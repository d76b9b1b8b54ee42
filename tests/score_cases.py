"""The inputs that tests/test_scores_cpu.py and tests/test_gpu_scores.py share: the shape grid of the
in-sample scores, drawn as ``_case`` of tests/test_gpu_ic.py draws its inputs, and the references of
tests/score_ref.py, computed once per case.

The seeds are chosen so that the precondition of the exact comparison holds for every scored dyad: the
rank key of pbar (1 - 1e-12) equals that of pbar (1 + 1e-12) (a bin is 3e-5 wide in relative terms, so at
these sizes about one seed in a thousand fails; ``find_seed`` is how they were picked)."""
import functools

import numpy as np

import score_ref
from test_gpu_ic import _case

# N: below a tile, one past a 32-bit word, no multiple of a tile dimension, more than one row block;
# D <= 4 and D > 4 take the two tile plans.  (N, T, D, S, directed, masked, seed)
CASES = [
    (5, 1, 1, 1, False, False, 0),
    (5, 3, 2, 7, True, True, 0),
    (33, 3, 3, 7, False, True, 0),
    (33, 1, 5, 1, True, False, 0),
    (70, 1, 8, 7, False, False, 0),
    (70, 3, 1, 1, True, True, 0),
    (130, 3, 2, 1, False, True, 0),
    (130, 1, 5, 7, True, False, 0),
    (130, 3, 8, 7, True, True, 0),
    (70, 3, 3, 7, False, False, 0),
]
IDS = ['N%d-T%d-D%d-S%d-%s%s' % (c[0], c[1], c[2], c[3], 'dir' if c[4] else 'und', '-mask' if c[5] else '')
       for c in CASES]


def random_mask(rng, T, N):
    """(T, N, N) boolean: 10 % of the entries at random and one whole row"""
    mask = rng.rand(T, N, N) < 0.1
    mask[rng.randint(T), rng.randint(N), :] = True
    return mask


def draw(N, T, D, S, directed, masked, seed):
    rng = np.random.RandomState(1000 * seed + 8 * N + D + 4 * directed)
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    mask = random_mask(rng, T, N) if masked else None
    return Y, Xs, ic, radii, mask


@functools.lru_cache(maxsize=None)
def case(index):
    """(inputs, reference) of CASES[index]; shared and not to be modified"""
    N, T, D, S, directed, masked, seed = CASES[index]
    inputs = draw(N, T, D, S, directed, masked, seed)
    Y, Xs, ic, radii, mask = inputs
    return inputs, score_ref.reference(Y, Xs, ic, radii, directed, mask)


def stable(ref):
    return score_ref.keys_are_stable(ref['pbar'][ref['scored']])


def find_seed(N, T, D, S, directed, masked):
    for seed in range(100):
        Y, Xs, ic, radii, mask = draw(N, T, D, S, directed, masked, seed)
        eta = score_ref.linear_predictor(Xs, ic, radii, directed)
        pbar = score_ref.posterior_mean_proba(eta)
        if score_ref.keys_are_stable(pbar[score_ref.scored_dyads(T, N, directed, mask)]):
            return seed
    raise RuntimeError('no seed found')
