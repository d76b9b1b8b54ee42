"""What the passes over a fitted model's trace share (gof, ic, scores, convergence, forecast_paths): which
rows of the trace they use, the arrays of those rows, the observed network, and the chain the device part
runs on.  No public API."""
import contextlib

import numpy as np

from .engine import Chain


def kept_start(model, n_rows):
    from .hdp_lpcm import DynamicNetworkHDPLPCM
    n_burn = model.n_burn_
    if isinstance(model, DynamicNetworkHDPLPCM):      # its n_burn_ counts iterations: rows are thinned
        n_burn = -(-n_burn // (model.thin or 1))
    return min(int(n_burn), n_rows - 1)


def observed_network(model):
    Y = np.asarray(model.Y_fit_) != 0         # a new boolean array
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = False
    return Y


def two_intercepts(ic):
    ic = np.asarray(ic, dtype=np.float64)
    ic = ic.reshape(ic.shape[0], -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    return np.ascontiguousarray(ic[:, :2])


def sample_rows(model, n_samples):
    """the trace rows a pass over the posterior uses: all kept rows (after the burn-in), or
    ``n_samples`` of them evenly spaced"""
    if not hasattr(model, 'Y_fit_') or not hasattr(model, 'intercepts_'):
        raise ValueError('Model not fit.')
    n_rows = np.shape(model.intercepts_)[0]
    start = kept_start(model, n_rows)
    if n_samples is None:
        return np.arange(start, n_rows, dtype=np.int64)
    n_samples_i = int(n_samples)
    if n_samples_i != n_samples or n_samples_i < 1:
        raise ValueError('n_samples must be a positive integer, got %r' % (n_samples,))
    if n_samples_i > n_rows - start:
        raise ValueError('n_samples=%d exceeds the %d kept samples of the trace'
                         % (n_samples_i, n_rows - start))
    return np.round(np.linspace(start, n_rows - 1, n_samples_i)).astype(np.int64)


def trace_samples(model, ids, step=None):
    """(Xs (S, T, N, D), intercepts (S, 2), radii (S, N) or None) of the trace rows ``ids``; ``step``: Xs
    (S, N, D) of that time step alone"""
    Xs = np.asarray(model.Xs_)
    return (np.ascontiguousarray(Xs[ids] if step is None else Xs[ids, step], dtype=np.float64),
            two_intercepts(np.asarray(model.intercepts_, dtype=np.float64)[ids]),
            np.asarray(model.radiis_, dtype=np.float64)[ids] if model.is_directed else None)


def point_estimate(model):
    """the same triple, S = 1, of the fit's point estimate (``X_``, ``intercept_``, ``radii_``)"""
    return (np.ascontiguousarray(model.X_, dtype=np.float64)[None],
            two_intercepts(np.asarray(model.intercept_, dtype=np.float64).reshape(1, -1)),
            np.asarray(model.radii_, dtype=np.float64)[None] if model.is_directed else None)


@contextlib.contextmanager
def model_chain(model, T, N, D, directed):
    """the model's ``chain_`` if it is alive, else a ``Chain`` of this shape that is closed afterwards"""
    chain = model.__dict__.get('chain_')
    if chain is None or getattr(chain, '_h', None) is None:
        with Chain(T, N, D, 'directed' if directed else 'undirected', device=getattr(model, 'device', 0)) as own:
            yield own
    else:
        yield chain
