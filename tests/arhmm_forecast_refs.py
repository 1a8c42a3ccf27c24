"""float64 numpy restatements of the exact multi-step forecasts of an ARHMM (ARHMM.forecast_maps,
bn_arhmm_forecast_sums, ARHMM.forecast_sums), for tests/test_arhmm_forecast_cpu.py and
tests/test_gpu_arhmm_forecast.py.  Three INDEPENDENT forms: the forecast of one origin by enumeration of every state
path, the forecasts of a table from given maps by a loop over origins, horizons and states (and the same loop with a
trial's origins as one array, for the larger shapes), and the same by one einsum; and the five sums with their
``sum |terms|`` straight from the validity rule.

Origin row t of a trial [beg, end) forecasts the rows t .. t + H - 1 from ``phi_t = (1, x_{t-1}, .., x_{t-L})``; the
pair (t, h) counts iff ``t - beg >= max(L, 1)`` and ``t + h - 1 < end``."""

import itertools

import numpy as np

from tests.arhmm_predict_refs import history_rows
from tests.arhmm_refs import trials_of


def forecast_brute_force(W, Ps, w, phi, H):
    """``E[x_{t+h-1}]`` for h = 1 .. H, (H, D), and ``sum |terms|`` (H, D), of ONE origin with state weights ``w`` (K,)
    and history ``phi`` (1 + L D,): every state path z_1 .. z_h runs its own affine recursion (the state's regression
    on the rows forecast so far and the history) and is weighted by ``w[z_1] prod Ps[z_i][z_{i+1}]``."""
    W = np.asarray(W, dtype=np.float64)
    K, D, Q = W.shape
    L = (Q - 1) // D if D else 0
    out, scale = np.zeros((H, D)), np.zeros((H, D))
    for h in range(1, H + 1):
        for path in itertools.product(range(K), repeat=h):
            p = w[path[0]]
            for a, b in zip(path[:-1], path[1:]):
                p = p * Ps[a][b]
            lagged = [np.asarray(phi[1 + l * D:1 + (l + 1) * D], dtype=np.float64) for l in range(L)]
            x = None
            for k in path:
                x = W[k][:, 0].copy()
                for l in range(L):
                    x = x + W[k][:, 1 + l * D:1 + (l + 1) * D] @ lagged[l]
                lagged = ([x] + lagged)[:L]
            out[h - 1] += p * x
            scale[h - 1] += np.abs(p * x)
    return out, scale


def origins_of(beg, end, lags):
    """The origin rows of a trial."""
    return range(min(beg + max(lags, 1), end), end)


def forecast_loop(table, offsets, N, weights, lags):
    """xhat (n, H, D) from the maps ``N (H, K, D, Q)``: a loop over origins, horizons and states, the state's map
    applied first and the mixture after.  Zeros where the pair (t, h) does not count."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    H, K = N.shape[:2]
    out = np.zeros((n, H, D))
    for beg, end in trials_of(offsets):
        for t in origins_of(beg, end, lags):
            phi = np.concatenate([[1.0]] + [z[t - 1 - l] for l in range(lags)])
            for h in range(min(H, end - t)):
                acc = np.zeros(D)
                for k in range(K):
                    acc = acc + weights[t, k] * (N[h, k] @ phi)
                out[t, h] = acc
    return out


def forecast_loop_trials(table, offsets, N, weights, lags):
    """``forecast_loop`` with a trial's origins as ONE array: still a loop over horizons and states, the state's map
    first (a matrix product over the history entries) and the mixture after, state by state.  What the device is held
    against at shapes where the loop over single origins would take minutes; tests/test_arhmm_forecast_cpu.py holds
    the two against each other."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    H, K = N.shape[:2]
    out = np.zeros((n, H, D))
    for beg, end in trials_of(offsets):
        lo = min(beg + max(lags, 1), end)
        if lo == end:
            continue
        phi = history_rows(z[beg:end], lags)[lo - beg - lags:]
        for h in range(min(H, end - lo)):
            stop = end - h                                  # origins lo .. end - h - 1 reach row t + h
            mapped = phi[:stop - lo] @ N[h].reshape(K * D, -1).T              # every state's map of every origin
            acc = np.zeros((stop - lo, D))
            for k in range(K):
                acc = acc + weights[lo:stop, k][:, None] * mapped[:, k * D:(k + 1) * D]
            out[lo:stop, h] = acc
    return out


def forecast_einsum(table, offsets, N, weights, lags):
    """The same forecasts, one einsum a trial over (state, history entry) for all horizons at once (``optimize``: numpy
    contracts the operands pair by pair, a product of matrices where the plain einsum is a loop over five indices)."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    H = N.shape[0]
    out = np.zeros((n, H, D))
    for beg, end in trials_of(offsets):
        lo = min(beg + max(lags, 1), end)
        if lo < end:
            phi = history_rows(z[beg:end], lags)[lo - beg - lags:]
            out[lo:end] = np.einsum('tk,tq,hkdq->thd', weights[lo:end], phi, N, optimize=True)
            for t in range(max(lo, end - H + 1), end):
                out[t, end - t:] = 0.0
    return out


def forecast_sums(table, xhat, offsets, lags):
    """``(H, S, D, 5)`` from forecasts ``xhat (n, H, D)`` straight from the validity rule, with ``y = x_{t+h-1}``: the
    count, ``sum y``, ``sum y^2``, ``sum (y - xhat_{t,h})^2``, ``sum (y - x_{t-1})^2``; and ``sum |terms|`` of each,
    the scale of a rounding error."""
    x = np.asarray(table, dtype=np.float64)
    n, H, D = xhat.shape
    tr = trials_of(offsets)
    sums, scale = np.zeros((H, len(tr), D, 5)), np.zeros((H, len(tr), D, 5))
    for s, (beg, end) in enumerate(tr):
        lo = min(beg + max(lags, 1), end)
        for h in range(1, H + 1):
            t = np.arange(lo, end - h + 1)                  # the origins with t + h - 1 < end
            if t.size:
                y = x[t + h - 1]
                terms = np.stack([np.ones_like(y), y, y * y, (y - xhat[t, h - 1]) ** 2, (y - x[t - 1]) ** 2], axis=2)
                sums[h - 1, s] = terms.sum(axis=0)
                scale[h - 1, s] = np.abs(terms).sum(axis=0)
    return sums, scale


def as_model_and_persistence(five):
    """(H, S, D, 5) -> (2, H, S, D, 4), the layout of ``ARHMM.forecast_sums``."""
    return np.stack([five[..., :4], five[..., [0, 1, 2, 4]]])
