"""float64 numpy restatements of the one-step-ahead predictions of an ARHMM (bn_hmm_predictive, bn_arhmm_predict,
ARHMM.prediction_sums), for tests/test_arhmm_predict_cpu.py and tests/test_gpu_arhmm_predict.py.  Two INDEPENDENT
forms of every quantity a tolerance is derived for: the causal weights in log space (scipy's logsumexp) and scaled;
the predictions by a loop over the states and by one einsum; and, for tiny trials, a brute force over every state
path."""

import itertools

import numpy as np
from scipy.special import logsumexp

from tests.arhmm_refs import path_score, trials_of


def weights_log(ll, log_Ps, log_pi0):
    """``w_t = p(z_t | x_0 .. x_{t-1})`` of ONE trial in log space: (T, K)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    w = np.zeros((T, K))
    if T == 0:
        return w
    with np.errstate(divide='ignore', invalid='ignore'):
        w[0] = np.exp(log_pi0)
        # la: log p(z_t, x_0 .. x_t) up to a constant per row -- the row's largest ll and the evidence so far are taken
        # out at every step, or la would grow to T |ll| and carry that size's rounding (3e-10 at 300 rows of -1e4)
        la = log_pi0 + (ll[0] - ll[0].max())
        for t in range(1, T):
            lw = logsumexp(la[:, None] + log_Ps, axis=0) - logsumexp(la)       # log p(z_t | x_0 .. x_{t-1})
            w[t] = np.exp(lw)
            la = lw + (ll[t] - ll[t].max())
    return w


def weights_scaled(ll, log_Ps, log_pi0):
    """The same weights by the scaled recursion (row maximum out, the filtered marginals normalised every step)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    w = np.zeros((T, K))
    if T == 0:
        return w
    Ps, pi0 = np.exp(log_Ps), np.exp(log_pi0)
    w[0] = pi0
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for t in range(T - 1):
            b = np.exp(ll[t] - ll[t].max())
            u = w[t] * b
            ah = u / u.sum()
            w[t + 1] = ah @ Ps
    return w


def weights_table(ll, offsets, log_Ps, log_pi0, form=weights_log):
    """Every trial: (n, K), zeros outside the trials."""
    ll = np.asarray(ll, dtype=np.float64)
    w = np.zeros_like(ll)
    for beg, end in trials_of(offsets):
        w[beg:end] = form(ll[beg:end], log_Ps, log_pi0)
    return w


def weights_brute_force(ll, log_Ps, log_pi0):
    """Every state path of a tiny trial: ``w_t[j] = sum over paths z_0 .. z_t with z_t = j of
    p(z_0 .. z_t, x_0 .. x_{t-1})``, divided by its sum over j."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    w = np.zeros((T, K))
    for t in range(T):
        for p in itertools.product(range(K), repeat=t + 1):
            # the path's score up to z_t without the emission of row t
            s = path_score(ll[:t + 1], log_Ps, log_pi0, p) - ll[t, p[t]]
            w[t, p[t]] += np.exp(s)
        w[t] /= w[t].sum()
    return w


def history_rows(x, lags):
    """``phi_t = (1, x_{t-1}, .., x_{t-lags})`` (T - lags, 1 + lags D) of ONE trial in float64, t = lags .. T - 1."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    rows = [np.concatenate([[1.0]] + [x[t - 1 - l] for l in range(lags)]) for t in range(lags, T)]
    return np.asarray(rows).reshape(-1, 1 + lags * D)


def predict_loop(table, offsets, W, weights, lags):
    """xhat (n, D) by a loop over trials, rows and states: the state's regression first, then the mixture."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    K = len(W)
    out = np.zeros((n, D))
    for beg, end in trials_of(offsets):
        out[beg:min(beg + lags, end)] = z[beg:min(beg + lags, end)]
        for t in range(beg + lags, end):
            acc = np.zeros(D)
            for k in range(K):
                mu = W[k][:, 0].copy()
                for l in range(lags):
                    mu = mu + W[k][:, 1 + l * D:1 + (l + 1) * D] @ z[t - 1 - l]
                acc = acc + weights[t, k] * mu
            out[t] = acc
    return out


def predict_einsum(table, offsets, W, weights, lags):
    """The predictions again, one einsum a trial over (state, history entry) at once."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    out = np.zeros((n, D))
    for beg, end in trials_of(offsets):
        out[beg:min(beg + lags, end)] = z[beg:min(beg + lags, end)]
        if end - beg > lags:
            phi = history_rows(z[beg:end], lags)
            out[beg + lags:end] = np.einsum('tk,tq,kdq->td', weights[beg + lags:end], phi, np.asarray(W))
    return out


def predict_scale(table, offsets, W, weights, lags):
    """``sum_k |w_k| sum_q |W_k[d, q] phi[q]|`` per element, the scale a rounding error of xhat is measured against
    (|x| for the initial rows, 1 outside the trials)."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    sc = np.ones((n, D))
    for beg, end in trials_of(offsets):
        sc[beg:min(beg + lags, end)] = np.abs(z[beg:min(beg + lags, end)])
        if end - beg > lags:
            phi = np.abs(history_rows(z[beg:end], lags))
            sc[beg + lags:end] = np.einsum('tk,tq,kdq->td', np.abs(weights[beg + lags:end]), phi, np.abs(W))
    return sc


def valid_rows(n, offsets, lags):
    """The rows that are scored: in a trial, with ``t >= max(lags, 1)``."""
    valid = np.zeros(n, dtype=bool)
    for beg, end in trials_of(offsets):
        valid[min(beg + max(lags, 1), end):end] = True
    return valid


def prediction_sums(table, pred, offsets, lags):
    """``(2, S, D, 4)`` straight from the definitions, per trial and dimension over the valid rows: the count,
    ``sum x``, ``sum x^2`` and ``sum (x - p)^2`` for ``p = pred`` ([0]) and for ``p_t = x_{t-1}`` ([1]); with them
    ``sum |terms|`` of the three sums, (2, S, D, 4) as well (the count's is the count), the scale of a rounding
    error."""
    x = np.asarray(table, dtype=np.float64)
    p = np.asarray(pred, dtype=np.float64)
    tr = trials_of(offsets)
    D = x.shape[1]
    sums, scale = np.zeros((2, len(tr), D, 4)), np.zeros((2, len(tr), D, 4))
    for s, (beg, end) in enumerate(tr):
        lo = min(beg + max(lags, 1), end)
        for which in (0, 1):
            for t in range(lo, end):
                guess = p[t] if which == 0 else x[t - 1]
                terms = np.stack([np.ones(D), x[t], x[t] * x[t], (x[t] - guess) ** 2], axis=1)
                sums[which, s] += terms
                scale[which, s] += np.abs(terms)
    return sums, scale


def scores(sums):
    """``{'n', 'mse', 'r2'}`` (..., D) from sums (..., D, 4), plainly: no rule for few rows or constant columns."""
    n, sy, syy, sd = (sums[..., i] for i in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'n': n, 'mse': sd / n, 'r2': 1.0 - sd / (syy - sy * sy / n)}
