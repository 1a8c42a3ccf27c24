"""float64 numpy restatements of the ARHMM launches (csrc/arhmm.hip) and of one EM iteration, for
tests/test_arhmm_cpu.py and tests/test_gpu_arhmm.py.  Two INDEPENDENT forms where a tolerance is derived from their
disagreement: the emission density directly from (As, bs, Sigmas) and through the model's fold(); forward-backward in
log space (scipy's logsumexp) and scaled."""

import itertools

import numpy as np
from scipy.special import logsumexp

LOG_2PI = float(np.log(2.0 * np.pi))


def trials_of(offsets):
    offsets = np.asarray(offsets, dtype=np.int64)
    return [(int(a), int(max(a, b))) for a, b in zip(offsets[:-1], offsets[1:])]


def lagged_rows(x, lags, shift=None):
    """``a_t`` (T - lags, P) of ONE trial x (T, D) in float64: (1, x_t - c, x_{t-1} - c, ..., x_{t-lags} - c)."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    c = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64)
    rows = []
    for t in range(lags, T):
        rows.append(np.concatenate([[1.0]] + [x[t - l] - c for l in range(lags + 1)]))
    return np.asarray(rows).reshape(-1, 1 + (lags + 1) * D)


def loglik_direct(table, offsets, As, bs, Sigmas, lags):
    """ll (n, K) straight from the parameters (np.linalg.solve / slogdet), NOT through fold()."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    K = len(bs)
    ll = np.zeros((n, K))
    logdets = [np.linalg.slogdet(Sigmas[k])[1] for k in range(K)]
    for beg, end in trials_of(offsets):
        for t in range(beg, min(beg + lags, end)):
            ll[t, :] = -0.5 * D * LOG_2PI - 0.5 * np.sum(z[t] * z[t])
        if end - beg <= lags:
            continue
        for k in range(K):
            mu = np.tile(bs[k], (end - beg - lags, 1))
            for l in range(lags):
                mu = mu + z[beg + lags - 1 - l:end - 1 - l] @ As[k][:, l * D:(l + 1) * D].T
            r = z[beg + lags:end] - mu
            quad = np.sum(r * np.linalg.solve(Sigmas[k], r.T).T, axis=1)
            ll[beg + lags:end, k] = -0.5 * D * LOG_2PI - 0.5 * logdets[k] - 0.5 * quad
    return ll


def loglik_folded(table, offsets, G, cst, lags, shift=None):
    """ll (n, K) from the folded parameters, as the kernel forms it."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    K = len(cst)
    ll = np.zeros((n, K))
    for beg, end in trials_of(offsets):
        for t in range(beg, min(beg + lags, end)):
            ll[t, :] = -0.5 * D * LOG_2PI - 0.5 * np.sum(z[t] * z[t])
        if end - beg > lags:
            a = lagged_rows(z[beg:end], lags, shift)
            for k in range(K):
                ll[beg + lags:end, k] = cst[k] - 0.5 * np.sum((a @ G[k].T) ** 2, axis=1)
    return ll


def fb_log(ll, log_Ps, log_pi0):
    """Log-space forward-backward of ONE trial: (gamma (T, K), xi_sum (K, K), loglik)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    if T == 0:
        return np.zeros((0, K)), np.zeros((K, K)), 0.0
    with np.errstate(divide='ignore'):
        la = np.zeros((T, K))
        la[0] = log_pi0 + ll[0]
        for t in range(1, T):
            la[t] = logsumexp(la[t - 1][:, None] + log_Ps, axis=0) + ll[t]
        lb = np.zeros((T, K))
        for t in range(T - 2, -1, -1):
            lb[t] = logsumexp(log_Ps + (ll[t + 1] + lb[t + 1])[None, :], axis=1)
        Z = logsumexp(la[T - 1])
        gamma = np.exp(la + lb - Z)
        xi = np.zeros((K, K))
        for t in range(T - 1):
            xi += np.exp(la[t][:, None] + log_Ps + (ll[t + 1] + lb[t + 1])[None, :] - Z)
    return gamma, xi, float(Z)


def fb_scaled(ll, log_Ps, log_pi0):
    """Scaled forward-backward of ONE trial (row maximum out, alpha normalised every step)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    if T == 0:
        return np.zeros((0, K)), np.zeros((K, K)), 0.0
    Ps, pi0 = np.exp(log_Ps), np.exp(log_pi0)
    m = ll.max(axis=1)
    b = np.exp(ll - m[:, None])
    ah, c = np.zeros((T, K)), np.zeros(T)
    u = pi0 * b[0]
    for t in range(T):
        if t:
            u = (ah[t - 1] @ Ps) * b[t]
        c[t] = u.sum()
        ah[t] = u / c[t]
    bh = np.ones((T, K))
    xi = np.zeros((K, K))
    for t in range(T - 2, -1, -1):
        v = b[t + 1] * bh[t + 1] / c[t + 1]
        bh[t] = Ps @ v
        xi += ah[t][:, None] * Ps * v[None, :]
    gamma = ah * bh
    gamma /= gamma.sum(axis=1, keepdims=True)
    return gamma, xi, float(np.sum(np.log(c)) + np.sum(m))


def forward_backward(ll, offsets, log_Ps, log_pi0, fb=fb_log):
    """Every trial: (gamma (n, K), xi (S, K, K), loglik (S))."""
    ll = np.asarray(ll, dtype=np.float64)
    K = ll.shape[1]
    tr = trials_of(offsets)
    gamma, xi, lls = np.zeros_like(ll), np.zeros((len(tr), K, K)), np.zeros(len(tr))
    for s, (beg, end) in enumerate(tr):
        gamma[beg:end], xi[s], lls[s] = fb(ll[beg:end], log_Ps, log_pi0)
    return gamma, xi, lls


def path_score(ll, log_Ps, log_pi0, path):
    ll = np.asarray(ll, dtype=np.float64)
    if len(path) == 0:
        return 0.0
    s = log_pi0[path[0]] + ll[0, path[0]]
    for t in range(1, len(path)):
        s += log_Ps[path[t - 1], path[t]] + ll[t, path[t]]
    return float(s)


def viterbi(ll, log_Ps, log_pi0):
    """The best path of ONE trial, ties to the lowest state (np.argmax takes the first maximum): (path, score)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    if T == 0:
        return np.zeros((0,), dtype=np.int32), 0.0
    delta = log_pi0 + ll[0]
    back = np.zeros((T, K), dtype=np.int64)
    for t in range(1, T):
        cand = delta[:, None] + log_Ps
        back[t] = np.argmax(cand, axis=0)
        delta = cand[back[t], np.arange(K)] + ll[t]
    path = np.zeros(T, dtype=np.int32)
    path[T - 1] = int(np.argmax(delta))
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path, float(np.max(delta))


def viterbi_table(ll, offsets, log_Ps, log_pi0):
    out = np.zeros((len(ll),), dtype=np.int32)
    for beg, end in trials_of(offsets):
        out[beg:end] = viterbi(ll[beg:end], log_Ps, log_pi0)[0]
    return out


def brute_force(ll, log_Ps, log_pi0):
    """Every path of a tiny trial: (gamma, xi_sum, loglik, best path (the first in lexicographic order), its score)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    paths = list(itertools.product(range(K), repeat=T))
    scores = np.asarray([path_score(ll, log_Ps, log_pi0, p) for p in paths])
    Z = logsumexp(scores)
    w = np.exp(scores - Z)
    gamma, xi = np.zeros((T, K)), np.zeros((K, K))
    for p, wp in zip(paths, w):
        for t in range(T):
            gamma[t, p[t]] += wp
        for t in range(T - 1):
            xi[p[t], p[t + 1]] += wp
    best = int(np.argmax(scores))
    return gamma, xi, float(Z), np.asarray(paths[best], dtype=np.int32), float(scores[best])


def moments(table, offsets, gamma, lags, shift=None):
    """(out (K, P, P), gamma0 (K)) by an explicit loop over the rows."""
    z = np.asarray(table, dtype=np.float64)
    D = z.shape[1]
    K = gamma.shape[1]
    P = 1 + (lags + 1) * D
    out, g0 = np.zeros((K, P, P)), np.zeros(K)
    for beg, end in trials_of(offsets):
        g0 += gamma[beg:min(beg + lags, end)].sum(axis=0)
        if end - beg > lags:
            a = lagged_rows(z[beg:end], lags, shift)
            for i in range(a.shape[0]):
                outer = np.outer(a[i], a[i])
                for k in range(K):
                    out[k] += gamma[beg + lags + i, k] * outer
    return out, g0


def moments_abs(table, offsets, gamma, lags, shift=None):
    """sum |gamma| |a_i| |a_j|: the scale a rounding error of the moments is measured against."""
    z = np.asarray(table, dtype=np.float64)
    K = gamma.shape[1]
    P = 1 + (lags + 1) * z.shape[1]
    out = np.zeros((K, P, P))
    for beg, end in trials_of(offsets):
        if end - beg > lags:
            a = np.abs(lagged_rows(z[beg:end], lags, shift))
            g = np.abs(gamma[beg + lags:end])
            out += np.einsum('tk,ti,tj->kij', g, a, a)
    return out


def moments_einsum(table, offsets, gamma, lags, shift=None):
    """The moments again, one einsum a trial (another summation order than the loop's)."""
    z = np.asarray(table, dtype=np.float64)
    K = gamma.shape[1]
    P = 1 + (lags + 1) * z.shape[1]
    out = np.zeros((K, P, P))
    for beg, end in trials_of(offsets):
        if end - beg > lags:
            a = lagged_rows(z[beg:end], lags, shift)
            out += np.einsum('tk,ti,tj->kij', gamma[beg + lags:end], a, a)
    return out


def table_loglik(model, table, offsets, second_form=False):
    if second_form:
        G, cst = model.fold()
        return loglik_folded(table, offsets, G, cst, model.lags, model.shift)
    return loglik_direct(table, offsets, model.As, model.bs, model.Sigmas, model.lags)


def em_iteration(model, table, offsets, second_form=False):
    """One EM iteration of ``model`` (a behavenet_amd.models.arhmm.ARHMM, updated in place) on the host from the
    restatements above: the direct density, log-space forward-backward, the looped moments, the model's M-step --
    or, with ``second_form``, the folded density, the scaled forward-backward and the einsum moments.
    Returns the per-trial log-likelihoods of the parameters before the update."""
    ll = table_loglik(model, table, offsets, second_form)
    gamma, xi, lls = forward_backward(ll, offsets, model.log_Ps, model.log_pi0, fb_scaled if second_form else fb_log)
    if second_form:
        mom = moments_einsum(table, offsets, gamma, model.lags, model.shift)
    else:
        mom, _ = moments(table, offsets, gamma, model.lags, model.shift)
    g0 = np.zeros(model.K)
    for beg, end in trials_of(offsets):
        if end > beg:
            g0 += gamma[beg]
    model.m_step(mom, xi.sum(axis=0), g0)
    return lls


def trial_logliks(model, table, offsets, second_form=False):
    ll = table_loglik(model, table, offsets, second_form)
    return forward_backward(ll, offsets, model.log_Ps, model.log_pi0, fb_scaled if second_form else fb_log)[2]


def loglik_scale(table, offsets, G, cst, lags, shift=None):
    """sum |terms| of every ll element, the scale a rounding error of it is measured against:
    |cst_k| + 1/2 sum_d (sum_p |G_kdp| |a_p|)^2 for AR rows, D/2 log 2 pi + 1/2 |x|^2 for initial rows."""
    z = np.asarray(table, dtype=np.float64)
    n, D = z.shape
    K = len(cst)
    sc = np.ones((n, K))
    for beg, end in trials_of(offsets):
        for t in range(beg, min(beg + lags, end)):
            sc[t, :] = 0.5 * D * LOG_2PI + 0.5 * np.sum(z[t] * z[t])
        if end - beg > lags:
            a = np.abs(lagged_rows(z[beg:end], lags, shift))
            for k in range(K):
                sc[beg + lags:end, k] = abs(cst[k]) + 0.5 * np.sum((a @ np.abs(G[k]).T) ** 2, axis=1)
    return sc


def sample_arhmm(rng, K, D, lags, lengths, sep=3.0):
    """Trials drawn from a seeded ARHMM with well-separated states: (list of (T, D) float32 arrays, list of paths)."""
    As = [np.concatenate([0.5 / max(lags, 1) * np.eye(D) + 0.05 * rng.randn(D, D) for _ in range(lags)], axis=1)
          if lags else np.zeros((D, 0)) for _ in range(K)]
    bs = [sep * rng.randn(D) for _ in range(K)]
    Ps = np.full((K, K), 0.05 / max(K - 1, 1)) + (0.95 - 0.05 / max(K - 1, 1)) * np.eye(K)
    Ps /= Ps.sum(axis=1, keepdims=True)
    datas, paths = [], []
    for T in lengths:
        x = np.zeros((T, D))
        zs = np.zeros(T, dtype=np.int32)
        z = rng.randint(K)
        for t in range(T):
            if t:
                z = rng.choice(K, p=Ps[z])
            zs[t] = z
            if t < lags:
                x[t] = rng.randn(D)
            else:
                mu = bs[z].copy()
                for l in range(lags):
                    mu += As[z][:, l * D:(l + 1) * D] @ x[t - 1 - l]
                x[t] = mu + 0.3 * rng.randn(D)
        datas.append(x.astype(np.float32))
        paths.append(zs)
    return datas, paths
