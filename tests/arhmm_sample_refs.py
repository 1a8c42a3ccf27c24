"""float64 numpy restatements of the ARHMM sampling launch (bn_arhmm_sample, csrc/arhmm.hip) for
tests/test_arhmm_sample_cpu.py and tests/test_gpu_arhmm_sample.py.  Two INDEPENDENT forms, so that a tolerance can be
derived from their disagreement:

  A  the plain loop over trials, rows and lags, the state of a row by the counting rule;
  B  the states first, then the drive ``v = b[z] + einsum(C[z], eps)`` for all rows at once, then the recursion in
     companion form (one (L D, L D) matrix per state on the stacked history).

``sample_scale`` is the same recursion on absolute values, the scale a rounding error of x is measured against.

Operands as the launch takes them: ``W`` (K, D, 1 + L D) = [b | A], ``C`` (K, D, D), ``cdf0`` (K), ``cdf`` (K, K),
``offsets`` (S + 1), ``eps`` (n, D), ``u`` (n) or ``states`` (n), ``init`` None or (n, D).  Rows of no trial keep
``fill`` in x and ``state_fill`` in the states."""

import numpy as np

from tests.arhmm_refs import trials_of


def lags_of(W):
    K, D, cols = W.shape
    assert (cols - 1) % D == 0
    return (cols - 1) // D


def count_state(u, row):
    """The number of j in [0, K - 1) with u >= row[j]: the last column is never compared."""
    z = 0
    for j in range(len(row) - 1):
        if u >= row[j]:
            z += 1
    return z


def sample_states(cdf0, cdf, offsets, u, n, state_fill=0):
    out = np.full((n,), state_fill, dtype=np.int32)
    for beg, end in trials_of(offsets):
        z = 0
        for t in range(beg, end):
            z = count_state(u[t], cdf0 if t == beg else cdf[z])
            out[t] = z
    return out


def _bad_from(states, beg, end, K):
    """The first row of the trial whose state is outside [0, K), ``end`` for none."""
    for t in range(beg, end):
        if states[t] < 0 or states[t] >= K:
            return t
    return end


def sample_a(W, C, cdf0, cdf, offsets, eps, u=None, states=None, init=None, fill=0.0, state_fill=0):
    """Restatement A: ``(x, states)``."""
    K, D, _ = W.shape
    L = lags_of(W)
    n = eps.shape[0]
    assert (u is None) != (states is None)
    x = np.full((n, D), fill, dtype=np.float64)
    if states is None:
        zs = sample_states(cdf0, cdf, offsets, u, n, state_fill)
    else:
        zs = np.full((n,), state_fill, dtype=np.int32)
        for beg, end in trials_of(offsets):
            zs[beg:end] = states[beg:end]
    for beg, end in trials_of(offsets):
        stop = _bad_from(zs, beg, end, K)
        x[stop:end] = np.nan
        for t in range(beg, stop):
            if t - beg < L:
                x[t] = np.asarray(init[t], dtype=np.float64) if init is not None else eps[t]
                continue
            k = zs[t]
            row = W[k, :, 0].copy()
            for l in range(L):
                row += W[k, :, 1 + l * D:1 + (l + 1) * D] @ x[t - 1 - l]
            x[t] = row + C[k] @ eps[t]
    return x, zs


def companion(W):
    """Per state the (L D, L D) matrix that advances the stacked history (x_{t-1}, ..., x_{t-L})."""
    K, D, _ = W.shape
    L = lags_of(W)
    H = L * D
    M = np.zeros((K, H, H))
    for k in range(K):
        M[k, :D, :] = W[k, :, 1:]
        if L > 1:
            M[k, D:, :H - D] = np.eye(H - D)
    return M


def sample_b(W, C, cdf0, cdf, offsets, eps, u=None, states=None, init=None, fill=0.0, state_fill=0):
    """Restatement B: ``(x, states)``."""
    K, D, _ = W.shape
    L = lags_of(W)
    n = eps.shape[0]
    x = np.full((n, D), fill, dtype=np.float64)
    if states is None:
        zs = sample_states(cdf0, cdf, offsets, u, n, state_fill)
    else:
        zs = np.full((n,), state_fill, dtype=np.int32)
        for beg, end in trials_of(offsets):
            zs[beg:end] = states[beg:end]
    safe = np.clip(zs, 0, K - 1)
    v = W[safe, :, 0] + np.einsum('tij,tj->ti', C[safe], eps)
    M = companion(W) if L else None
    for beg, end in trials_of(offsets):
        stop = _bad_from(zs, beg, end, K)
        x[stop:end] = np.nan
        head = min(beg + L, stop)
        x[beg:head] = np.asarray(init[beg:head], dtype=np.float64) if init is not None else eps[beg:head]
        if stop - beg <= L:
            continue
        if L == 0:
            x[beg:stop] = v[beg:stop]
            continue
        h = x[beg:beg + L][::-1].reshape(-1).copy()               # (x_{t-1}, ..., x_{t-L}) stacked
        drive = np.zeros(L * D)
        for t in range(beg + L, stop):
            drive[:D] = v[t]
            h = M[safe[t]] @ h + drive
            x[t] = h[:D]
    return x, zs


def sample_scale(W, C, offsets, eps, states, init=None):
    """``s_t = |b| + |A| s_hist + |C| |eps|`` along the states ``states`` (valid ones): the sum of the absolute values
    of every term that enters x_t, 1 where no trial is."""
    K, D, _ = W.shape
    L = lags_of(W)
    n = eps.shape[0]
    s = np.ones((n, D))
    aW, aC, ae = np.abs(W), np.abs(C), np.abs(eps)
    for beg, end in trials_of(offsets):
        for t in range(beg, end):
            if t - beg < L:
                s[t] = np.abs(np.asarray(init[t], dtype=np.float64)) if init is not None else ae[t]
                continue
            k = min(max(int(states[t]), 0), K - 1)
            row = aW[k, :, 0] + aC[k] @ ae[t]
            for l in range(L):
                row = row + aW[k, :, 1 + l * D:1 + (l + 1) * D] @ s[t - 1 - l]
            s[t] = row
    return s


def spectral_radii(W):
    """The spectral radius of every state's companion matrix (zeros without lags)."""
    if lags_of(W) == 0:
        return np.zeros(W.shape[0])
    return np.asarray([np.abs(np.linalg.eigvals(m)).max() for m in companion(W)])


def stationary(Ps):
    """The stationary distribution of the row-stochastic matrix ``Ps``."""
    K = Ps.shape[0]
    A = np.concatenate([Ps.T - np.eye(K), np.ones((1, K))], axis=0)
    b = np.concatenate([np.zeros(K), [1.0]])
    return np.linalg.lstsq(A, b, rcond=None)[0]


# ------------------------------------------------------------------------------------------------------------
# the shapes and parameters both test files use
SHAPES = [(1, 0), (3, 1), (16, 1), (32, 1), (12, 4), (7, 8)]           # (D, L)
STATES = [1, 2, 5, 32]


def trial_offsets(L, n_long=(37, 150)):
    """tests/test_gpu_arhmm.py's ``_offsets``: trials of length 0, L, L + 1, 37, 150, 0, 1 with two rows in front that
    belong to none (the tests add three behind)."""
    lens = [0, L, L + 1] + list(n_long) + [0, 1]
    return np.cumsum([2] + lens).astype(np.int64)


def shape_model(D, L, K):
    """The seeded model of a test shape (seed 1000 D + 10 L + K): ``A_k[l] = 0.5 / L I + 0.2 / sqrt(D L) randn``,
    ``Sigma_k = B B^T / D + 0.2 I``, random transition rows and initial distribution."""
    from behavenet_amd.models.arhmm import ARHMM
    rng = np.random.RandomState(1000 * D + 10 * L + K)
    m = ARHMM(K, D, lags=L)
    for k in range(K):
        for l in range(L):
            m.As[k][:, l * D:(l + 1) * D] = 0.5 / L * np.eye(D) + 0.2 / np.sqrt(D * L) * rng.randn(D, D)
    m.bs = rng.randn(K, D)
    for k in range(K):
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    Ps = rng.rand(K, K) + 0.1
    pi0 = rng.rand(K) + 0.1
    m.log_Ps, m.log_pi0 = np.log(Ps / Ps.sum(axis=1, keepdims=True)), np.log(pi0 / pi0.sum())
    return m


def shape_noise(D, L, K, with_init=True):
    """``(offsets, n, eps, u, init)`` of a test shape: init is fp32, (n, D + 3) wide so that a row stride can be cut."""
    rng = np.random.RandomState(7 + 1000 * D + 10 * L + K)
    offsets = trial_offsets(L)
    n = int(offsets[-1]) + 3
    eps = rng.randn(n, D)
    u = rng.rand(n)
    init = (rng.randn(n, D + 3) + 0.5).astype(np.float32)
    return offsets, n, eps, u, init
