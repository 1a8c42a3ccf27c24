"""Autoregressive hidden Markov models on autoencoder latents, fitted by EM with the E-step on the device
("ARHMM"; csrc/arhmm.hip).

The class has the duck type the reference's ARHMM driver (fitting/arhmm_grid_search.py:132-209) and ``export_states``
use of the ``ssm`` library's ``HMM``: ``initialize``, ``fit(method='em', num_iters=1, initialize=False)`` in a loop,
``log_likelihood``, ``expected_states``, ``most_likely_states``, ``permute``.  Served: Gaussian AR observations with
full covariance, ``lags >= 0`` (0 is the reference's ``hmm`` class), ``stationary`` and ``sticky`` transitions, EM.
Everything else is a ``NotImplementedError`` that names the type.

Host side: numpy float64 only -- the M-step, the fold of the parameters for the kernel, the priors.  Device side (per EM
iteration): ``bn_arhmm_loglik`` -> ``bn_hmm_forward_backward`` -> ``bn_arhmm_moments`` on one fp32 table that holds
every trial, one transfer of ``K (P^2 + K + 1)`` doubles.  A fitted model predicts the next latent
(``table_predictions``, ``prediction_sums``, ``predict``, ``smooth``): ``bn_hmm_predictive`` or the posterior marginals
for the state weights, ``bn_arhmm_predict`` for the mixture of the states' regressions; and the latents up to 32 frames
ahead (``forecast_maps``, ``forecast_sums``, ``table_forecast``, ``forecast``): ``bn_arhmm_forecast_sums``.

Model, with ``x_t`` the row, ``L = lags`` and state ``k`` at time ``t``:

    x_t | z_t = k  ~  N(b_k + sum_l A_k[l] x_{t-1-l}, Sigma_k)           t >= L   (``As[k][:, l D:(l + 1) D] = A_k[l]``)
    x_t            ~  N(0, I)                                            t <  L   (the same for every state)

The priors and their defaults (``l2_penalty_A``, ``l2_penalty_b``, ``nu0``, ``Psi0``, ``alpha``, ``kappa``) and the
standard-normal initial rows are THIS project's definitions.  They follow what the ``ssm`` library does as far as its
authors' papers describe it, but that library is not installed where this was written and no parity with it has been
checked.
"""

import numpy as np

_LOG_2PI = float(np.log(2.0 * np.pi))
_SERVED_TRANSITIONS = ('stationary', 'sticky')
_SERVED_OBSERVATIONS = ('ar', 'gaussian')
PREDICTION_WEIGHTS = ('predictive', 'smoothed')


class ARHMM(object):

    def __init__(self, K, D, lags=1, transitions='stationary', kappa=0, alpha=1, l2_penalty_A=1e-8, l2_penalty_b=1e-8,
                 nu0=1e-4, Psi0=1e-4, observations='ar'):
        if observations not in _SERVED_OBSERVATIONS:
            raise NotImplementedError('ARHMM: observations %r are not served (%s are)'
                                      % (observations, ', '.join(_SERVED_OBSERVATIONS)))
        if transitions not in _SERVED_TRANSITIONS:
            raise NotImplementedError('ARHMM: transitions %r are not served (%s are)'
                                      % (transitions, ', '.join(_SERVED_TRANSITIONS)))
        if observations == 'gaussian':
            lags = 0
        from behavenet_amd import _hip
        _hip.check_arhmm_dims('ARHMM', int(D), int(lags), int(K))
        self.K, self.D, self.lags = int(K), int(D), int(lags)
        self.transitions = transitions
        self.kappa = float(kappa) if transitions == 'sticky' else 0.0
        self.alpha = float(alpha)
        self.l2_penalty_A, self.l2_penalty_b = float(l2_penalty_A), float(l2_penalty_b)
        self.nu0, self.Psi0 = float(nu0), float(Psi0)
        K, D, L = self.K, self.D, self.lags
        self.As = np.zeros((K, D, L * D))
        self.bs = np.zeros((K, D))
        self.Sigmas = np.tile(np.eye(D), (K, 1, 1))
        self.log_pi0 = np.full((K,), -np.log(K))
        self.log_Ps = self._initial_log_Ps()
        self.shift = np.zeros((D,))          # the kernels' column shift c: a property of the fit, not of the model

    @property
    def P(self):
        return 1 + (self.lags + 1) * self.D

    def _initial_log_Ps(self):
        Ps = np.ones((self.K, self.K)) + self.kappa * np.eye(self.K)
        return np.log(Ps / Ps.sum(axis=1, keepdims=True))

    # ------------------------------------------------------------------------------------------------------
    # host side
    # ------------------------------------------------------------------------------------------------------
    def fold(self):
        """``(G, cst)`` for ``bn_arhmm_loglik``: ``G[k] = R_k [-(b_k - c + sum_l A_k[l] c) | I | -A_k]`` with
        ``R_k = C_k^-1``, ``Sigma_k = C_k C_k^T`` (Cholesky), so ``|G_k a_t|^2`` is the Mahalanobis distance of the
        residual, and ``cst[k] = -D/2 log 2 pi + log det R_k``."""
        K, D, L, P = self.K, self.D, self.lags, self.P
        G = np.zeros((K, D, P))
        cst = np.zeros((K,))
        c = self.shift
        for k in range(K):
            try:
                C = np.linalg.cholesky(self.Sigmas[k])
            except np.linalg.LinAlgError:
                raise ValueError('ARHMM.fold: Sigmas[%d] is not positive definite' % k)
            if not np.all(np.isfinite(C)):
                raise ValueError('ARHMM.fold: Sigmas[%d] is not finite' % k)
            M = np.zeros((D, P))
            Ac = np.zeros((D,))
            for l in range(L):
                Ac += self.As[k][:, l * D:(l + 1) * D] @ c
            M[:, 0] = -(self.bs[k] - c + Ac)
            M[:, 1:1 + D] = np.eye(D)
            M[:, 1 + D:] = -self.As[k]
            G[k] = np.linalg.solve(C, M)
            cst[k] = -0.5 * D * _LOG_2PI - np.sum(np.log(np.diag(C)))
        return G, cst

    def _ridge(self):
        lam = np.full((1 + self.lags * self.D,), self.l2_penalty_A)
        lam[0] = self.l2_penalty_b
        return lam

    def _shifted_weights(self, k):
        """``W = [b' | A]`` of state k in the shifted coordinates of the moments: ``x_t - c = b' + A (u - c)``."""
        c, D = self.shift, self.D
        Ac = np.zeros((D,))
        for l in range(self.lags):
            Ac += self.As[k][:, l * D:(l + 1) * D] @ c
        return np.concatenate([(self.bs[k] - c + Ac)[:, None], self.As[k]], axis=1)

    def m_step_observations(self, moments):
        """Per state the ridge-regularised weighted least squares for ``[b | A]`` and the MAP covariance from the
        moment matrices ``moments`` (K, P, P) of ``a_t = (1, x_t - c, x_{t-1} - c, ...)``.  A state whose expected
        count is below ``D + 1`` keeps its parameters."""
        K, D, L = self.K, self.D, self.lags
        moments = np.asarray(moments, dtype=np.float64)
        assert moments.shape == (K, self.P, self.P), moments.shape
        c = self.shift
        phi = np.concatenate([[0], np.arange(1 + D, self.P)]).astype(int)       # (1, lagged columns)
        y = np.arange(1, 1 + D)
        lam = np.diag(self._ridge())
        for k in range(K):
            M = moments[k]
            N = M[0, 0]
            if not np.isfinite(N) or N < D + 1:
                continue
            Sxx = M[np.ix_(phi, phi)] + lam
            Sxy = M[np.ix_(phi, y)]
            Syy = M[np.ix_(y, y)]
            W = np.linalg.solve(Sxx, Sxy).T                                     # (D, 1 + L D), shifted coordinates
            scatter = Syy - W @ Sxy - Sxy.T @ W.T + W @ Sxx @ W.T               # (residuals and the ridge term)
            Sigma = (scatter + self.Psi0 * np.eye(D)) / (N + self.nu0 + D + 1)
            A = W[:, 1:]
            Ac = np.zeros((D,))
            for l in range(L):
                Ac += A[:, l * D:(l + 1) * D] @ c
            self.As[k] = A
            self.bs[k] = W[:, 0] + c - Ac
            self.Sigmas[k] = 0.5 * (Sigma + Sigma.T)

    def m_step_transitions(self, xi_sum, gamma0_sum):
        """Transition rows ``~ xi_sum + kappa I + (alpha - 1)`` and ``pi0 ~ gamma0_sum + 1e-8`` (the summed pairwise
        posteriors (K, K) and the summed first-row marginals (K)).  A row without mass keeps its values."""
        xi_sum = np.asarray(xi_sum, dtype=np.float64)
        Ps = np.maximum(xi_sum + self.kappa * np.eye(self.K) + (self.alpha - 1.0), 0.0)
        tot = Ps.sum(axis=1)
        with np.errstate(divide='ignore'):
            for k in range(self.K):
                if np.isfinite(tot[k]) and tot[k] > 0:
                    self.log_Ps[k] = np.log(Ps[k] / tot[k])
            p0 = np.asarray(gamma0_sum, dtype=np.float64) + 1e-8
            if np.all(np.isfinite(p0)):
                self.log_pi0 = np.log(p0 / p0.sum())

    def m_step(self, moments, xi_sum, gamma0_sum):
        self.m_step_observations(moments)
        self.m_step_transitions(xi_sum, gamma0_sum)

    def log_prior(self):
        """The log prior the M-step maximises with the expected log-likelihood (up to constants): per state
        ``-1/2 (nu0 + D + 1) log det Sigma - 1/2 tr(Sigma^-1 (Psi0 I + W Lambda W^T))`` with ``W`` in the shifted
        coordinates and ``Lambda`` the ridge; ``sum (kappa I + alpha - 1) log Ps``; ``1e-8 sum log pi0``."""
        lp = 0.0
        lam = np.diag(self._ridge())
        for k in range(self.K):
            W = self._shifted_weights(k)
            _, logdet = np.linalg.slogdet(self.Sigmas[k])
            B = self.Psi0 * np.eye(self.D) + W @ lam @ W.T
            lp += -0.5 * (self.nu0 + self.D + 1) * logdet - 0.5 * np.trace(np.linalg.solve(self.Sigmas[k], B))
        w = self.kappa * np.eye(self.K) + (self.alpha - 1.0)
        nz = w != 0
        lp += float(np.sum(w[nz] * self.log_Ps[nz]))
        lp += 1e-8 * float(np.sum(self.log_pi0))
        return float(lp)

    def permute(self, perm):
        """State ``k`` becomes the old state ``perm[k]`` (the reference relabels by usage with it)."""
        perm = np.asarray(perm, dtype=int)
        assert sorted(perm.tolist()) == list(range(self.K)), perm
        self.As, self.bs, self.Sigmas = self.As[perm].copy(), self.bs[perm].copy(), self.Sigmas[perm].copy()
        self.log_pi0 = self.log_pi0[perm].copy()
        self.log_Ps = self.log_Ps[np.ix_(perm, perm)].copy()

    # ------------------------------------------------------------------------------------------------------
    # device side
    # ------------------------------------------------------------------------------------------------------
    @staticmethod
    def as_table(datas, device=None):
        """``(table, offsets)``: the trials ``datas`` -- one (T, D) array or tensor, or a list of them -- as ONE fp32
        device table and the int64 host offsets of its trials."""
        import torch
        if not isinstance(datas, (list, tuple)):
            datas = [datas]
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        parts, offsets = [], [0]
        for x in datas:
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
            if t.dim() != 2:
                raise ValueError('ARHMM: a trial must be (T, D), got %s' % (tuple(t.shape),))
            parts.append(t.to(device=device, dtype=torch.float32))
            offsets.append(offsets[-1] + int(t.shape[0]))
        if not parts:
            raise ValueError('ARHMM: no trials')
        return torch.cat(parts, dim=0).contiguous(), np.asarray(offsets, dtype=np.int64)

    def _check_table(self, table):
        if table.dim() != 2 or int(table.shape[1]) != self.D:
            raise ValueError('ARHMM: the model has D = %d, the data %s' % (self.D, tuple(table.shape)))

    def set_shift(self, table):
        """The kernels' shift: the column means of the table (from ``bn_segment_gram``'s sums), rounded to fp32 values.
        The moments lose no digits to a mean far from zero; the model's parameters do not depend on it."""
        from behavenet_amd import _hip
        n = int(table.shape[0])
        g = _hip.segment_gram(table, np.asarray([0, n], dtype=np.int64))[0].cpu().numpy()
        self.shift = (g[0, 1:] / max(g[0, 0], 1.0)).astype(np.float32).astype(np.float64)
        return self.shift

    def _loglik_table(self, table, offsets_d):
        from behavenet_amd import _hip
        G, cst = self.fold()
        return _hip.arhmm_loglik(table, offsets_d, G, cst, self.lags, shift=self.shift)

    def _offsets_d(self, table, offsets):
        import torch
        if torch.is_tensor(offsets):
            return offsets
        return torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(table.device)

    def trial_logliks(self, table, offsets):
        """The log-likelihood of every trial of the table, a float64 host array (S,) (forward sweep only)."""
        from behavenet_amd import _hip
        self._check_table(table)
        offsets_d = self._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        return _hip.hmm_forward_backward(ll, offsets_d, self.log_Ps, self.log_pi0,
                                         want_posteriors=False)[2].cpu().numpy()

    def e_step(self, table, offsets):
        """``(moments, gamma_init, xi_sum, gamma0_sum, logliks)`` of the current parameters, host arrays: the three
        launches of an EM iteration and ONE transfer."""
        import torch
        from behavenet_amd import _hip
        self._check_table(table)
        offsets_d = self._offsets_d(table, offsets)
        K, P = self.K, self.P
        ll = self._loglik_table(table, offsets_d)
        gamma, xi, lls = _hip.hmm_forward_backward(ll, offsets_d, self.log_Ps, self.log_pi0)
        mom, ginit = _hip.arhmm_moments(table, offsets_d, gamma, self.lags, shift=self.shift)
        # the first row of every trial that has one
        first = offsets_d[:-1][offsets_d[1:] > offsets_d[:-1]]
        g0 = gamma.index_select(0, first).sum(dim=0) if first.numel() else gamma.new_zeros((K,))
        packed = torch.cat([mom.reshape(-1), ginit, xi.sum(dim=0).reshape(-1), g0, lls]).cpu().numpy()
        o = np.cumsum([0, K * P * P, K, K * K, K])
        return (packed[o[0]:o[1]].reshape(K, P, P), packed[o[1]:o[2]], packed[o[2]:o[3]].reshape(K, K),
                packed[o[3]:o[4]], packed[o[4]:])

    def em_step(self, table, offsets):
        """One EM iteration on the table; returns the per-trial log-likelihoods of the parameters BEFORE the update."""
        mom, _, xi_sum, g0, lls = self.e_step(table, offsets)
        self.m_step(mom, xi_sum, g0)
        return lls

    def initialize(self, table, offsets=None, seed=0):
        """Per state one least-squares AR fit on a randomly drawn contiguous window of the table (0/1 weights through
        ``bn_arhmm_moments``), uniform ``pi0``, transition rows ``~ 1 + kappa I``.  ``table`` may be a list of trials."""
        import torch
        from behavenet_amd import _hip
        if offsets is None:
            table, offsets = self.as_table(table)
        self._check_table(table)
        n = int(table.shape[0])
        self.set_shift(table)
        rng = np.random.RandomState(seed)
        width = min(n, max(8 * self.P, n // max(self.K, 1)))
        gamma = torch.zeros((n, self.K), dtype=torch.float64, device=table.device)
        for k in range(self.K):
            start = int(rng.randint(0, n - width + 1))
            gamma[start:start + width, k] = 1.0
        mom, _ = _hip.arhmm_moments(table, self._offsets_d(table, offsets), gamma, self.lags, shift=self.shift)
        self.m_step_observations(mom.cpu().numpy())
        self.log_pi0 = np.full((self.K,), -np.log(self.K))
        self.log_Ps = self._initial_log_Ps()

    def fit(self, datas, method='em', num_iters=100, initialize=True, seed=0, **kwargs):
        """EM on the trials ``datas``; returns the total log-likelihood before every iteration (the library's
        ``fit`` returns its ``lls`` the same way)."""
        if method != 'em':
            raise NotImplementedError('ARHMM.fit: method %r is not served (em is)' % (method,))
        table, offsets = self.as_table(datas)
        if initialize:
            self.initialize(table, offsets, seed=seed)
        elif not np.any(self.shift):
            self.set_shift(table)
        return [float(np.sum(self.em_step(table, offsets))) for _ in range(int(num_iters))]

    def log_likelihood(self, datas):
        table, offsets = self.as_table(datas)
        return float(np.sum(self.trial_logliks(table, offsets)))

    def expected_states(self, x):
        """``(Ez, Ezzp1_sum, loglik)`` of ONE trial: the marginals (T, K), the pairwise posteriors summed over time
        (K, K) -- the library returns them per step -- and the log-likelihood."""
        from behavenet_amd import _hip
        table, offsets = self.as_table(x)
        offsets_d = self._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        gamma, xi, lls = _hip.hmm_forward_backward(ll, offsets_d, self.log_Ps, self.log_pi0)
        return gamma.cpu().numpy(), xi[0].cpu().numpy(), float(lls[0])

    def table_states(self, table, offsets):
        """The Viterbi path of every trial of the table in ONE launch: an int32 host array (n,)."""
        from behavenet_amd import _hip
        self._check_table(table)
        offsets_d = self._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        return _hip.hmm_viterbi(ll, offsets_d, self.log_Ps, self.log_pi0).cpu().numpy()

    def table_runs(self, table, offsets):
        """The runs of the Viterbi paths of the table's trials: ``(runs, frames, trans)``, host arrays -- int32
        (R, 4) rows ``(trial, beg, end, state)`` in table order, ``beg`` / ``end`` relative to the trial and ``end``
        exclusive, int64 (K) frames per state and int64 (K, K) in-trial transition counts (``_hip.state_runs``).
        Log-likelihoods, Viterbi and the run search follow each other on the device; the states never leave it and
        the three results cross in ONE transfer."""
        import torch
        from behavenet_amd import _hip
        self._check_table(table)
        offsets_d = self._offsets_d(table, offsets)
        K = self.K
        ll = self._loglik_table(table, offsets_d)
        states = _hip.hmm_viterbi(ll, offsets_d, self.log_Ps, self.log_pi0)
        runs, frames, trans = _hip.state_runs(states, offsets_d, K)
        packed = torch.cat([runs.reshape(-1).to(torch.int64), frames, trans.reshape(-1)]).cpu().numpy()
        R = int(runs.shape[0])
        return (packed[:4 * R].astype(np.int32).reshape(R, 4), packed[4 * R:4 * R + K].copy(),
                packed[4 * R + K:].reshape(K, K).copy())

    def most_likely_states(self, x):
        table, offsets = self.as_table(x)
        return self.table_states(table, offsets)

    # ------------------------------------------------------------------------------------------------------
    # one-step-ahead predictions (bn_hmm_predictive, bn_arhmm_predict)
    # ------------------------------------------------------------------------------------------------------
    def table_weights(self, table, offsets, weights='predictive'):
        """The state weights (n, K) the predictions are mixed with, a float64 device tensor: ``'predictive'``, the
        causal ``p(z_t | x_0 .. x_{t-1})`` (``bn_hmm_predictive``), or ``'smoothed'``, the posterior marginals
        ``gamma`` (``bn_hmm_forward_backward``), which have seen the whole trial."""
        from behavenet_amd import _hip
        if weights not in PREDICTION_WEIGHTS:
            raise ValueError('ARHMM: weights %r are not served (%s are)' % (weights, ', '.join(PREDICTION_WEIGHTS)))
        self._check_table(table)
        offsets_d = self._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        if weights == 'predictive':
            return _hip.hmm_predictive(ll, offsets_d, self.log_Ps, self.log_pi0)
        return _hip.hmm_forward_backward(ll, offsets_d, self.log_Ps, self.log_pi0)[0]

    def table_predictions(self, table, offsets, weights='predictive'):
        """``(xhat, valid)`` for every row of the table, device tensors float64 (n, D) and bool (n,):
        ``xhat_t = sum_k w_t[k] (b_k + sum_l A_k[l] x_{t-1-l})`` for row ``t >= lags`` of a trial, the row's own
        values before (nothing to predict from), zeros outside the trials; ``valid`` marks the in-trial rows with
        ``t >= max(lags, 1)``, on which the prediction and the persistence baseline ``x_{t-1}`` are both defined.
        Three launches (log-likelihoods, weights, the product); nothing crosses to the host."""
        import torch
        from behavenet_amd import _hip
        w = self.table_weights(table, offsets, weights)
        offsets_d = self._offsets_d(table, offsets)
        xhat = _hip.arhmm_predict(table, offsets_d, self.generative()[0], w, self.lags)
        n = int(table.shape[0])
        e = offsets_d.clamp(0, n)
        beg = torch.minimum(e[:-1] + max(self.lags, 1), e[1:])
        steps = torch.zeros((n + 1,), dtype=torch.int32, device=table.device)
        steps.index_add_(0, beg, torch.ones_like(beg, dtype=torch.int32))
        steps.index_add_(0, torch.maximum(e[1:], beg), -torch.ones_like(beg, dtype=torch.int32))
        return xhat, steps.cumsum(0)[:n] > 0

    def prediction_sums(self, table, offsets, weights='predictive'):
        """Per trial and dimension the count, ``sum x``, ``sum x^2`` and ``sum (x - pred)^2`` over the valid rows, for
        the model's prediction ([0]) and for the persistence baseline ``pred_t = x_{t-1}`` ([1]): a float64 host array
        ``(2, S, D, 4)`` for ``fitting.eval.summarise_label_sums``.  R^2 of a one-step prediction on smooth latents is
        close to 1 for any model; the baseline says what the model adds.  The prediction is rounded to fp32, the
        table's own format; both reductions are ``bn_segment_label_sums`` launches and ONE transfer follows."""
        return self.sums_of_predictions(table, offsets, *self.table_predictions(table, offsets, weights))

    def sums_of_predictions(self, table, offsets, xhat, valid):
        """``prediction_sums`` for predictions ``table_predictions`` has made already."""
        import torch
        from behavenet_amd import _hip
        offsets_d = self._offsets_d(table, offsets)
        mask = valid.to(torch.float32)[:, None].expand(-1, self.D).contiguous()
        previous = torch.zeros(tuple(table.shape), dtype=torch.float32, device=table.device)
        previous[1:] = table[:-1]
        sums = torch.stack([_hip.segment_label_sums(xhat.to(torch.float32), table, mask, offsets_d),
                            _hip.segment_label_sums(previous, table, mask, offsets_d)])
        return sums.cpu().numpy()

    def predict(self, x, weights='predictive'):
        """``table_predictions`` for ONE host trial (T, D): a float64 host array (T, D)."""
        table, offsets = self.as_table(x)
        return self.table_predictions(table, offsets, weights)[0].cpu().numpy()

    def smooth(self, x):
        """The posterior-weighted mean of the observation model for one trial (the library's ``smooth``)."""
        return self.predict(x, 'smoothed')

    # ------------------------------------------------------------------------------------------------------
    # exact multi-step forecasts (bn_arhmm_forecast_sums; bn_arhmm_predict for one horizon)
    # ------------------------------------------------------------------------------------------------------
    def forecast_maps(self, H):
        """``N (H, K, D, Q)``, ``Q = 1 + L D``, host float64: ``E[x_{t+h-1} | z_t = k, phi_t] = N[h - 1, k] phi_t``
        with ``phi_t = (1, x_{t-1}, .., x_{t-L})``, so that the exact h-step conditional mean is
        ``sum_k w_t[k] N[h - 1, k] phi_t`` with the causal weights ``w_t``.  Given a state path the mean is an affine
        recursion in ``phi_t`` and the path probabilities given ``z_t`` do not depend on ``phi_t``, so the maps are
        ``B_1[k][k'] = delta_kk' C_k``, ``B_{h+1}[k][k''] = C_k'' sum_k' P[k'][k''] B_h[k][k']`` with ``C_k`` the
        (Q, Q) companion matrix of state k (row 0 ``e_0``, rows 1 .. D ``[b_k | A_k]``, the lag blocks shifted down
        below) and ``N_h[k]`` rows 1 .. D of ``sum_k' B_h[k][k']``.  ``N[0]`` is ``generative()[0]`` element for
        element.  Without lags ``N_h[k] = sum_k' (P^{h-1})[k][k'] b_k'``.  The entries grow like the spectral radius
        of the ``A_k`` to the power h: a map that is not finite is a ValueError that names the horizon."""
        from behavenet_amd._hip import check_arhmm_horizons
        check_arhmm_horizons('ARHMM.forecast_maps', H)
        H, K, D, L = int(H), self.K, self.D, self.lags
        Q = 1 + L * D
        W = np.ascontiguousarray(np.concatenate([self.bs[:, :, None], self.As], axis=2).astype(np.float64))
        P = np.exp(np.asarray(self.log_Ps, dtype=np.float64))
        N = np.zeros((H, K, D, Q))
        N[0] = W
        with np.errstate(all='ignore'):
            if L == 0:
                reach = np.eye(K)                               # P^{h-1}
                for h in range(1, H):
                    reach = reach @ P
                    N[h, :, :, 0] = reach @ W[:, :, 0]
            else:
                C = np.zeros((K, Q, Q))
                C[:, 0, 0] = 1.0
                C[:, 1:1 + D, :] = W
                for i in range((L - 1) * D):
                    C[:, 1 + D + i, 1 + i] = 1.0
                B = np.zeros((K, K, Q, Q))
                B[np.arange(K), np.arange(K)] = C
                for h in range(1, H):
                    # sum_k' P[k'][k''] B[k][k'] for all (k, k'') as one product, then C_k'' from the left (batched)
                    B = np.matmul(C[None], np.matmul(P.T[None], B.reshape(K, K, Q * Q)).reshape(K, K, Q, Q))
                    N[h] = B.sum(axis=1)[:, 1:1 + D, :]
        for h in range(H):
            if not np.all(np.isfinite(N[h])):
                raise ValueError('ARHMM.forecast_maps: the map of horizon %d is not finite' % (h + 1))
        return N

    def forecast_sums(self, table, offsets, horizons=10, weights='predictive'):
        """The sums behind R^2 per horizon: a float64 host array ``(2, H, S, D, 4)``, ``[0]`` the model's exact h-step
        forecast ``E[x_{t+h-1} | x_0 .. x_{t-1}]``, ``[1]`` the persistence baseline ``x_{t-1}``, the last axis that
        of ``prediction_sums`` (count, ``sum y``, ``sum y^2``, ``sum (y - pred)^2`` with ``y = x_{t+h-1}``), over the
        origin rows ``t - beg >= max(lags, 1)`` with ``t + h - 1`` inside the trial.  The log-likelihoods, the causal
        weights and ONE launch for all horizons, scored in float64 in its epilogue (the forecasts are never written),
        then one transfer.  Only the causal weights are served: smoothed weights have seen the rows being forecast."""
        from behavenet_amd import _hip
        if weights != 'predictive':
            raise ValueError('ARHMM.forecast_sums: weights %r are not served (predictive are: smoothed weights have '
                             'seen the rows that are forecast)' % (weights,))
        N = self.forecast_maps(horizons)
        w = self.table_weights(table, offsets, 'predictive')
        five = _hip.arhmm_forecast_sums(table, self._offsets_d(table, offsets), N, w, self.lags).cpu().numpy()
        return np.stack([five[..., :4], five[..., [0, 1, 2, 4]]])

    def table_forecast(self, table, offsets, horizon):
        """``(xhat, valid)`` aligned with the TARGET row, device tensors float64 (n, D) and bool (n,): row t holds
        the forecast of ``x_t`` made ``horizon`` steps back, from the history before row ``t - horizon + 1``.  A row
        with no such origin in its trial (``t - beg < max(lags, 1) + horizon - 1``) holds its own values and is not
        valid; zeros outside the trials.  The unfused route: ``bn_arhmm_predict`` with the map of this horizon in
        place of ``[b_k | A_k]``, then a shift inside the trials -- what ``real_vs_sampled_movie`` gets laid beside the
        real latents."""
        import torch
        from behavenet_amd import _hip
        N = self.forecast_maps(horizon)[-1]
        back = int(horizon) - 1
        w = self.table_weights(table, offsets, 'predictive')
        offsets_d = self._offsets_d(table, offsets)
        at_origin = _hip.arhmm_predict(table, offsets_d, N, w, self.lags)
        n = int(table.shape[0])
        e = offsets_d.clamp(0, n)
        one = torch.ones_like(e[:-1], dtype=torch.int32)

        def rows_from(beg):                                 # the rows [beg[s], e[s + 1]) of every trial
            steps = torch.zeros((n + 1,), dtype=torch.int32, device=table.device)
            steps.index_add_(0, beg, one)
            steps.index_add_(0, torch.maximum(e[1:], beg), -one)
            return steps.cumsum(0)[:n] > 0
        inside = rows_from(e[:-1])
        valid = rows_from(torch.minimum(e[:-1] + max(self.lags, 1) + back, e[1:]))
        xhat = torch.zeros((n, self.D), dtype=torch.float64, device=table.device)
        xhat[inside] = table[inside].to(torch.float64)
        rows = valid.nonzero()[:, 0]
        xhat[rows] = at_origin[rows - back]
        return xhat, valid

    def forecast(self, x, horizon):
        """``table_forecast`` for ONE host trial (T, D): a float64 host array (T, D)."""
        table, offsets = self.as_table(x)
        return self.table_forecast(table, offsets, horizon)[0].cpu().numpy()

    # ------------------------------------------------------------------------------------------------------
    # the generative process (bn_arhmm_sample)
    # ------------------------------------------------------------------------------------------------------
    def generative(self):
        """``(W, C, cdf0, cdf)`` for ``bn_arhmm_sample``, host float64: ``W[k] = [b_k | A_k]`` (K, D, 1 + L D) in the
        model's own coordinates, ``C[k]`` the lower Cholesky factor of ``Sigma_k``, ``cdf0`` the cumulative sum in
        state order of ``exp(log_pi0)`` and ``cdf`` the same for every row of ``exp(log_Ps)``."""
        K, D = self.K, self.D
        W = np.concatenate([self.bs[:, :, None], self.As], axis=2).astype(np.float64)
        C = np.zeros((K, D, D))
        for k in range(K):
            try:
                C[k] = np.linalg.cholesky(self.Sigmas[k])
            except np.linalg.LinAlgError:
                raise ValueError('ARHMM.generative: Sigmas[%d] is not positive definite' % k)
            if not np.all(np.isfinite(C[k])):
                raise ValueError('ARHMM.generative: Sigmas[%d] is not finite' % k)
        return (np.ascontiguousarray(W), C, np.cumsum(np.exp(self.log_pi0)),
                np.cumsum(np.exp(self.log_Ps), axis=1))

    def sample_table(self, offsets, seed=0, states=None, init=None, device=None):
        """Latents and states of the trials ``offsets`` (int64 (S + 1), rows of ONE table of ``offsets[-1]`` rows)
        drawn from the model in ONE launch: ``(x, states)``, float64 (n, D) and int32 (n) device tensors.

        The noise comes from a ``torch.Generator`` on the device seeded with ``seed``: ``eps`` (n, D) standard normals
        first, then -- when ``states`` is None -- ``u`` (n) uniforms, both float64.  So the draws are reproducible for
        a given seed, device and torch build only; that is torch's generator, the launch itself is a deterministic
        function of the noise.  ``states``: int32 (n), given states (host arrays are uploaded; a state outside
        [0, K) is a ValueError).  ``init``: fp32 (n, D) whose rows are a trial's first ``lags`` rows; without it those
        rows are N(0, I), the model's own density for them."""
        import torch
        from behavenet_amd import _hip
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets),
                                       dtype=np.int64)
        if offsets.ndim != 1 or offsets.size < 1:
            raise ValueError('ARHMM.sample_table: expected offsets (S + 1,), got %s' % (offsets.shape,))
        _hip.check_arhmm_dims('ARHMM.sample_table', self.D, self.lags, self.K)
        n = max(int(offsets.max()), 0)
        W, C, cdf0, cdf = self.generative()
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        eps = torch.randn((n, self.D), dtype=torch.float64, device=device, generator=gen)
        u = None
        if states is None:
            u = torch.rand((n,), dtype=torch.float64, device=device, generator=gen)
        elif not torch.is_tensor(states):
            states = torch.from_numpy(np.ascontiguousarray(np.asarray(states), dtype=np.int32)).to(device)
        if init is not None and not torch.is_tensor(init):
            init = torch.from_numpy(np.ascontiguousarray(np.asarray(init), dtype=np.float32)).to(device)
        return _hip.arhmm_sample(W, C, cdf0, cdf, offsets, eps, u=u, states=states, init=init)

    def sample(self, T, n_samples=1, burn_in=200, seed=0):
        """``n_samples`` trials of ``T`` rows generated by the model, states and latents both drawn:
        ``(states_list, latents_list)`` of host arrays (T,) int32 and (T, D) float64.  Every trial runs for
        ``T + burn_in`` rows and the first ``burn_in`` are dropped -- the reference's ``hmm.sample(T + 200)[200:]``
        loop (plotting/arhmm_utils.py) -- in one launch.  Reproducible for a seed, device and torch build
        (``sample_table``)."""
        from behavenet_amd import _hip
        T, n_samples, burn_in = int(T), int(n_samples), int(burn_in)
        if T < 0 or n_samples < 0 or burn_in < 0:
            raise ValueError('ARHMM.sample: T %d, n_samples %d, burn_in %d' % (T, n_samples, burn_in))
        _hip.check_arhmm_dims('ARHMM.sample', self.D, self.lags, self.K)
        per = T + burn_in
        if not n_samples or not per:
            return ([np.zeros((T,), dtype=np.int32) for _ in range(n_samples)],
                    [np.zeros((T, self.D)) for _ in range(n_samples)])
        offsets = np.arange(n_samples + 1, dtype=np.int64) * per
        x, z = self.sample_table(offsets, seed=seed)
        x, z = x.cpu().numpy(), z.cpu().numpy()
        return ([z[i * per + burn_in:(i + 1) * per].copy() for i in range(n_samples)],
                [x[i * per + burn_in:(i + 1) * per].copy() for i in range(n_samples)])

    def sample_conditional(self, datas, seed=0):
        """Latents drawn from the model along the most likely state path of every trial of ``datas`` (the reference's
        ``cond_sampling=True``): ``(states_list, latents_list)`` of host arrays.  One ``table_states`` call gives the
        Viterbi paths, one launch the samples; the first ``lags`` rows of a sampled trial are the real trial's."""
        table, offsets = self.as_table(datas)
        self._check_table(table)
        states = self.table_states(table, offsets)
        x, z = self.sample_table(offsets, seed=seed, states=states, init=table, device=table.device)
        x, z = x.cpu().numpy(), z.cpu().numpy()
        S = len(offsets) - 1
        return ([z[offsets[i]:offsets[i + 1]].copy() for i in range(S)],
                [x[offsets[i]:offsets[i + 1]].copy() for i in range(S)])


class ARHMMGroup(object):
    """``M`` models with the same ``D`` and ``lags`` that advance one EM iteration in ONE set of launches on one table
    ("ARHMM: a grid of models"): their states lie side by side as ``KT = sum K_m`` columns of the
    folded parameters, of ``ll`` and of ``gamma`` (``bn_arhmm_grid_loglik``, ``bn_hmm_grid_forward_backward``,
    ``bn_arhmm_grid_moments``).  The group holds references to its models and numpy arrays only; every model keeps its
    own host M-step."""

    def __init__(self, models):
        from behavenet_amd import _hip
        models = list(models)
        if not models:
            raise ValueError('ARHMMGroup: no models')
        for m in models:
            if not isinstance(m, ARHMM):
                raise ValueError('ARHMMGroup: expected ARHMM models, got %s' % type(m).__name__)
            if (m.D, m.lags) != (models[0].D, models[0].lags):
                raise ValueError('ARHMMGroup: the models of a group share D and lags, got (%d, %d) and (%d, %d)'
                                 % (models[0].D, models[0].lags, m.D, m.lags))
        self.models = models
        self.D, self.lags = models[0].D, models[0].lags
        self.Ks = np.asarray([m.K for m in models], dtype=np.int64)
        self.koff, self.xoff = _hip.check_arhmm_grid_states('ARHMMGroup', self.Ks)
        _hip.check_arhmm_grid_dims('ARHMMGroup', self.D, self.lags, int(self.koff[-1]))

    @property
    def M(self):
        return len(self.models)

    @property
    def KT(self):
        return int(self.koff[-1])

    @property
    def P(self):
        return 1 + (self.lags + 1) * self.D

    def fold(self):
        """``(G, cst)`` of all states side by side: (KT, D, P) and (KT,)."""
        folded = [m.fold() for m in self.models]
        return np.concatenate([f[0] for f in folded], axis=0), np.concatenate([f[1] for f in folded])

    def set_shift(self, table):
        """The shift is a property of the table: computed once, as ``ARHMM.set_shift`` computes it, for every model."""
        shift = self.models[0].set_shift(table)
        for m in self.models[1:]:
            m.shift = shift.copy()
        return shift

    def _shift(self):
        shift = self.models[0].shift
        for m in self.models[1:]:
            if not np.array_equal(m.shift, shift):
                raise ValueError('ARHMMGroup: the models of a group share the shift of their table (set_shift)')
        return shift

    def _transitions(self):
        return (np.concatenate([m.log_Ps.reshape(-1) for m in self.models]),
                np.concatenate([m.log_pi0 for m in self.models]))

    def _loglik_table(self, table, offsets_d):
        from behavenet_amd import _hip
        G, cst = self.fold()
        return _hip.arhmm_grid_loglik(table, offsets_d, G, cst, self.lags, shift=self._shift())

    def trial_logliks(self, table, offsets):
        """The log-likelihood of every trial under every model, a float64 host array (M, S) (forward sweep only)."""
        from behavenet_amd import _hip
        self.models[0]._check_table(table)
        offsets_d = self.models[0]._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        log_Ps, log_pi0 = self._transitions()
        return _hip.hmm_grid_forward_backward(ll, offsets_d, self.Ks, log_Ps, log_pi0,
                                              want_posteriors=False)[2].cpu().numpy()

    def table_states_device(self, table, offsets):
        """The Viterbi paths of every trial under every model: an int32 DEVICE tensor (M, n), row m what
        ``models[m].table_states`` returns.  One grid log-likelihood launch and one Viterbi launch a class
        (``bn_hmm_grid_viterbi``); nothing crosses to the host."""
        from behavenet_amd import _hip
        self.models[0]._check_table(table)
        offsets_d = self.models[0]._offsets_d(table, offsets)
        ll = self._loglik_table(table, offsets_d)
        log_Ps, log_pi0 = self._transitions()
        return _hip.hmm_grid_viterbi(ll, offsets_d, self.Ks, log_Ps, log_pi0)

    def table_states(self, table, offsets):
        """``table_states_device`` on the host: a list of M int32 arrays (n,), one transfer for the group."""
        states = self.table_states_device(table, offsets).cpu().numpy()
        return [states[i].copy() for i in range(self.M)]

    def table_runs(self, table, offsets):
        """Per model the ``(runs, frames, trans)`` of ``ARHMM.table_runs``, host arrays.  Log-likelihoods, Viterbi and
        the run searches of all models follow each other on the device; the states never leave it and the results
        cross in TWO transfers for the whole group (``_hip.state_runs_grid``: the statistics, then the trimmed runs)."""
        from behavenet_amd import _hip
        states = self.table_states_device(table, offsets)
        return _hip.state_runs_grid(states, self.models[0]._offsets_d(table, offsets), self.Ks)

    def e_step(self, table, offsets):
        """Per model the ``(moments, gamma_init, xi_sum, gamma0_sum, logliks)`` of ``ARHMM.e_step``, host arrays, from
        three launches and ONE transfer for the whole group."""
        import torch
        from behavenet_amd import _hip
        self.models[0]._check_table(table)
        offsets_d = self.models[0]._offsets_d(table, offsets)
        M, KT, P, XT = self.M, self.KT, self.P, int(self.xoff[-1])
        ll = self._loglik_table(table, offsets_d)
        log_Ps, log_pi0 = self._transitions()
        gamma, xi, lls = _hip.hmm_grid_forward_backward(ll, offsets_d, self.Ks, log_Ps, log_pi0)
        del ll
        mom, ginit = _hip.arhmm_grid_moments(table, offsets_d, gamma, self.lags, shift=self._shift())
        first = offsets_d[:-1][offsets_d[1:] > offsets_d[:-1]]
        g0 = gamma.index_select(0, first).sum(dim=0) if first.numel() else gamma.new_zeros((KT,))
        S = int(lls.shape[1])
        packed = torch.cat([mom.reshape(-1), ginit, xi.sum(dim=0), g0, lls.reshape(-1)]).cpu().numpy()
        o = np.cumsum([0, KT * P * P, KT, XT, KT])
        mom, ginit, xi_sum, g0 = (packed[o[0]:o[1]].reshape(KT, P, P), packed[o[1]:o[2]], packed[o[2]:o[3]],
                                  packed[o[3]:o[4]])
        lls = packed[o[4]:].reshape(M, S)
        out = []
        for i, m in enumerate(self.models):
            k0, k1, x0, x1 = self.koff[i], self.koff[i + 1], self.xoff[i], self.xoff[i + 1]
            out.append((mom[k0:k1], ginit[k0:k1], xi_sum[x0:x1].reshape(m.K, m.K), g0[k0:k1], lls[i]))
        return out

    def m_step(self, stats):
        """Every model's own host M-step on its five-tuple of ``e_step``."""
        for m, (mom, _, xi_sum, g0, _) in zip(self.models, stats):
            m.m_step(mom, xi_sum, g0)

    def em_step(self, table, offsets):
        """One EM iteration of every model; returns the per-trial log-likelihoods (M, S) of the parameters BEFORE the
        update."""
        stats = self.e_step(table, offsets)
        self.m_step(stats)
        return np.stack([s[4] for s in stats]) if stats else np.zeros((0, 0))
