"""The session classifier on latents: the host side ("session classifier").

The reference scores an MSPS-VAE by ``fc``, the fraction of frames whose session sklearn's
``LogisticRegressionCV(Cs=<8 values>, cv=5, penalty='l2', multi_class='multinomial')`` recovers from the
session-independent latents (``fit_classifier``, plotting/cond_ae_utils.py:1282-1369).  With one weight row a class,
intercepts unpenalised, sklearn's ``LogisticRegression(C)`` minimises

    F(W, b) = (1 / n) sum_rows [logsumexp_k(l_k) - l_y] + ||W||^2 / (2 C n),          l = W z + b

and the ``n_splits x len(Cs)`` models of the cross-validation differ only in C and in the fold they leave out.  Here
they are fitted together: ``evaluate(W)`` returns the data sums of all models in one pass over the table (on the
device ``bn_softmax_cv_lossgrad``, in the CPU tests a numpy float64 evaluator) and the optimiser -- a batched L-BFGS,
float64 numpy -- runs on the host, where only ``M (S (D + 1) + 2)`` doubles an iteration arrive.

Nothing here imports torch or touches a GPU."""

import warnings

import numpy as np

__all__ = ['stratified_folds', 'softmax_objective', 'fit_softmax_lockstep', 'cross_validate', 'SessionClassifier',
           'DEFAULT_CS']

DEFAULT_CS = (0.00001, 0.0001, 0.001, 0.01, 0.1, 1, 10, 100)          # the reference's grid
HISTORY = 10                    # L-BFGS pairs kept
ARMIJO = 1e-4                   # sufficient decrease: F(x + t d) <= F(x) + ARMIJO t g.d
MAX_BACKTRACKS = 30
FLAT = 2.0 ** -50               # |F(x + t d) - F(x)| <= FLAT |F|: the difference is rounding noise


def stratified_folds(y, n_splits=5):
    """int32 fold ids ``(n,)`` equal to the test folds of sklearn's ``StratifiedKFold(n_splits)`` without shuffling:
    with the classes numbered in the order of their first rows, fold i gets of class k as many rows as
    ``sorted(y)[i::n_splits]`` holds of k, and within a class the rows take the folds 0, 1, ... in row order, as
    contiguous blocks.  A class with fewer than ``n_splits`` rows: ValueError."""
    y = np.asarray(y)
    if y.ndim != 1 or y.size < 1:
        raise ValueError('stratified_folds: expected class ids (n,), got %s' % (tuple(y.shape),))
    if n_splits < 2:
        raise ValueError('stratified_folds: %d folds (at least 2)' % n_splits)
    classes, first, y_idx = np.unique(y, return_index=True, return_inverse=True)
    counts = np.bincount(y_idx, minlength=len(classes))
    if counts.min() < n_splits:
        raise ValueError('stratified_folds: class %s has %d rows, fewer than the %d folds'
                         % (classes[int(np.argmin(counts))], int(counts.min()), n_splits))
    # (sklearn numbers the classes in the order of their first rows before it sorts: the allocation depends on it)
    y_idx = np.argsort(np.argsort(first))[y_idx]
    y_sorted = np.sort(y_idx)
    allocation = np.asarray([np.bincount(y_sorted[i::n_splits], minlength=len(classes)) for i in range(n_splits)])
    folds = np.empty(len(y), dtype=np.int32)
    for k in range(len(classes)):
        folds[y_idx == k] = np.arange(n_splits, dtype=np.int32).repeat(allocation[:, k])
    return folds


def softmax_objective(W, loss, grad, Cs, ns):
    """``(F, dF)`` per model, ``(M,)`` and ``(M, S, D + 1)``, from the data sums ``loss (M,)`` and ``grad
    (M, S, D + 1)`` at the weights ``W (M, S, D + 1)`` (column D the intercept, unpenalised):
    ``F = loss / n + ||W[..., :D]||^2 / (2 C n)``."""
    Cs, ns = np.asarray(Cs, dtype=np.float64), np.asarray(ns, dtype=np.float64)
    pen = W.copy()
    pen[..., -1] = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        F = loss / ns + np.einsum('msd,msd->m', pen, pen) / (2.0 * Cs * ns)
        dF = grad / ns[:, None, None] + pen / (Cs * ns)[:, None, None]
    return F, dF


def _directions(g, s_hist, y_hist, rho):
    """``-H g`` per model by the two-loop recursion over histories ``(M, HISTORY, P)``, oldest first; a slot with
    ``rho == 0`` is empty and passes the vector through."""
    q = g.copy()
    alphas = np.zeros(rho.shape)
    for i in range(HISTORY - 1, -1, -1):
        alphas[:, i] = rho[:, i] * np.einsum('mp,mp->m', s_hist[:, i], q)
        q -= alphas[:, i, None] * y_hist[:, i]
    yy = np.einsum('mp,mp->m', y_hist[:, -1], y_hist[:, -1])
    with np.errstate(divide='ignore', invalid='ignore'):
        gamma = np.where(rho[:, -1] > 0, 1.0 / (rho[:, -1] * yy), 1.0)
    q *= gamma[:, None]
    for i in range(HISTORY):
        beta = rho[:, i] * np.einsum('mp,mp->m', y_hist[:, i], q)
        q += (alphas[:, i] - beta)[:, None] * s_hist[:, i]
    return -q


def _first_step(g):
    return 1.0 / np.maximum(1.0, np.sqrt(np.einsum('mp,mp->m', g, g)))


def fit_softmax_lockstep(evaluate, M, S, D, Cs_of_model, n_of_model, tol=1e-4, max_iter=100, W0=None):
    """Minimise ``F`` (module docstring) for M models at once -> ``(W (M, S, D + 1), n_iter (M,), converged (M,))``.

    ``evaluate(W) -> (loss, grad, count)`` returns the data sums of all models at the weights ``W (M, S, D + 1)``;
    ``Cs_of_model`` and ``n_of_model`` are each model's C and the number of rows it includes (``count`` must say the
    same).  Every model runs its own L-BFGS (history 10) with a backtracking line search, in float64 numpy, but all
    advance together: one call of ``evaluate`` takes one trial point from every model that is still running -- the
    next quasi-Newton step for a model whose last trial was accepted, a shorter step along the same direction for
    one whose trial was not.  A trial is accepted when ``F(x + t d) <= F(x) + 1e-4 t g.d``; where the two values of F
    differ by rounding noise alone (``2^-50 |F|``) the slope decides instead, ``g(x + t d).d <= (2e-4 - 1) g.d``,
    Hager and Zhang's approximate form of the same condition.  A model stops when ``||dF||_inf <= tol`` (converged),
    after ``max_iter`` accepted steps, or when 30 shortenings of a steepest-descent step find no decrease; it is
    frozen then: its weights are passed on to ``evaluate`` bit for bit and never written again.  Models that did not
    converge: one ConvergenceWarning-like ``UserWarning``, no error."""
    Cs_of_model = np.asarray(Cs_of_model, dtype=np.float64).reshape(M)
    n_of_model = np.asarray(n_of_model, dtype=np.float64).reshape(M)
    if np.any(n_of_model < 1) or np.any(Cs_of_model <= 0):
        raise ValueError('fit_softmax_lockstep: every model needs rows and a positive C')
    P = S * (D + 1)
    x = np.zeros((M, P)) if W0 is None else np.array(W0, dtype=np.float64).reshape(M, P)

    def objective(points):
        W = points.reshape(M, S, D + 1)
        loss, grad, count = evaluate(W)
        if not np.array_equal(np.asarray(count, dtype=np.float64).reshape(M), n_of_model):
            raise ValueError('fit_softmax_lockstep: the evaluator counted %s rows, the caller %s'
                             % (np.asarray(count).tolist(), n_of_model.tolist()))
        F, dF = softmax_objective(W, np.asarray(loss, dtype=np.float64).reshape(M),
                                  np.asarray(grad, dtype=np.float64).reshape(M, S, D + 1), Cs_of_model, n_of_model)
        return F, dF.reshape(M, P)

    f, g = objective(x)
    if not (np.isfinite(f).all() and np.isfinite(g).all()):
        raise ValueError('fit_softmax_lockstep: the objective is not finite at the starting point (models %s)'
                         % np.nonzero(~np.isfinite(f))[0].tolist())
    n_iter = np.zeros(M, dtype=np.int64)
    converged = np.abs(g).max(axis=1) <= tol
    active = ~converged
    if max_iter < 1:
        active[:] = False
    s_hist, y_hist, rho = np.zeros((M, HISTORY, P)), np.zeros((M, HISTORY, P)), np.zeros((M, HISTORY))
    d = -g
    gd = np.einsum('mp,mp->m', g, d)
    t = _first_step(g)
    backtracks = np.zeros(M, dtype=np.int64)
    while active.any():
        trial = x.copy()                                   # (a frozen model's row is its own weights, untouched)
        trial[active] = x[active] + t[active, None] * d[active]
        ft, gt = objective(trial)
        with np.errstate(invalid='ignore'):
            gtd = np.einsum('mp,mp->m', gt, d)
            fine = np.isfinite(ft) & np.isfinite(gt).all(axis=1)
            decrease = ft <= f + ARMIJO * t * gd
            flat = (np.abs(ft - f) <= FLAT * np.abs(f)) & (gtd <= (2.0 * ARMIJO - 1.0) * gd)
        accept = active & fine & (decrease | flat)
        reject = active & ~accept
        if accept.any():
            a = np.nonzero(accept)[0]
            s, yv = trial[a] - x[a], gt[a] - g[a]
            x[a], f[a], g[a] = trial[a], ft[a], gt[a]
            n_iter[a] += 1
            sy, yy = np.einsum('mp,mp->m', s, yv), np.einsum('mp,mp->m', yv, yv)
            keep = sy > 2.2e-16 * yy                       # (a pair without curvature is not kept)
            k = a[keep]
            s_hist[k] = np.roll(s_hist[k], -1, axis=1)
            y_hist[k] = np.roll(y_hist[k], -1, axis=1)
            rho[k] = np.roll(rho[k], -1, axis=1)
            s_hist[k, -1], y_hist[k, -1], rho[k, -1] = s[keep], yv[keep], 1.0 / sy[keep]
            done = np.abs(g[a]).max(axis=1) <= tol
            converged[a[done]] = True
            active[a[done | (n_iter[a] >= max_iter)]] = False
            d[a] = _directions(g[a], s_hist[a], y_hist[a], rho[a])
            gd[a] = np.einsum('mp,mp->m', g[a], d[a])
            uphill = a[~(gd[a] < 0)]                       # (cannot happen with kept pairs of positive curvature)
            rho[uphill] = 0.0
            d[uphill] = -g[uphill]
            gd[uphill] = np.einsum('mp,mp->m', g[uphill], d[uphill])
            t[a] = 1.0
            t[uphill] = _first_step(g[uphill])
            backtracks[a] = 0
        if reject.any():
            r = np.nonzero(reject)[0]
            backtracks[r] += 1
            with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                # the minimiser of the parabola through F(x), its slope and F(x + t d), kept within [0.1 t, 0.5 t]
                quad = -gd[r] * t[r] ** 2 / (2.0 * (ft[r] - f[r] - gd[r] * t[r]))
            quad = np.where(np.isfinite(quad), quad, 0.1 * t[r])
            t[r] = np.clip(quad, 0.1 * t[r], 0.5 * t[r])
            spent = r[backtracks[r] > MAX_BACKTRACKS]
            had_history = rho[spent].any(axis=1)
            again = spent[had_history]                     # once more along the plain gradient
            rho[again] = 0.0
            d[again] = -g[again]
            gd[again] = np.einsum('mp,mp->m', g[again], d[again])
            t[again] = _first_step(g[again])
            backtracks[again] = 0
            active[spent[~had_history]] = False
    if not converged.all():
        warnings.warn('fit_softmax_lockstep: %d of %d models did not reach ||dF||_inf <= %g within %d iterations '
                      '(the worst is at %.3g); increase max_iter or tol'
                      % (int((~converged).sum()), M, tol, max_iter, float(np.abs(g[~converged]).max())), UserWarning)
    return x.reshape(M, S, D + 1), n_iter, converged


class SessionClassifier(object):
    """The fitted classifier, with the attributes sklearn's ``LogisticRegressionCV`` reports: ``coef_ (S, D)`` -- for
    two classes ``(1, D)``, the weight row of class 1, as sklearn has it --, ``intercept_`` (centred to sum zero over
    the classes before the same selection), ``C_`` (one float), ``Cs_``, ``scores_ (n_splits, len(Cs))`` the held-out
    accuracy of every (fold, C), ``classes_``, ``n_iter_ (n_splits, len(Cs))`` and ``refit_n_iter_``; ``weights_`` is
    the full ``(S, D + 1)`` table, ``cv_weights_ (n_splits, len(Cs), S, D + 1)`` those of the fold models and
    ``columns_`` the latents the rows were made of.  ``decision_function``, ``predict_proba`` and ``predict`` run in numpy float64 on
    the host."""

    def __init__(self, weights, classes, C, Cs, scores, n_iter, refit_n_iter=0, converged=True, columns=None,
                 cv_weights=None):
        weights = np.array(weights, dtype=np.float64)
        weights[:, -1] -= weights[:, -1].mean()
        self.weights_ = weights
        self.classes_ = np.asarray(classes)
        two = weights.shape[0] == 2
        self.coef_ = weights[1:, :-1].copy() if two else weights[:, :-1].copy()
        self.intercept_ = weights[1:, -1].copy() if two else weights[:, -1].copy()
        self.C_ = float(C)
        self.Cs_ = np.asarray(Cs, dtype=np.float64)
        self.scores_ = np.asarray(scores, dtype=np.float64)
        self.n_iter_ = np.asarray(n_iter)
        self.refit_n_iter_ = int(refit_n_iter)
        self.converged_ = bool(converged)
        self.columns_ = columns
        self.cv_weights_ = cv_weights

    def decision_function(self, z):
        z = np.asarray(z, dtype=np.float64)
        scores = z @ self.coef_.T + self.intercept_
        return scores[:, 0] if scores.shape[1] == 1 else scores

    def predict_proba(self, z):
        d = self.decision_function(z)
        if d.ndim == 1:
            d = np.stack([-d, d], axis=1)
        e = np.exp(d - d.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def predict(self, z):
        d = self.decision_function(z)
        return self.classes_[(d > 0).astype(np.int64) if d.ndim == 1 else np.argmax(d, axis=1)]


def cross_validate(lossgrad, score, fold_counts, S, D, Cs=DEFAULT_CS, tol=1e-4, max_iter=100, classes=None,
                   columns=None):
    """The whole procedure of ``LogisticRegressionCV`` on evaluators: fit the ``n_splits x len(Cs)`` models in
    lockstep, score each on the fold it left out, choose ``C_`` -- the argmax of the fold mean, the first maximum --
    and refit on all rows at ``C_`` from the fold mean of the weights at ``C_``  -> ``SessionClassifier``.

    ``lossgrad(W, leave) -> (loss, grad, count)`` and ``score(W, leave) -> (M, 2)`` hits and rows take weights
    ``(M, S, D + 1)`` and the int32 fold each model leaves out (-1: none); ``fold_counts`` holds the rows of every
    fold, ``(n_splits,)``.  Model ``i len(Cs) + j`` leaves fold i out at ``Cs[j]``."""
    Cs = np.asarray(Cs, dtype=np.float64)
    fold_counts = np.asarray(fold_counts, dtype=np.int64)
    n_splits, n = len(fold_counts), int(fold_counts.sum())
    M = n_splits * len(Cs)
    if Cs.ndim != 1 or Cs.size < 1 or np.any(Cs <= 0):
        raise ValueError('session classifier: Cs must be positive values, got %r' % (Cs,))
    if M > 64:
        raise ValueError('session classifier: %d folds x %d values of C = %d models (64 a launch are served)'
                         % (n_splits, len(Cs), M))
    leave = np.repeat(np.arange(n_splits, dtype=np.int32), len(Cs))
    W, n_iter, conv = fit_softmax_lockstep(lambda w: lossgrad(w, leave), M, S, D, np.tile(Cs, n_splits),
                                           (n - fold_counts).repeat(len(Cs)), tol, max_iter)
    held = np.asarray(score(W, leave), dtype=np.float64).reshape(M, 2)
    if not np.array_equal(held[:, 1], fold_counts.repeat(len(Cs))):
        raise ValueError('session classifier: the scorer counted %s held-out rows, the folds hold %s'
                         % (held[:, 1].tolist(), fold_counts.tolist()))
    scores = (held[:, 0] / held[:, 1]).reshape(n_splits, len(Cs))
    best = int(np.argmax(scores.mean(axis=0)))
    start = W.reshape(n_splits, len(Cs), S, D + 1)[:, best].mean(axis=0)[None]
    none = np.full(1, -1, dtype=np.int32)
    final, refit_iter, refit_conv = fit_softmax_lockstep(lambda w: lossgrad(w, none), 1, S, D, Cs[best:best + 1],
                                                         [n], tol, max_iter, W0=start)
    return SessionClassifier(final[0], np.arange(S) if classes is None else classes, Cs[best], Cs, scores,
                             n_iter.reshape(n_splits, len(Cs)), refit_iter[0], conv.all() and refit_conv.all(),
                             columns, W.reshape(n_splits, len(Cs), S, D + 1))
