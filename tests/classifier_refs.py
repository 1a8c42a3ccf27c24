"""What the session-classifier tests share (tests/test_classifier_cpu.py, tests/test_gpu_classifier.py): the
reference of ``bn_softmax_cv_lossgrad`` and ``bn_softmax_cv_score`` in numpy float64 with ``math.fsum`` per output
entry -- so the reference's sums carry no summation error --, the derived tolerance, a fast numpy evaluator that drives
``fitting.classifier`` on the CPU, the objective written out on its own, the oracle procedure and the input families.

Tolerance.  ``u = 2^-53``.  Device and reference start from the same fp32 rows and float64 weights.

1. Logits.  ``l_k = sum_{j < D} w_kj z_j + b_k`` is a chain of D + 1 float64 terms, on the device fused multiply-adds
   in k order, in the reference numpy's dot product.  Either is within ``(D + 1) u A_k`` of the exact value,
   ``A_k = sum_j |w_kj z_j| + |b_k|`` (Higham, gamma_{D+1}).  The shifted exponent ``l_k - top`` rounds once more,
   ``u |l_k - top| <= 2 u A``.  Both sides together:
       delta_i = 2 (D + 3) u max_k A_ik                                   per row i and model.
2. ``exp`` and ``log``.  Budget ``E = 3`` ulp each: OpenCL's bound for the double-precision functions, which the
   device library states it meets; numpy's libm is within 1.
3. A row's loss ``t = (top - l_y) + log(sum_k exp(l_k - top))``.  ``d logsumexp / d l_k = p_k`` and ``sum p_k = 1``,
   so the logit errors move ``t`` by at most ``2 delta``.  The S exponentials carry ``(E + 1) u`` each, their sum
   ``(S - 1) u``, the logarithm turns that relative error into an absolute one and adds ``E u |log sum| <= E u log S
   <= 3 E u``, and the two additions round: ``u (|top - l_y| + |t|) <= u (2 A + |t|)``.
       tau_i = 2 delta_i + 2 u A_i + (4 E + S + 2) u (1 + |t_i|)
4. A residual ``r_k = p_k - [k = y]``.  ``p_k = e_k / sum``: the exponent errors scale it by ``exp(+-2 delta)``, the
   exponentials, the sum and the division by ``(2 E + S + 3) u``, and the subtraction rounds once:
       rho_ik = (2 delta_i + (2 E + S + 4) u) max(p_ik, |r_ik|)
   and the gradient term ``r_k z_j`` (``z_j`` is exact, 1 for the intercept) is off by ``rho_ik |z_ij|``.
5. Sums of m terms in any order: ``4 m u sum |term|``, the project's bound (tests/label_r2_refs.py), which also covers
   the product's one rounding.
       |loss - ref|  <= sum_i tau_i + 4 m u sum_i |t_i|
       |grad - ref|  <= sum_i rho_ik |z_ij| + 4 m u sum_i |r_ik z_ij|
   both doubled, because the reference's own ``t_i`` and ``r_ik`` carry the errors of steps 1 to 4 as well.
Counts are exact; NaN positions must agree exactly.

Scores.  The device's argmax can differ from the reference's only on a row whose two largest logits are within
``2 delta_i`` of one another; ``near_ties`` counts those rows, and the tests' inputs have none but the exact ties
they plant (equal weight rows give equal bits on both sides)."""

import math

import numpy as np

U = 2.0 ** -53
ULP_BUDGET = 3


def _fsum(terms):
    return math.fsum(terms.tolist()) if np.isfinite(terms).all() else float(np.sum(terms))


def includes(y, fold, leave, S):
    """bool (n, M): the rows model m includes -- a class in [0, S) and a fold other than ``leave[m]``."""
    y, leave = np.asarray(y), np.asarray(leave)
    fold = np.full(len(y), -1) if fold is None else np.asarray(fold)
    valid = (y >= 0) & (y < S)
    return valid[:, None] & ~((leave[None, :] >= 0) & (fold[:, None] == leave[None, :]))


def scored(y, fold, leave, S):
    """bool (n, M): the rows model m is scored on -- a class in [0, S) and the fold ``leave[m]`` (-1: every fold)."""
    y, leave = np.asarray(y), np.asarray(leave)
    fold = np.full(len(y), -1) if fold is None else np.asarray(fold)
    valid = (y >= 0) & (y < S)
    return valid[:, None] & ((leave[None, :] < 0) | (fold[:, None] == leave[None, :]))


def logits_ref(z, W):
    """float64 (n, M, S) logits and (n, M) ``max_k A_k`` of the fp32 rows ``z`` under the weights ``W (M, S, D + 1)``."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        logit = np.einsum('nd,msd->nms', z64, W[..., :-1]) + W[..., -1]
        mag = (np.einsum('nd,msd->nms', np.abs(z64), np.abs(W[..., :-1])) + np.abs(W[..., -1])).max(axis=2)
    return logit, mag


def lossgrad_ref(z, y, fold, W, leave):
    """-> ``(loss (M,), grad (M, S, D + 1), count (M,), loss_tol (M,), grad_tol (M, S, D + 1))``: the sums of
    ``bn_softmax_cv_lossgrad`` with ``math.fsum`` and the tolerances of the module docstring."""
    z = np.asarray(z, dtype=np.float32)
    n, D = z.shape
    M, S = W.shape[:2]
    y = np.asarray(y)
    inc = includes(y, fold, leave, S)
    logit, mag = logits_ref(z, W)
    za = np.concatenate([z.astype(np.float64), np.ones((n, 1))], axis=1)
    loss, count = np.zeros(M), inc.sum(axis=0).astype(np.float64)
    grad, loss_tol, grad_tol = np.zeros((M, S, D + 1)), np.zeros(M), np.zeros((M, S, D + 1))
    E = ULP_BUDGET
    for m in range(M):
        rows = np.nonzero(inc[:, m])[0]
        if not len(rows):
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            l = logit[rows, m]
            top = l.max(axis=1, keepdims=True)
            e = np.exp(l - top)
            p = e / e.sum(axis=1, keepdims=True)
            ly = l[np.arange(len(rows)), y[rows]]
            t = (top[:, 0] - ly) + np.log(e.sum(axis=1))
            r = p.copy()
            r[np.arange(len(rows)), y[rows]] -= 1.0
            delta = 2 * (D + 3) * U * mag[rows, m]
            tau = 2 * delta + 2 * U * mag[rows, m] + (4 * E + S + 2) * U * (1 + np.abs(t))
            rho = (2 * delta + (2 * E + S + 4) * U)[:, None] * np.maximum(p, np.abs(r))
            loss[m] = _fsum(t)
            loss_tol[m] = 2 * (_fsum(tau) + 4 * len(rows) * U * _fsum(np.abs(t)))
            for k in range(S):
                for j in range(D + 1):
                    terms = r[:, k] * za[rows, j]
                    grad[m, k, j] = _fsum(terms)
                    grad_tol[m, k, j] = 2 * (_fsum(rho[:, k] * np.abs(za[rows, j]))
                                             + 4 * len(rows) * U * _fsum(np.abs(terms)))
    return loss, grad, count, loss_tol, grad_tol


def score_ref(z, y, fold, W, leave):
    """-> ``(out (M, 2), near (M,))``: hits and rows of ``bn_softmax_cv_score`` by ``np.argmax`` (ties and rows of
    NaNs to the lowest class), and the scored rows whose two largest logits lie within ``2 delta`` of one another
    without being equal."""
    z = np.asarray(z, dtype=np.float32)
    D = z.shape[1]
    M, S = W.shape[:2]
    y = np.asarray(y)
    sc = scored(y, fold, leave, S)
    logit, mag = logits_ref(z, W)
    pred = np.argmax(logit, axis=2)
    hits = ((pred == y[:, None]) & sc).sum(axis=0)
    with np.errstate(invalid='ignore'):
        two = np.sort(logit, axis=2)[:, :, -2:]
        gap = two[:, :, 1] - two[:, :, 0]
        near = (gap > 0) & (gap <= 2 * 2 * (D + 3) * U * mag) & sc
    return np.stack([hits, sc.sum(axis=0)], axis=1).astype(np.float64), near.sum(axis=0)


def assert_lossgrad_close(got, want, what=''):
    loss, grad, count = (np.asarray(a) for a in got)
    w_loss, w_grad, w_count, loss_tol, grad_tol = want
    assert loss.dtype == grad.dtype == count.dtype == np.float64, what
    assert loss.shape == w_loss.shape and grad.shape == w_grad.shape and count.shape == w_count.shape, what
    assert np.array_equal(count, w_count), (what, 'counts', count, w_count)
    for name, g, w, tol in (('loss', loss, w_loss, loss_tol), ('grad', grad, w_grad, grad_tol)):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, 'NaN positions')
        with np.errstate(invalid='ignore'):
            bad = np.abs(g - w) > tol
        bad &= np.isfinite(w)
        assert not bad.any(), (what, name, np.argwhere(bad)[:5], g[bad][:5], w[bad][:5], tol[bad][:5])


# ------------------------------------------------------------------------------------------ a numpy evaluator
class NumpyEvaluator(object):
    """``lossgrad(W, leave)`` and ``score(W, leave)`` over a host table in vectorised numpy float64: what drives
    ``fitting.classifier`` in the CPU tests, and the checker of its gradients."""

    def __init__(self, z, y, fold=None):
        self.z = np.asarray(z, dtype=np.float32).astype(np.float64)
        self.za = np.concatenate([self.z, np.ones((len(self.z), 1))], axis=1)
        self.y = np.asarray(y)
        self.fold = fold
        self.calls = 0

    def lossgrad(self, W, leave):
        self.calls += 1
        M, S = W.shape[:2]
        inc = includes(self.y, self.fold, leave, S)
        l = np.einsum('nd,msd->nms', self.za, W)
        top = l.max(axis=2, keepdims=True)
        e = np.exp(l - top)
        total = e.sum(axis=2, keepdims=True)
        yy = np.clip(self.y, 0, S - 1)
        t = (top[..., 0] - np.take_along_axis(l, yy[:, None, None].repeat(M, 1), axis=2)[..., 0]) + np.log(total[..., 0])
        r = e / total
        r[np.arange(len(yy)), :, yy] -= 1.0
        r *= inc[:, :, None]
        return (t * inc).sum(axis=0), np.einsum('nms,nd->msd', r, self.za), inc.sum(axis=0).astype(np.float64)

    def score(self, W, leave):
        S = W.shape[1]
        sc = scored(self.y, self.fold, leave, S)
        pred = np.argmax(np.einsum('nd,msd->nms', self.za, W), axis=2)
        return np.stack([((pred == self.y[:, None]) & sc).sum(axis=0), sc.sum(axis=0)], axis=1).astype(np.float64)


def objective_ref(z, y, W, C):
    """``(F, dF)`` of ONE model ``W (S, D + 1)`` on all rows, written out here in numpy float64 on its own -- nothing
    of the package enters: ``F = (1 / n) sum_rows [logsumexp(l) - l_y] + ||W[:, :D]||^2 / (2 C n)``, the objective
    sklearn's ``LogisticRegression(C)`` minimises (intercepts, column D, unpenalised), and its gradient."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    y = np.asarray(y)
    n, D = z64.shape
    l = z64 @ W[:, :D].T + W[:, D]
    top = l.max(axis=1)
    e = np.exp(l - top[:, None])
    total = e.sum(axis=1)
    F = np.sum(top + np.log(total) - l[np.arange(n), y]) / n + np.sum(W[:, :D] ** 2) / (2.0 * C * n)
    r = e / total[:, None]
    r[np.arange(n), y] -= 1.0
    dF = np.empty_like(W)
    dF[:, :D] = r.T @ z64 / n + W[:, :D] / (C * n)
    dF[:, D] = r.sum(axis=0) / n
    return F, dF


# ------------------------------------------------------------------------------------------ the whole procedure
GAP = 1e-6          # rows whose two largest decision values under the oracle's model are closer than this are not compared
CAP = 0.001         # ... and they are at most this fraction of the rows


def whole_procedure_on_numpy(z, y, Cs=None, tol=1e-8, max_iter=1000):
    """``fitting.classifier.cross_validate`` on the numpy evaluator over the table ``z`` with classes ``y``: the
    oracle of the GPU tests, itself held to sklearn in tests/test_classifier_cpu.py."""
    from behavenet_amd.fitting import classifier as clf
    folds = clf.stratified_folds(y, 5)
    ev = NumpyEvaluator(z, y, folds)
    S = int(np.max(y)) + 1
    return clf.cross_validate(ev.lossgrad, ev.score, np.bincount(folds, minlength=5), S, z.shape[1],
                              clf.DEFAULT_CS if Cs is None else Cs, tol, max_iter)


# ------------------------------------------------------------------------------------------ inputs
def gaussian_classes(sizes, D, seed=0, spread=0.5, draw=None):
    """fp32 ``(n, D)`` rows of overlapping Gaussian classes and their int class ids, shuffled: class k has
    ``sizes[k]`` rows of unit deviation around a centre drawn with deviation ``spread``.  The centres depend on
    ``(seed, D, len(sizes))`` alone; ``draw`` names another sample of rows around the SAME centres (a held-out table
    of the same classes).  The default spread puts the centres about ``sqrt(2 D) / 2`` deviations apart: classes that
    overlap, as sessions do in latents that were trained to hide them.  (Nearly separable classes at C = 100 make F so
    flat that a gradient of 1e-8, where the optimiser must stop, no longer pins F to a few ulp:
    ``F - F* <= |dF|^2 / (2 lambda_min)``.)"""
    rng = np.random.default_rng([seed, D, len(sizes)])
    centres = spread * rng.standard_normal((len(sizes), D))
    if draw is not None:
        rng = np.random.default_rng([seed, D, len(sizes), 1 + draw])
    z = np.concatenate([centres[k] + rng.standard_normal((s, D)) for k, s in enumerate(sizes)])
    y = np.concatenate([np.full(s, k) for k, s in enumerate(sizes)])
    order = rng.permutation(len(y))
    return z[order].astype(np.float32), y[order].astype(np.int64)


def kernel_case(n, D, S, M, seed=0, scale=1.0):
    """Operands of a kernel test: rows, classes (every one present when n allows), folds 0..4, weights of deviation
    ``scale / sqrt(D)`` and the fold each model leaves out: -1 for the first, then 0..4 in turn."""
    rng = np.random.default_rng([seed, n, D, S, M])
    z = rng.standard_normal((n, D)).astype(np.float32)
    y = rng.integers(0, S, n).astype(np.int32)
    fold = rng.integers(0, 5, n).astype(np.int32)
    W = scale * rng.standard_normal((M, S, D + 1)) / np.sqrt(D)
    leave = ((np.arange(M) % 6) - 1).astype(np.int32)
    return z, y, fold, W, leave
