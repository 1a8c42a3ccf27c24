"""The session classifier's host side against sklearn, without a GPU ("session classifier"):
the folds, the lockstep L-BFGS on a numpy float64 evaluator, the whole cross-validated procedure against
``LogisticRegressionCV``, ``fit_classifier``'s file and messages, and the library's checks that come before a launch."""

import os
import types
import warnings

import numpy as np
import pytest

from behavenet_amd import _hip
from behavenet_amd.fitting import classifier as clf
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.fitting import training
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import classifier_refs as refs

U = 2.0 ** -53
GAP, CAP = refs.GAP, refs.CAP
whole_procedure_on_numpy = refs.whole_procedure_on_numpy


def _sklearn(cls, **kwargs):
    """sklearn's model as the reference calls it; a version that has dropped ``multi_class`` fits the multinomial
    model for three classes and more without it."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            return cls(multi_class='multinomial', **kwargs)
        except TypeError:
            return cls(**kwargs)


def _fit(model, z, y):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return model.fit(z, y)


# ------------------------------------------------------------------------------------------ folds
@pytest.mark.parametrize('sizes', [(500, 400, 300), (5, 23, 7), (17, 5), (6, 6, 6, 9, 31, 5, 12, 8)])
def test_stratified_folds_are_sklearns(sizes):
    rng = np.random.default_rng(len(sizes))
    StratifiedKFold = pytest.importorskip('sklearn.model_selection').StratifiedKFold
    y = rng.permutation(np.concatenate([np.full(s, 3 * k + 1) for k, s in enumerate(sizes)]))
    folds = clf.stratified_folds(y, 5)
    assert folds.dtype == np.int32 and folds.shape == y.shape
    want = np.empty(len(y), dtype=np.int32)
    for i, (_, test) in enumerate(StratifiedKFold(5).split(np.zeros((len(y), 1)), y)):
        want[test] = i
    assert np.array_equal(folds, want)
    if sizes == (500, 400, 300):
        assert [np.bincount(folds[y == c]).tolist() for c in (1, 4, 7)] == [[100] * 5, [80] * 5, [60] * 5]


def test_a_class_smaller_than_the_folds_is_refused():
    y = np.array([0] * 9 + [1] * 4)
    with pytest.raises(ValueError, match='class 1 has 4 rows'):
        clf.stratified_folds(y, 5)
    assert clf.stratified_folds(np.array([0] * 9 + [1] * 5), 5).shape == (14,)


# ------------------------------------------------------------------------------------------ the optimiser
CS3 = (1e-5, 0.1, 100)


@pytest.mark.parametrize('S', [2, 3])
def test_lockstep_reaches_sklearns_optimum(S):
    """tol = 1e-8 at C = 1e-5, 0.1 and 100 together: the numpy float64 gradient at the returned weights is within tol,
    and F is no larger than at sklearn's ``LogisticRegression(tol=1e-10, max_iter=10000)`` solution by more than
    ``64 2^-53 |F|``.  The classes overlap (``classifier_refs.gaussian_classes``, centres half a deviation a column
    apart).  With centres a whole deviation apart two classes are nearly separable (F = 0.027 at C = 100) and F is so
    flat there that the prescribed stop, a gradient of 1e-8, left F 8.4e-16 above sklearn's against a bound of 1.9e-16;
    the other five cases passed on those rows as well."""
    LogisticRegression = pytest.importorskip('sklearn.linear_model').LogisticRegression
    sizes = (500, 400, 300)[:S]
    z, y = refs.gaussian_classes(sizes, 5, seed=11)
    ev = refs.NumpyEvaluator(z, y)
    none = np.full(len(CS3), -1)
    W, n_iter, converged = clf.fit_softmax_lockstep(lambda w: ev.lossgrad(w, none), len(CS3), S, 5, CS3,
                                                    [len(y)] * len(CS3), tol=1e-8, max_iter=1000)
    assert converged.all() and (n_iter > 0).all() and W.shape == (len(CS3), S, 6)
    for m, C in enumerate(CS3):
        F, dF = refs.objective_ref(z, y, W[m], C)
        assert np.abs(dF).max() <= 1e-8, (S, C, np.abs(dF).max())
        try:
            sk = _fit(_sklearn(LogisticRegression, C=C, tol=1e-10, max_iter=10000), z.astype(np.float64), y)
            coef, icpt = sk.coef_, sk.intercept_
            if S == 2:
                assert coef.shape == (1, 5)          # (the two-row softmax model, reported as its row of class 1)
                coef, icpt = np.concatenate([-coef, coef]), np.concatenate([-icpt, icpt])
        except (TypeError, ValueError):
            assert S == 2          # a later sklearn without the keyword: the binomial model at 2 C is the same optimum
            sk = _fit(LogisticRegression(C=2 * C, tol=1e-10, max_iter=10000), z.astype(np.float64), y)
            coef, icpt = np.concatenate([-sk.coef_, sk.coef_]) / 2, np.concatenate([-sk.intercept_, sk.intercept_]) / 2
        F_sk, _ = refs.objective_ref(z, y, np.concatenate([coef, icpt[:, None]], axis=1), C)
        print('S %d C %g: F %.17g, sklearn %.17g, |dF| %.3g, %d iterations' % (S, C, F, F_sk, np.abs(dF).max(), n_iter[m]))
        assert F <= F_sk + 64 * U * abs(F_sk), (S, C, F, F_sk)
        # the classifier object reports what sklearn reports
        got = clf.SessionClassifier(W[m], sk.classes_, C, CS3, np.zeros((5, 3)), n_iter[m])
        assert got.coef_.shape == sk.coef_.shape and got.intercept_.shape == sk.intercept_.shape
        assert np.array_equal(got.predict(z[:50].astype(np.float64)), sk.predict(z[:50].astype(np.float64)))
        assert np.allclose(got.predict_proba(z[:50]), sk.predict_proba(z[:50].astype(np.float64)), rtol=0, atol=1e-5)


def test_a_frozen_model_keeps_its_bits_and_max_iter_only_warns():
    z, y = refs.gaussian_classes((300, 200, 250), 4, seed=5)
    ev = refs.NumpyEvaluator(z, y)
    none = np.full(2, -1)
    seen = []

    def evaluate(W):
        seen.append(W.copy())
        return ev.lossgrad(W, none)
    # C = 0.1 takes fewer steps than C = 1e-5, whose penalised weights and free intercepts are scaled far apart
    Cs = [0.1, 1e-5]
    W, n_iter, converged = clf.fit_softmax_lockstep(evaluate, 2, 3, 4, Cs, [len(y)] * 2, tol=1e-8, max_iter=1000)
    assert converged.all() and n_iter[0] + 3 <= n_iter[1], n_iter
    frozen = [k for k, w in enumerate(seen) if np.array_equal(w[0], W[0])]
    assert len(frozen) >= 3 and frozen == list(range(frozen[0], len(seen)))          # from its last step to the end
    assert all(np.array_equal(seen[k][0].view(np.int64), W[0].view(np.int64)) for k in frozen)
    assert not np.array_equal(seen[frozen[0]][1], W[1])          # ... while the other one went on
    with pytest.warns(UserWarning, match='1 of 2 models did not reach'):
        W2, n_iter2, converged2 = clf.fit_softmax_lockstep(evaluate, 2, 3, 4, Cs, [len(y)] * 2, tol=1e-8,
                                                           max_iter=n_iter[0])
    assert converged2.tolist() == [True, False] and n_iter2.tolist() == [n_iter[0]] * 2
    assert np.array_equal(W2[0], W[0])
    # a start at the optimum: no step is taken
    W3, n_iter3, converged3 = clf.fit_softmax_lockstep(evaluate, 2, 3, 4, Cs, [len(y)] * 2, tol=1e-8, W0=W)
    assert converged3.all() and not n_iter3.any() and np.array_equal(W3, W)
    with pytest.raises(ValueError, match='counted'):
        clf.fit_softmax_lockstep(evaluate, 2, 3, 4, Cs, [len(y) - 1] * 2)


# ------------------------------------------------------------------------------------------ the whole procedure
def compare_with_sklearn(got, z, y, z_held, what=''):
    """``scores_`` entry for entry, ``C_`` and the predictions on ``z_held`` against ``LogisticRegressionCV`` as the
    reference calls it at ``tol=1e-10, max_iter=10000``; rows within GAP of a tie under sklearn's model are left out
    and counted -> (sklearn's model, rows left out of the held table, rows left out of the folds)."""
    LogisticRegressionCV = pytest.importorskip('sklearn.linear_model').LogisticRegressionCV
    sk = _fit(_sklearn(LogisticRegressionCV, Cs=list(got.Cs_), cv=5, penalty='l2', tol=1e-10, max_iter=10000),
              z.astype(np.float64), y)
    assert got.C_ == sk.C_[0], (what, got.C_, sk.C_)
    d = sk.decision_function(z_held.astype(np.float64))
    gap = 2 * np.abs(d) if d.ndim == 1 else np.diff(np.sort(d, axis=1)[:, -2:], axis=1)[:, 0]
    near = gap < GAP
    assert near.sum() <= CAP * len(z_held), (what, int(near.sum()))
    assert np.array_equal(got.predict(z_held.astype(np.float64))[~near], sk.predict(z_held.astype(np.float64))[~near]), what
    sk_scores = sk.scores_[sk.classes_[-1]]
    assert sk_scores.shape == got.scores_.shape == (5, len(got.Cs_))
    # a fold's score moves by 1 / rows for every held-out row whose prediction differs: none may, outside the near ties
    folds = clf.stratified_folds(y, 5)
    counts = np.bincount(folds, minlength=5)
    off = np.rint(np.abs(got.scores_ - sk_scores) * counts[:, None])
    print(what, 'min gap %.3g, near ties %d, score differences in rows:' % (gap.min(), near.sum()), off.sum())
    return sk, int(near.sum()), off


@pytest.mark.parametrize('sizes', [(500, 400, 300), (450, 350)])
def test_whole_procedure_is_logistic_regression_cv(sizes):
    """1200 x 5 (800 x 5 for two classes) overlapping Gaussian classes: ``scores_`` equal entry for entry, ``C_``
    equal, predictions on a held-out table equal; the seeds leave no row of the held-out table within 1e-6 of a tie
    (smallest gap seen: printed)."""
    z, y = refs.gaussian_classes(sizes, 5, seed=21)
    z_held, _ = refs.gaussian_classes(tuple(s // 2 for s in sizes), 5, seed=21, draw=0)          # the same classes
    got = whole_procedure_on_numpy(z, y)
    sk, near, off = compare_with_sklearn(got, z, y, z_held, sizes)
    assert near == 0 and not off.any(), (near, off)
    assert np.allclose(got.coef_, sk.coef_, rtol=0, atol=1e-5) and np.allclose(got.intercept_, sk.intercept_, rtol=0, atol=1e-5)
    assert abs(got.weights_[:, -1].sum()) < 1e-12
    assert got.n_iter_.shape == (5, 8) and got.converged_


# ------------------------------------------------------------------------------------------ fit_classifier
def _stub(root, model_class='msps-vae'):
    os.makedirs(os.path.join(root, 'version_2'), exist_ok=True)
    return types.SimpleNamespace(hparams={'model_class': model_class, 'expt_dir': root, 'n_labels': 2}, version=2)


def test_fit_classifier_file_messages_and_overwrite(tmp_path, capsys, monkeypatch):
    calls = []

    def fake(data_generator, model, dtype='val', columns=None, **kwargs):
        calls.append((dtype, columns))
        return 0.25 * len(calls), 'classifier %d' % len(calls)
    monkeypatch.setattr(bn_eval, 'session_classifier', fake)
    model = _stub(str(tmp_path))
    path = os.path.join(str(tmp_path), 'version_2', 'fc_session_classification.npy')
    fc, lr = cau.fit_classifier(model, 'gen', dtype='test')
    out = capsys.readouterr().out
    assert (fc, lr) == (0.25, 'classifier 1') and calls == [('test', None)]
    for line in ('FC metrics do not exist; computing from scratch', 'collecting training labels and latents',
                 'collecting test labels and latents', 'fitting linear classifier model with training data',
                 'computing fraction correct on test data', 'done', 'saving results to %s' % path):
        assert line in out, line
    saved = np.load(path)
    assert saved.shape == (1,) and saved.dtype == np.float64 and saved[0] == 0.25
    fc, lr = cau.fit_classifier(model, None)          # read back: neither model weights nor generator are needed
    assert (fc, lr) == (0.25, None) and len(calls) == 1
    assert capsys.readouterr().out == 'loading results from %s\n' % path
    fc, lr = cau.fit_classifier(model, 'gen', overwrite=True, fit_full=True)
    assert (fc, lr) == (0.5, 'classifier 2') and calls[-1] == ('val', None)          # msps-vae: fit_full is ignored
    assert 'overwriting metrics at %s' % path in capsys.readouterr().out and np.load(path)[0] == 0.5
    ps = _stub(str(tmp_path / 'ps'), 'ps-vae')
    cau.fit_classifier(ps, 'gen', fit_full=True)
    cau.fit_classifier(ps, 'gen', overwrite=True)
    assert calls[-2:] == [('val', slice(None)), ('val', None)]
    for model_class in ('cond-ae', 'cond-ae-msp', 'beta-tcvae'):
        with pytest.raises(NotImplementedError):
            cau.fit_classifier(_stub(str(tmp_path), model_class), 'gen')
    assert 'fit_classifier' in cau.__all__ and 'session_classifier' in bn_eval.__all__


def test_one_session_is_refused_before_the_walk_and_before_the_first_epoch():
    gen = types.SimpleNamespace(datasets=[object()])
    model = types.SimpleNamespace(hparams={'model_class': 'ae', 'n_ae_latents': 8})
    with pytest.raises(ValueError, match='session_classifier: 1 session'):
        bn_eval.session_classifier(gen, model)
    two = types.SimpleNamespace(datasets=[object(), object()])
    with pytest.raises(ValueError, match='session_classifier: 1 session'):
        bn_eval.session_classifier(two, model, sess_idx=[1])
    with pytest.raises(ValueError, match='session_classifier: 9 sessions'):
        bn_eval.session_classifier(types.SimpleNamespace(datasets=[object()] * 9), model)
    with pytest.raises(ValueError, match='session_classifier: 9 folds x 8'):
        bn_eval.session_classifier(two, model, n_splits=9)
    with pytest.raises(ValueError, match="export_session_classifier.*1 session"):
        training._fit({'export_session_classifier': True}, model, gen, None, method='ae')


# ------------------------------------------------------------------------------------------ the library's side
def test_plan_and_workspace_queries_agree():
    lib = _hip.load()
    for n, D, S, M in ((1, 1, 2, 1), (127, 64, 8, 64), (128, 3, 3, 5), (129, 16, 4, 40), (421, 17, 3, 40),
                       (10 ** 6, 16, 4, 40), (10 ** 6, 64, 4, 40), (10 ** 6, 64, 8, 64), (2 ** 31 - 1, 64, 2, 1)):
        for score in (False, True):
            blocks, rows, mg = _hip._softmax_cv_plan(n, D, S, M, score)
            assert (blocks - 1) * rows < n <= blocks * rows and 1 <= mg <= M and mg * S <= 128
            pm = 2 if score else S * (D + 1) + 2
            query = lib.bn_softmax_cv_score_ws_bytes if score else lib.bn_softmax_cv_lossgrad_ws_bytes
            assert query(n, D, S, M) == blocks * M * pm * 8 <= 32 << 20, (n, D, S, M, score)
    assert _hip._softmax_cv_plan(421, 17, 3, 40) == (4, 106, 40) and _hip._softmax_cv_plan(10 ** 6, 64, 4, 40) == (400, 2500, 32)
    assert lib.bn_softmax_cv_lossgrad_ws_bytes(0, 3, 3, 5) == 16 == lib.bn_softmax_cv_score_ws_bytes(0, 3, 3, 5)
    for n, D, S, M in ((-1, 3, 3, 5), (10, 0, 3, 5), (10, 65, 3, 5), (10, 3, 1, 5), (10, 3, 9, 5), (10, 3, 3, 0),
                       (10, 3, 3, 65)):
        assert lib.bn_softmax_cv_lossgrad_ws_bytes(n, D, S, M) == 0 == lib.bn_softmax_cv_score_ws_bytes(n, D, S, M)


def test_host_side_refusals_of_the_c_entry_points():
    """The checks that come before any launch run without a GPU: nothing is dereferenced."""
    lib = _hip.load()
    z, y, fold, W, leave, out, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    need = lib.bn_softmax_cv_lossgrad_ws_bytes(10, 3, 3, 5)
    E_ARG, E_SHAPE = -1, -2

    def lossgrad(z=z, ld=3, y=y, fold=fold, W=W, leave=leave, n=10, D=3, S=3, M=5, loss=out, grad=out + 64,
                 count=out + 1024, ws=ws, nbytes=need):
        return lib.bn_softmax_cv_lossgrad(z, ld, y, fold, W, leave, n, D, S, M, loss, grad, count, ws, nbytes, None)

    def score(z=z, ld=3, y=y, fold=fold, W=W, leave=leave, n=10, D=3, S=3, M=5, out=out, ws=ws, nbytes=need):
        return lib.bn_softmax_cv_score(z, ld, y, fold, W, leave, n, D, S, M, out, ws, nbytes, None)
    for call in (lossgrad, score):
        for bad in ({'D': 0}, {'D': 65, 'ld': 65}, {'ld': 2}, {'S': 1}, {'S': 9}, {'M': 0}, {'M': 65}, {'n': -1},
                    {'z': z + 2}, {'y': y + 1}, {'fold': fold + 2}, {'leave': leave + 3}, {'W': W + 4},
                    {'ws': ws + 8}, {'nbytes': 7}):
            assert call(**bad) == E_SHAPE, (call.__name__, bad)
        for bad in ({'z': None}, {'y': None}, {'W': None}, {'leave': None}, {'ws': None}):
            assert call(**bad) == E_ARG, (call.__name__, bad)
    assert lossgrad(loss=None) == E_ARG and lossgrad(grad=None) == E_ARG and lossgrad(count=None) == E_ARG
    assert lossgrad(loss=out + 4) == E_SHAPE and lossgrad(nbytes=need - 1) == E_SHAPE
    assert score(out=None) == E_ARG and score(out=out + 4) == E_SHAPE


def test_wrappers_check_their_operands_before_a_launch():
    import torch
    z = torch.zeros((10, 3))
    y = torch.zeros(10, dtype=torch.int32)
    W = torch.zeros((5, 3, 4), dtype=torch.float64)
    leave = torch.zeros(5, dtype=torch.int32)
    for fn in (_hip.softmax_cv_lossgrad, _hip.softmax_cv_score):
        with pytest.raises(ValueError, match='no CPU fallback'):
            fn(z, y, None, W, leave)
        with pytest.raises(TypeError, match='must be float32'):
            fn(z.double(), y, None, W, leave)
        with pytest.raises(TypeError, match='expected a device table'):
            fn(z.numpy(), y, None, W, leave)
