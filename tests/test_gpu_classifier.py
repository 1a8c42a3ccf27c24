"""The session classifier on the device ("session classifier").

1. ``bn_softmax_cv_lossgrad`` and ``bn_softmax_cv_score`` by direct C calls on operands between guard bands, the
   outputs pre-filled with a sentinel and the workspace guarded and NaN-filled, against
   ``tests/classifier_refs`` (numpy float64 with ``math.fsum``) within the tolerance derived in that file: counts
   exact, the same NaN positions, the same bits on a second call.
2. The wrappers ``_hip.softmax_cv_lossgrad`` and ``_hip.softmax_cv_score``.
3. ``fitting.eval.classify_table`` on Gaussian tables against the numpy procedure of ``tests/classifier_refs.py``
   (held to sklearn in ``tests/test_classifier_cpu.py``).
4. Whole models (the small golden MSPS-VAE and AE) with two and three synthetic sessions: ``session_classifier``
   against that procedure run on ``encode_trial``'s latents, ``fit_classifier``'s file and the ``fit`` key.
"""

import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting import classifier as clf
from behavenet_amd.fitting.eval import classify_table, encode_trial, export_latents, score_table, session_classifier
from behavenet_amd.plotting.cond_ae_utils import fit_classifier
from tests import classifier_refs as refs
from tests.classifier_refs import CAP, GAP, whole_procedure_on_numpy
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_latent_corr import _doubles, _place
from tests.test_gpu_ranges import LENS, _model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2
SENTINEL = -77.0


# ------------------------------------------------------------------------------------------ 1: the kernels
def _int32(values):
    values = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.int32)
    t = guarded(torch.zeros(max(values.numel(), 1))).view(torch.int32)
    t[:values.numel()].copy_(values)          # (no values: one element that is never read, an empty tensor has no address)
    return t


def _workspace(n, D, S, M, score):
    lib = _hip.load()
    nbytes = (lib.bn_softmax_cv_score_ws_bytes if score else lib.bn_softmax_cv_lossgrad_ws_bytes)(n, D, S, M)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _call(score, z, ld, y, fold, W, leave, n, D, S, M, outs, ws, nbytes):
    lib = _hip.load()
    fn = lib.bn_softmax_cv_score if score else lib.bn_softmax_cv_lossgrad
    return fn(_ptr(z), ld, _ptr(y), _ptr(fold), _ptr(W), _ptr(leave), n, D, S, M, *[_ptr(o) for o in outs], _ptr(ws),
              nbytes, torch.cuda.current_stream().cuda_stream)


def _run(score, z, y, fold, W, leave, ld=None, offset=0, what=''):
    """One guarded call and a second one on the used workspace -> the outputs (numpy); the inputs keep their bits."""
    n, D = z.shape
    M, S = W.shape[:2]
    ld = D if ld is None else ld
    z_d, whole = _place(z, ld, offset) if n else (_place(np.zeros((1, D), dtype=np.float32), ld, offset))
    ints = [_int32(y), None if fold is None else _int32(fold), _int32(leave)]
    W_d = _doubles(W.shape, 0.0)
    W_d.copy_(torch.from_numpy(W))
    before = [whole.view(torch.int32).clone(), W_d.view(torch.int64).clone()]
    before += [None if t is None else t.clone() for t in ints]
    ws, nbytes = _workspace(n, D, S, M, score)
    shapes = [(M, 2)] if score else [(M,), (M, S, D + 1), (M,)]
    outs = [_doubles(s, SENTINEL) for s in shapes]
    args = (score, z_d, ld, ints[0], ints[1], W_d, ints[2], n, D, S, M, outs, ws, nbytes)
    assert _call(*args) == 0, what
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(SENTINEL)
    assert _call(*args) == 0, what
    for o, f in zip(outs, first):
        assert torch.equal(o.view(torch.int64), f.view(torch.int64)), (what, 'a second call gave other bits')
    after = [whole.view(torch.int32), W_d.view(torch.int64)] + ints
    for a, b in zip(after, before):
        assert b is None or torch.equal(a, b), (what, 'an input was written')
    got = [f.cpu().numpy() for f in first]
    return got[0] if score else got


def _check(case, variants=((None, 0),), with_fold=True, seed=0, scale=1.0):
    n, D, S, M = case
    z, y, fold, W, leave = refs.kernel_case(n, D, S, M, seed, scale)
    fold = fold if with_fold else None
    want = refs.lossgrad_ref(z, y, fold, W, leave)
    want_score, near = refs.score_ref(z, y, fold, W, leave)
    assert not near.any(), (case, 'the case has near ties')
    for ld, offset in variants:
        what = (case, ld, offset, with_fold)
        refs.assert_lossgrad_close(_run(False, z, y, fold, W, leave, ld, offset, what), want, what)
        got = _run(True, z, y, fold, W, leave, ld, offset, what)
        assert got.dtype == np.float64 and np.array_equal(got, want_score), (what, got, want_score)
    return want, want_score


# 421 rows: ceil(421 / 128) = 4 row blocks of ceil(421 / 4) = 106 rows, the last one of 103; a chunk is 32 rows
SPAN = 421
CASES = [(0, 3, 3, 5), (1, 1, 2, 1), (31, 17, 3, 5), (SPAN, 16, 2, 40), (SPAN, 3, 3, 40), (161, 64, 8, 64),
         (130, 64, 3, 64), (SPAN, 17, 8, 5), (33, 1, 8, 64), (SPAN, 16, 4, 1)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d-D%d-S%d-M%d' % c)
def test_kernels_against_the_reference(case):
    """n in {0, 1, a chunk less one row, three row blocks and a ragged fourth}, D in {1, 3, 16, 17, 64}, S in
    {2, 3, 8}, M in {1, 5, 40, 64} -- one, two (42 + 22 models of three classes) and four model groups --; leading
    dimension D on a 16-byte boundary and D + 5 four bytes off one; every sixth model includes every row."""
    n, D, S, M = case
    assert _hip._softmax_cv_plan(SPAN, D, S, M)[:2] == (4, 106) and _hip._softmax_cv_plan(161, D, S, M)[:2] == (2, 81)
    assert _hip.SOFTMAX_CV_CHUNK_ROWS == 32
    want, want_score = _check(case, ((None, 0), (D + 5, 1)))
    if n >= 31:
        assert want[2].min() > 0 and (want[2][::6] == n).all() and (want_score[::6, 1] == n).all()
    else:
        assert n == 0 or M == 1
        assert n or (not want[0].any() and not want[1].any() and not want[2].any() and not want_score.any())


def test_no_fold_array_and_a_model_that_excludes_every_row():
    want, want_score = _check((SPAN, 16, 3, 5), ((21, 1),), with_fold=False)
    # no row belongs to a fold: every model includes every row; only the model that leaves no fold out scores any
    assert (want[2] == SPAN).all() and want_score[:, 1].tolist() == [SPAN, 0, 0, 0, 0]
    z, y, fold, W, leave = refs.kernel_case(SPAN, 16, 3, 5, seed=1)
    fold[:] = 2
    assert leave.tolist() == [-1, 0, 1, 2, 3]
    got = _run(False, z, y, fold, W, leave)
    refs.assert_lossgrad_close(got, refs.lossgrad_ref(z, y, fold, W, leave), 'one fold')
    assert got[2].tolist() == [SPAN, SPAN, SPAN, 0, SPAN] and got[0][3] == 0 and not got[1][3].any()
    assert _run(True, z, y, fold, W, leave)[:, 1].tolist() == [SPAN, 0, 0, SPAN, 0]


def test_logits_of_800_stay_finite():
    """Weights that put the logits at +-800: exp alone would overflow and underflow; with the row maximum subtracted
    every sum is finite and within the tolerance (which grows with the logits, as the rounding of the dot product
    does)."""
    z, y, fold, W, leave = refs.kernel_case(SPAN, 3, 3, 5, seed=2)
    W[:, 1] = -W[:, 0]             # class 1 mirrors class 0: the row that reaches 800 reaches -800 as well
    W *= (800.0 / np.abs(refs.logits_ref(z, W)[0][:, :, :2]).max(axis=(0, 2)))[:, None, None]
    logit = refs.logits_ref(z, W)[0]
    assert (logit.max(axis=(0, 2)) > 799).all() and (logit.min(axis=(0, 2)) < -799).all()
    want = refs.lossgrad_ref(z, y, fold, W, leave)
    got = _run(False, z, y, fold, W, leave)
    assert all(np.isfinite(g).all() for g in got) and got[0].min() > 100
    refs.assert_lossgrad_close(got, want, '800')
    want_score, near = refs.score_ref(z, y, fold, W, leave)
    assert not near.any() and np.array_equal(_run(True, z, y, fold, W, leave), want_score)


def test_a_nan_row_reaches_the_models_that_include_it_and_a_class_out_of_range_none():
    z, y, fold, W, leave = refs.kernel_case(SPAN, 17, 3, 40, seed=3)
    row = 250
    z[row, 5] = np.nan
    fold[row] = 1
    y[[7, 300]] = [3, -1]          # classes outside [0, 3): rows of no model
    z[7] = 1e30                    # ... whatever they hold
    want = refs.lossgrad_ref(z, y, fold, W, leave)
    got = _run(False, z, y, fold, W, leave, 22, 1)
    refs.assert_lossgrad_close(got, want, 'nan')
    hit = leave != 1               # the models that do not leave fold 1 out include the row
    assert hit.sum() == 33 and np.array_equal(np.isnan(got[0]), hit)
    assert np.array_equal(np.isnan(got[1]), np.broadcast_to(hit[:, None, None], got[1].shape))
    assert np.isfinite(got[2]).all() and got[2].max() == SPAN - 2
    # the score reads the row as class 0, as np.argmax of a row of NaNs does
    want_score, near = refs.score_ref(z, y, fold, W, leave)
    assert not near.any() and np.array_equal(_run(True, z, y, fold, W, leave, 22, 1), want_score)
    assert want_score[0, 1] == SPAN - 2


def test_exact_ties_go_to_the_lowest_class():
    z, y, fold, W, leave = refs.kernel_case(SPAN, 16, 4, 5, seed=4)
    W[:] = 0.0                     # model 0: every logit zero, class 0 wins every row
    W[1, 1] = W[1, 3] = refs.kernel_case(SPAN, 16, 4, 5, seed=5)[3][1, 1]          # model 1: classes 1 and 3 tie
    W[1, 0] = W[1, 2] = -5.0 * np.abs(W[1, 1])
    W[2] = refs.kernel_case(SPAN, 16, 4, 5, seed=6)[3][2]
    W[2, 3] = W[2, 2]              # model 2: class 3 repeats class 2
    leave[:] = -1
    want_score, near = refs.score_ref(z, y, fold, W, leave)
    assert not near.any()
    got = _run(True, z, y, fold, W, leave)
    assert np.array_equal(got, want_score)
    assert got[0, 0] == (y == 0).sum() and got[1, 0] < (np.isin(y, (1, 3))).sum()
    logit = refs.logits_ref(z, W)[0]
    assert (np.argmax(logit[:, 1], axis=1) != 3).all() and (np.argmax(logit[:, 2], axis=1) != 3).all()
    refs.assert_lossgrad_close(_run(False, z, y, fold, W, leave), refs.lossgrad_ref(z, y, fold, W, leave), 'ties')


def test_refusals_write_nothing():
    z, y, fold, W, leave = refs.kernel_case(40, 3, 3, 5)
    n = 40
    p = _place(z, 8)[0]
    y_d, fold_d, leave_d = _int32(y), _int32(fold), _int32(leave)
    W_d = _doubles((64, 8, 65), 0.0)
    for score in (False, True):
        ws, nbytes = _workspace(n, 64, 8, 64, score)
        outs = [_doubles((64, 2), SENTINEL)] if score else [_doubles(s, SENTINEL) for s in ((64,), (64, 8, 65), (64,))]
        need = _workspace(n, 3, 3, 5, score)[1]

        def call(z=p, ld=8, y=y_d, fold=fold_d, W=W_d, leave=leave_d, n=n, D=3, S=3, M=5, outs=outs, ws=ws,
                 nbytes=nbytes):
            return _call(score, z, ld, y, fold, W, leave, n, D, S, M, outs, ws, nbytes)
        for bad in ({'D': 0}, {'D': 65, 'ld': 65}, {'S': 1}, {'S': 9}, {'M': 0}, {'M': 65}, {'n': -1}, {'ld': 2},
                    {'nbytes': need - 1}, {'z': p.data_ptr() + 2}, {'y': y_d.data_ptr() + 2},
                    {'W': W_d.data_ptr() + 4}, {'ws': ws.data_ptr() + 4}):
            assert call(**bad) == E_SHAPE, (score, bad)
        for bad in ({'z': None}, {'y': None}, {'W': None}, {'leave': None}, {'ws': None},
                    {'outs': [None] + outs[1:]}):
            assert call(**bad) == E_ARG, (score, bad)
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs) and bool(torch.isnan(ws).all())
        assert call() == 0
        torch.cuda.synchronize()
        assert not bool((outs[0].view(-1)[:5] == SENTINEL).any())


# ------------------------------------------------------------------------------------------ 2: the wrappers
def test_wrappers():
    z, y, fold, W, leave = refs.kernel_case(SPAN, 16, 3, 40, seed=8)
    want = refs.lossgrad_ref(z, y, fold, W, leave)
    want_score, _ = refs.score_ref(z, y, fold, W, leave)
    wide = np.random.default_rng(2).standard_normal((SPAN, 21)).astype(np.float32)
    wide[:, 3:19] = z
    wide_d = torch.from_numpy(wide).to(DEV)
    y_d, fold_d, leave_d = (torch.from_numpy(a).to(DEV) for a in (y, fold, leave))
    W_d = torch.from_numpy(W).to(DEV)
    got = _hip.softmax_cv_lossgrad(wide_d[:, 3:19], y_d, fold_d, W_d, leave_d)
    assert all(g.is_cuda and g.dtype == torch.float64 for g in got)
    assert [tuple(g.shape) for g in got] == [(40,), (40, 3, 17), (40,)]
    refs.assert_lossgrad_close([g.cpu().numpy() for g in got], want, 'wrapper')
    flat = _hip.softmax_cv_lossgrad(wide_d[:, 3:19], y_d, fold_d, W_d, leave_d, packed=True)
    assert flat.shape == (40 * (3 * 17 + 2),) and torch.equal(flat, torch.cat([got[0], got[2], got[1].reshape(-1)]))
    out = _hip.softmax_cv_score(wide_d[:, 3:19], y_d, fold_d, W_d, leave_d)
    assert out.is_cuda and out.dtype == torch.float64 and np.array_equal(out.cpu().numpy(), want_score)
    nofold = _hip.softmax_cv_lossgrad(wide_d[:, 3:19], y_d, None, W_d, leave_d)
    assert (nofold[2] == SPAN).all()
    empty = _hip.softmax_cv_lossgrad(wide_d[:0, 3:19], y_d[:0], None, W_d, leave_d)
    assert not empty[0].any() and not empty[1].any() and not empty[2].any()
    args = (wide_d[:, 3:19], y_d, fold_d, W_d, leave_d)
    for fn in (_hip.softmax_cv_lossgrad, _hip.softmax_cv_score):
        for k, bad, error, match in (
                (0, wide_d[:, 3:19].double(), TypeError, 'must be float32'),
                (0, wide_d[:, 3:19].t().contiguous().t(), ValueError, 'must be contiguous'),
                (0, wide_d[:, 3:19].cpu(), ValueError, 'no CPU fallback'),
                (0, torch.zeros((5, 65), device=DEV), ValueError, '1 to 64'),
                (1, y_d.long(), TypeError, 'y must be int32'),
                (1, y_d[:-1], ValueError, r'expected y \(421,\)'),
                (2, fold_d.cpu(), ValueError, 'no CPU fallback'),
                (3, W_d.float(), TypeError, 'must be float64'),
                (3, W_d[:, :, :16], ValueError, 'for 16 columns and an intercept'),
                (3, W_d[:, :1], ValueError, '1 classes'),
                (4, leave_d[:39], ValueError, r'expected leave \(40,\)')):
            with pytest.raises(error, match=match):
                fn(*(args[:k] + (bad,) + args[k + 1:]))


# ------------------------------------------------------------------------------------------ 3: the procedure
def _near(weights, z, rows=None):
    """Rows of ``z`` whose two largest logits under ``weights (S, D + 1)`` are within GAP of one another."""
    l = np.sort(z.astype(np.float64) @ weights[:, :-1].T + weights[:, -1], axis=1)
    near = (l[:, -1] - l[:, -2]) < GAP
    return near if rows is None else near & rows


def _same_procedure(got, want, z_train, y_train, what):
    """``scores_`` and ``C_`` of the device's procedure against the oracle's (the numpy procedure on the same rows):
    a score may differ by the held-out rows within GAP of a tie under the oracle's model, which are capped."""
    folds = clf.stratified_folds(y_train, 5)
    assert got.converged_ and want.converged_, what
    near = np.array([[_near(want.cv_weights_[i, j], z_train, folds == i).sum() for j in range(8)] for i in range(5)])
    print(what, 'near ties in the folds: %d; C_ %g; mean scores' % (near.sum(), want.C_), want.scores_.mean(axis=0))
    assert near.sum() <= CAP * len(y_train), (what, near)
    counts = np.bincount(folds, minlength=5)[:, None]
    assert (np.abs(got.scores_ - want.scores_) * counts <= near + 1e-9).all(), (what, got.scores_, want.scores_)
    assert got.C_ == want.C_ and got.scores_.shape == (5, 8), what


@pytest.mark.parametrize('sizes', [(500, 400, 300), (450, 350)])
def test_the_procedure_on_the_device_is_the_procedure_in_numpy(sizes):
    """1200 x 5 (800 x 5) overlapping Gaussian classes, tol = 1e-8: the 40 models fitted through
    ``bn_softmax_cv_lossgrad`` score their folds as the 40 fitted through the numpy evaluator do, ``C_`` is the same,
    the refitted model's numpy float64 gradient is within tol (plus the kernel's own rounding, 1e-11 at these sizes)
    and it predicts a held-out table as the oracle does.  Near ties under the oracle: none (printed)."""
    z, y = refs.gaussian_classes(sizes, 5, seed=21)
    z_held, y_held = refs.gaussian_classes(tuple(s // 2 for s in sizes), 5, seed=21, draw=0)          # the same classes
    want = whole_procedure_on_numpy(z, y)
    got = classify_table(torch.from_numpy(z).to(DEV), y, len(sizes), tol=1e-8, max_iter=1000)
    _same_procedure(got, want, z, y, sizes)
    F, dF = refs.objective_ref(z, y, got.weights_, got.C_)
    assert np.abs(dF).max() <= 1e-8 + 1e-11, np.abs(dF).max()
    near = _near(want.weights_, z_held)
    assert near.sum() <= CAP * len(y_held)
    assert np.array_equal(got.predict(z_held)[~near], want.predict(z_held)[~near])
    hits, rows = score_table(torch.from_numpy(z_held).to(DEV), y_held, got.weights_)
    assert rows == len(y_held) and abs(hits - (got.predict(z_held) == y_held).sum()) <= near.sum()


# ------------------------------------------------------------------------------------------ 4: whole models
GOLDENS = {'mspsvae_cfg1': (4, 8), 'ae_cfg1': (0, 8)}          # the default column block
GROW = 4          # frames a trial of session s has more than one of session s - 1: the sessions differ in size


def _generator(meta, n_sessions):
    """Sessions that differ in their frames (another seed, a fixed background mixed into every frame) and in size:
    trial t of session s has ``LENS[t] + 4 s`` frames."""
    sessions = []
    for s in range(n_sessions):
        lens = [n + GROW * s for n in LENS]
        sess = SyntheticSession(len(lens), lens, meta['dim'], seed=3 + s, n_labels=meta['n_labels'],
                                trial_splits='4;1;1;1', name=('lab', 'expt', 'animal', 'sess%d' % s))
        back = np.random.default_rng(100 + s).integers(0, 255, size=sess.images_u8[0].shape[1:])
        sess.images_u8 = [(0.75 * im + 0.25 * back).astype(np.uint8) for im in sess.images_u8]
        sessions.append(sess)
    return SyntheticSessionsGenerator(sessions, device=DEV, placement='device_u8')


def _tables(model, gen, split, lo, hi):
    """The per-trial route: ``encode_trial`` per trial in the reference's order -> (rows of the block, session ids)."""
    parts, ys = [], []
    for s, ds in enumerate(gen.datasets):
        for t in ds.batch_idxs[split]:
            z = encode_trial(model, torch.from_numpy(ds.images_u8[int(t)]).to(DEV), s)
            parts.append(np.asarray(z, dtype=np.float32)[:, lo:hi])
            ys.append(np.full(len(z), s))
    return np.concatenate(parts), np.concatenate(ys)


@pytest.mark.parametrize('n_sessions', [2, 3])
@pytest.mark.parametrize('golden', sorted(GOLDENS))
def test_session_classifier_is_the_cpu_procedure_on_the_per_trial_latents(golden, n_sessions, tmp_path):
    """Untrained models, sessions of 92, 108 and 124 train rows.  An untrained encoder hardly answers to its frames
    (the latents of two sessions differ by 1e-4 in the mean, whatever the frames' brightness, contrast or
    background), so with sessions of one size every held-out row lay within 1e-6 of a tie under the oracle alone
    (1116 of 276 x 8 at three sessions); sessions of different sizes give the intercepts something to decide, and the
    oracle's near ties are 0 in all four cases (smallest gap 0.12).  What the test holds to the oracle is therefore
    the walk, the table order, the columns, the classes and folds and the files; the numbers of a classifier that has
    something to find are held to it in the test above."""
    model, meta = _model(golden, str(tmp_path))
    lo, hi = GOLDENS[golden]
    gen = _generator(meta, n_sessions)
    z_train, y_train = _tables(model, gen, 'train', lo, hi)
    z_val, y_val = _tables(model, gen, 'val', lo, hi)
    assert np.bincount(y_train).tolist() == [92, 108, 124][:n_sessions]
    assert np.bincount(y_val).tolist() == [40, 44, 48][:n_sessions]
    want = whole_procedure_on_numpy(z_train, y_train, tol=1e-8, max_iter=1000)
    fc, got = session_classifier(gen, model, dtype='val', tol=1e-8, max_iter=1000)
    _same_procedure(got, want, z_train, y_train, (golden, n_sessions))
    near_val = _near(want.weights_, z_val)
    assert near_val.sum() <= CAP * len(y_val)
    want_fc = np.mean(want.predict(z_val) == y_val)
    assert abs(fc - want_fc) * len(y_val) <= near_val.sum() + 1e-9, (fc, want_fc)
    assert np.array_equal(got.classes_, np.arange(n_sessions)) and got.columns_ == (lo, hi)
    assert got.coef_.shape == ((1, hi - lo) if n_sessions == 2 else (n_sessions, hi - lo))
    F, dF = refs.objective_ref(z_train, y_train, got.weights_, got.C_)
    assert np.abs(dF).max() <= 1e-8 + 1e-11, np.abs(dF).max()          # (on the per-trial route's rows: the same table)
    if golden == 'ae_cfg1' and n_sessions == 3:
        # two of three sessions, every column, the train split
        fc_all, every = session_classifier(gen, model, dtype='train', columns=slice(None), sess_idx=[0, 2], tol=1e-6)
        assert every.coef_.shape == (1, 8) and every.classes_.tolist() == [0, 2] and 0.0 <= fc_all <= 1.0
        rows = np.isin(y_train, (0, 2))
        assert fc_all == np.mean(every.predict(z_train[rows]) == y_train[rows])
        again = session_classifier(gen, model, dtype='train', columns=slice(None), sess_idx=[0, 2], tol=1e-6)
        assert again[0] == fc_all and np.array_equal(again[1].weights_, every.weights_)          # the same bits


def test_fit_classifier_file_and_the_models_bits(tmp_path, capsys):
    """``fit_classifier`` on an AE with three sessions: the file, the messages, the read-back -- and ``loss()`` and
    ``export_latents`` give the same bits after the classifier calls as before them."""
    model, meta = _model('ae_cfg1', str(tmp_path))
    gen = _generator(meta, 3)

    def read(paths):
        out = []
        for p in paths:
            with open(p, 'rb') as f:
                out.append(f.read())
        return out

    def loss():
        model.eval()
        torch.manual_seed(1)
        x = torch.from_numpy(gen.datasets[0].images_u8[0]).to(DEV).float().div(255.0)
        return {k: float(v) for k, v in dict(model.loss({'images': x[None]}, dataset=0, accumulate_grad=False)).items()}
    latents, before = read(export_latents(gen, model)), loss()
    fc, lr = fit_classifier(model, gen, dtype='val')
    out = capsys.readouterr().out
    path = os.path.join(str(tmp_path), 'version_0', 'fc_session_classification.npy')
    assert 'FC metrics do not exist; computing from scratch' in out and 'saving results to %s' % path in out
    saved = np.load(path)
    assert saved.shape == (1,) and saved[0] == fc and isinstance(lr, clf.SessionClassifier) and 0.0 <= fc <= 1.0
    assert lr.coef_.shape == (3, 8) and lr.scores_.shape == (5, 8) and lr.C_ in lr.Cs_
    assert fc == session_classifier(gen, model, dtype='val')[0]
    again, none = fit_classifier(model, None)
    assert again == fc and none is None and 'loading results from' in capsys.readouterr().out
    assert loss() == before and read(export_latents(gen, model)) == latents
    cond, _ = _model('ae_cfg1', str(tmp_path / 'cond'))
    cond.hparams['model_class'] = 'cond-ae'
    with pytest.raises(NotImplementedError):
        fit_classifier(cond, gen)


def test_fit_writes_the_session_classifier_score(tmp_path):
    from behavenet_amd.fitting.training import fit
    from tests.cases import case_hparams, load_case, seeded_build
    from tests.test_gpu_model import BUILDERS
    _, meta = load_case('ae_cfg1')
    meta = dict(meta, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0, 'val_check_interval': 1,
                             'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0,
                             'export_latents': False, 'export_session_classifier': True, 'progress_bar': False,
                             'device': 'cuda'})
    hp = case_hparams(meta)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sessions = [SyntheticSession(6, 16, meta['dim'], seed=s, n_labels=meta['n_labels'], trial_splits='4;1;1;0')
                for s in range(2)]
    sessions[1].images_u8 = [(im * 0.7).astype(np.uint8) for im in sessions[1].images_u8]
    gen = SyntheticSessionsGenerator(sessions, device=DEV, placement='device_u8')
    model = seeded_build(BUILDERS['ae'], hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    best = fit(hp, model, gen, Exp(), method='ae')
    path = os.path.join(str(tmp_path), 'version_0', 'fc_session_classification.npy')
    assert os.path.exists(path)
    assert np.load(path)[0] == session_classifier(gen, best, dtype='val')[0]
    one = SyntheticSessionsGenerator(sessions[:1], device=DEV, placement='device_u8')
    with pytest.raises(ValueError, match="export_session_classifier.*1 session"):
        fit(hp, model, one, Exp(), method='ae')
