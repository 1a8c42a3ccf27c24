"""Label R^2 and MSE per trial, reduced on the device ("label scores").

1. ``bn_segment_label_sums`` by direct C calls on operands between guard bands, the output pre-filled with a sentinel
   and the workspace guarded too, against ``tests/label_r2_refs.sums_ref`` (numpy float64 with ``math.fsum``) within
   the derived tolerance of that file: counts exact, every sum within ``4 m 2^-53 sum|term|``, the same NaN positions.
2. Whole models (the small golden PS-VAE and AE-MSP): ``label_r2`` against the per-trial route's own numbers, the
   AE-MSP's latents against ``get_transformed_latents(images)``;
   ``export_label_r2``, ``get_label_r2`` and the ``fit`` key.
"""

import csv
import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession
from behavenet_amd.fitting.eval import encode_trial, export_label_r2, label_r2, summarise_label_sums
from behavenet_amd.hip_functions import encode_precision
from behavenet_amd.plotting.cond_ae_utils import get_label_r2
from tests import label_r2_refs as refs
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_ranges import LENS, _model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2
SENTINEL = -77.0
PAD = 7.0e7          # what lies in the columns from L to ld: finite, so a kernel that summed them would show


# ------------------------------------------------------------------------------------------ 1: the kernel
def _place(x, ld=None, offset=0):
    """The table on the device between guard bands, with leading dimension ``ld`` (PAD in the columns from L on; the
    last row ends after its L values) and ``offset`` ELEMENTS off its 16-byte boundary -> (view (n, L), whole)."""
    n, L = x.shape
    ld = L if ld is None else ld
    host = np.full(offset + (n - 1) * ld + L, PAD, dtype=np.float32)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (n, L), (4 * ld, 4))
    rows[...] = x
    whole = guarded(torch.from_numpy(host))
    assert whole.data_ptr() % 16 == 0
    return torch.as_strided(whole, (n, L), (ld, 1), whole.storage_offset() + offset), whole


def _doubles(shape, fill):
    """float64 values on the device between guard bands."""
    count = int(np.prod(shape))
    t = guarded(torch.zeros(2 * max(count, 1))).view(torch.float64)[:count].view(shape)
    t.fill_(fill)
    return t


def _int64(values):
    values = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.int64)
    t = guarded(torch.zeros(2 * values.numel())).view(torch.int64)[:values.numel()]
    t.copy_(values)
    return t


def _workspace(n, S, L):
    nbytes = _hip.load().bn_segment_label_sums_ws_bytes(n, S, L)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def _call(pred, ld_pred, truth, ld_truth, mask, ld_mask, offsets, S, L, n, out, ws, nbytes):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())          # noqa: E731
    return _hip.load().bn_segment_label_sums(ptr(pred), ld_pred, ptr(truth), ld_truth, ptr(mask), ld_mask, ptr(offsets),
                                             S, L, n, ptr(out), ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)


def _run(pred, truth, mask, offsets, ld_pred=None, offset=0, what=''):
    """One guarded call and a second one on the used workspace -> the sums (numpy); the inputs keep their bits."""
    n, L = truth.shape
    S = len(offsets) - 1
    ld_pred = L if ld_pred is None else ld_pred
    placed = [_place(pred, ld_pred, offset), _place(truth, L, offset), None if mask is None else _place(mask, L, offset)]
    before = [None if p is None else p[1].view(torch.int32).clone() for p in placed]
    off_d = _int64(offsets)
    ws, nbytes = _workspace(n, S, L)
    out = _doubles((S, L, 4), SENTINEL)
    args = (placed[0][0], ld_pred, placed[1][0], L, None if mask is None else placed[2][0], L if mask is not None else 0,
            off_d, S, L, n, out, ws, nbytes)
    assert _call(*args) == 0, what
    first = out.clone()
    out.fill_(SENTINEL)
    assert _call(*args) == 0, what
    assert torch.equal(out.view(torch.int64), first.view(torch.int64)), (what, 'a second call gave other bits')
    for p, b in zip(placed, before):
        assert p is None or torch.equal(p[1].view(torch.int32), b), (what, 'an input was written')
    assert np.array_equal(off_d.cpu().numpy(), np.asarray(offsets)), what
    return first.cpu().numpy()


@pytest.mark.parametrize('L', [1, 3, 16, 64])
def test_kernel_against_the_reference(L):
    """Segments of 0, 1, 10, 11, 257, 1023, 0 and 4099 rows in one call after three leading rows; the predictions with
    leading dimension L and L + 5; the tables on and 4 bytes off a 16-byte boundary; without a mask, and with one of
    about 80 % ones that is all zero in one segment; labels of mean 300 and deviation 50, one column constant within
    a segment.  The rows of no segment hold NaNs under a one mask."""
    for with_mask in (False, True):
        pred, truth, mask, offsets = refs.kernel_case(L, with_mask)
        want, mags = refs.kernel_case_ref(L, with_mask)
        assert not np.isnan(want).any() and want[0].sum() == 0 and want[6].sum() == 0
        if not with_mask:
            assert (want[:, :, 0] == np.array(refs.LENGTHS)[:, None]).all()
        else:
            assert want[refs.ALL_ZERO_SEGMENT].sum() == 0 and 0.7 < want[7, :, 0].mean() / 4099 < 0.9
        for ld_pred in (L, L + 5):
            for offset in (0, 1):
                what = (L, with_mask, ld_pred, offset)
                got = _run(pred, truth, mask, offsets, ld_pred, offset, what)
                refs.assert_sums_close(got, want, mags, what)


# 70001 rows of 16 columns: SL_MIN_ELEMS = 2^14 elements a row block at least is 1024 rows, so ceil(70001 / 1024) = 69
# blocks of ceil(70001 / 69) = 1015 rows -- and the last block holds 70001 - 68 * 1015 = 981: ragged
LONG = 70001


def test_a_single_long_segment_is_split_over_row_blocks():
    blocks, rows = _hip._segment_sums_plan(LONG, 16)
    assert blocks == 69 and 0 < LONG - (blocks - 1) * rows < rows
    rng = np.random.default_rng(7)
    truth = (300 + 50 * rng.standard_normal((LONG, 16))).astype(np.float32)
    pred = (truth + 20 * rng.standard_normal((LONG, 16))).astype(np.float32)
    mask = (rng.random((LONG, 16)) < 0.8).astype(np.float32)
    want, mags = refs.sums_ref(pred, truth, mask, [0, LONG], 16)
    refs.assert_sums_close(_run(pred, truth, mask, [0, LONG], 21, 0, 'long'), want, mags, 'long')
    # segments that begin and end inside row blocks, at their boundaries and across several of them
    offsets = [5, rows - 1, rows, rows + 1, 3 * rows, 3 * rows, 40000, 5 * 10 ** 9, -3]
    want, mags = refs.sums_ref(pred, truth, mask, offsets, 16)
    assert want[:, 0, 0].astype(bool).tolist() == [True, True, True, True, False, True, True, False]
    refs.assert_sums_close(_run(pred, truth, mask, offsets, 16, 0, 'crossing'), want, mags, 'crossing')


def test_invalid_entries_are_selected_out():
    L = 16
    pred, truth, mask, offsets = (np.array(a) for a in refs.kernel_case(L, True))
    rng = np.random.default_rng(11)
    inside = slice(int(offsets[0]), int(offsets[-1]))
    zero = np.argwhere(mask[inside] == 0) + [int(offsets[0]), 0]
    assert len(zero) > 3000
    bad = [np.nan, np.inf, -np.inf]
    for k, (i, j) in enumerate(zero[rng.permutation(len(zero))[:3000]]):
        (truth if k % 2 else pred)[i, j] = bad[k % 3]
        if k % 5 == 0:
            truth[i, j] = pred[i, j] = bad[(k // 5) % 3]
    # mask values that are not one are not valid either
    ones = np.argwhere(mask[inside] == 1) + [int(offsets[0]), 0]
    for k, (i, j) in enumerate(ones[rng.permutation(len(ones))[:300]]):
        mask[i, j] = [0.5, 2.0, np.nan][k % 3]
        truth[i, j] = 1e30
    want, mags = refs.sums_ref(pred, truth, mask, offsets, L)
    assert np.isfinite(want).all() and want[..., 1].max() < 1e9
    got = _run(pred, truth, mask, offsets, L + 5, 0, 'planted')
    assert np.isfinite(got).all()
    refs.assert_sums_close(got, want, mags, 'planted')
    # one NaN under a one mask: exactly that (segment, column)
    seg, col = 5, 7
    i = int(offsets[seg]) + int(np.argmax(mask[offsets[seg]:offsets[seg + 1], col] == 1))
    assert mask[i, col] == 1
    truth[i, col] = np.nan
    want, mags = refs.sums_ref(pred, truth, mask, offsets, L)
    got = _run(pred, truth, mask, offsets, L, 0, 'one NaN')
    refs.assert_sums_close(got, want, mags, 'one NaN')
    nan = np.isnan(got)
    assert nan[seg, col, 1:].all() and not nan[seg, col, 0] and nan.sum() == 3
    # ... and in the prediction alone only the squared error is lost
    truth[i, col] = 300
    pred[i, col] = np.nan
    got = _run(pred, truth, mask, offsets, L, 0, 'one NaN prediction')
    nan = np.isnan(got)
    assert nan[seg, col, 3] and nan.sum() == 1


def test_refusals_write_nothing():
    pred, truth, mask, offsets = refs.kernel_case(3, True)
    n, S = truth.shape[0], len(offsets) - 1
    p, t, m = _place(pred, 8)[0], _place(truth, 3)[0], _place(mask, 3)[0]
    off_d = _int64(offsets)
    ws, nbytes = _workspace(n, S, 64)
    out = _doubles((S, 64, 4), SENTINEL)
    need = _hip.load().bn_segment_label_sums_ws_bytes(n, S, 3)
    assert _call(p, 8, t, 3, m, 3, off_d, S, 0, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 65, t, 65, m, 65, off_d, S, 65, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, t, 3, m, 3, off_d, S, 3, n, out, ws, need - 1) == E_SHAPE          # a workspace one byte short
    assert _call(None, 8, t, 3, m, 3, off_d, S, 3, n, out, ws, nbytes) == E_ARG
    assert _call(p, 8, None, 3, m, 3, off_d, S, 3, n, out, ws, nbytes) == E_ARG
    assert _call(p, 8, t, 3, m, 3, None, S, 3, n, out, ws, nbytes) == E_ARG
    assert _call(p, 8, t, 3, m, 3, off_d, S, 3, n, None, ws, nbytes) == E_ARG
    assert _call(p, 8, t, 3, m, 3, off_d, S, 3, n, out, None, nbytes) == E_ARG
    assert _call(p, 2, t, 3, m, 3, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, t, 3, m, 2, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, t, 3, m, 3, off_d, -1, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, t, 3, m, 3, off_d, S, 3, -1, out, ws, nbytes) == E_SHAPE
    assert _call(p.data_ptr() + 2, 8, t, 3, m, 3, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, t, 3, m, 3, off_d, S, 3, n, out, ws.data_ptr() + 4, nbytes) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(ws).all())
    # no segments: nothing to write, and that is no error
    assert _call(p, 8, t, 3, m, 3, off_d, 0, 3, n, out, ws, nbytes) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(ws).all())


def test_wrapper():
    pred, truth, mask, offsets = refs.kernel_case(16, True)
    want, mags = refs.kernel_case_ref(16, True)
    rng = np.random.default_rng(2)
    wide = rng.standard_normal((pred.shape[0], 21)).astype(np.float32)
    wide[:, :16] = pred
    wide_d, truth_d, mask_d = (torch.from_numpy(a).to(DEV) for a in (wide, truth, mask))
    for given in (offsets, torch.from_numpy(offsets).to(DEV)):
        got = _hip.segment_label_sums(wide_d[:, :16], truth_d, mask_d, given)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (8, 16, 4)
        refs.assert_sums_close(got.cpu().numpy(), want, mags, 'wrapper')
    plain, plain_mags = refs.kernel_case_ref(16, False)
    refs.assert_sums_close(_hip.segment_label_sums(wide_d[:, :16], truth_d, None, offsets).cpu().numpy(), plain,
                           plain_mags, 'no mask')
    assert _hip.segment_label_sums(wide_d[:, :16], truth_d, None, offsets[:1]).shape == (0, 16, 4)
    with pytest.raises(ValueError, match='must be contiguous'):
        _hip.segment_label_sums(wide_d[:, :16], truth_d.t().contiguous().t(), None, offsets)
    with pytest.raises(ValueError, match='truth is'):
        _hip.segment_label_sums(wide_d[:, :15], truth_d, None, offsets)
    with pytest.raises(ValueError, match='offsets int64'):
        _hip.segment_label_sums(wide_d[:, :16], truth_d, None, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.segment_label_sums(wide_d[:, :16], truth_d, mask_d.cpu(), offsets)
    with pytest.raises(ValueError, match='1 to 64'):
        _hip.segment_label_sums(torch.zeros((2, 65), device=DEV), torch.zeros((2, 65), device=DEV), None, [0, 2])


# ------------------------------------------------------------------------------------------ 2: whole models
def _generator(meta, n_sessions=1):
    sessions = [SyntheticSession(len(LENS), LENS, meta['dim'], seed=3 + s, n_labels=meta['n_labels'],
                                 trial_splits='4;1;1;1', name=('lab', 'expt', 'animal', 'sess%d' % s))
                for s in range(n_sessions)]
    rng = np.random.default_rng(9)
    for sess in sessions:
        sess.labels_masks = [(rng.random(l.shape) < 0.8).astype(np.float32) for l in sess.labels]
        for m in sess.labels_masks:
            if len(m) == 12:
                m[:2] = 0          # (ten valid entries at most, whatever was drawn)
    return refs.MaskedSessionsGenerator(sessions, device=DEV, placement='device_u8')


def _per_trial_sums(model, gen, sess, trial):
    """One trial by the per-trial route, with the served labels and masks.  PS-VAE:
    ``get_transformed_latents(encode_trial(...))``.  AE-MSP: ``encode_trial`` has applied ``U`` already, so its latents
    ARE the transformed ones; they are first held against the reference's own call, ``get_transformed_latents(images)``
    -- another GEMM on the same encoder output, so equal up to the rounding of an fp32 dot product of K terms in any
    order, ``2 K 2^-24 sum_k |U_jk z_k|`` -- and a second ``U`` on top of them is shown to lie far outside that."""
    ds = gen.datasets[sess]
    images = torch.from_numpy(ds.images_u8[trial]).to(DEV)
    z = encode_trial(model, images, sess)
    L = model.hparams['n_labels']
    if model.hparams['model_class'] == 'cond-ae-msp':
        with torch.no_grad(), encode_precision(model.hparams['hip_encode_dtype']):
            by_images = model.get_transformed_latents(images, dataset=sess)
            plain = model.encoding(images, dataset=sess)[0]
        U = model.U.weight.detach()
        bound = (2 * U.shape[1] * 2.0 ** -24 * (plain.abs().double() @ U.abs().double().t())).cpu().numpy()
        assert (np.abs(z.astype(np.float64) - by_images) <= bound).all(), np.abs(z - by_images).max()
        twice = (torch.from_numpy(z).to(DEV) @ U.t()).cpu().numpy()
        assert (np.abs(twice - by_images)[:, :L] > 100 * bound[:, :L]).mean() > 0.9
        pred = z
    else:
        pred = model.get_transformed_latents(torch.from_numpy(z).to(DEV))
    return refs.sums_ref(pred[:, :L], ds.labels[trial], ds.labels_masks[trial], [0, len(z)], L)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('golden', ['psvae_cfg4', 'aemsp_cfg1'])
def test_label_r2_is_the_per_trial_route(golden, dtype, tmp_path):
    model, meta = _model(golden, str(tmp_path))
    if golden == 'aemsp_cfg1':
        model.create_orthogonal_matrix()
    model.hparams['hip_encode_dtype'] = dtype
    gen = _generator(meta)
    ds = gen.datasets[0]
    reference = {}
    for split in ('val', 'test', ['train', 'val']):
        kinds = [split] if isinstance(split, str) else split
        got = label_r2(gen, model, split)
        assert sorted(got['trial'].tolist()) == sorted(int(t) for k in kinds for t in ds.batch_idxs[k])
        n_first = len(ds.batch_idxs[kinds[0]])          # the walk goes split by split
        assert set(got['trial'][:n_first].tolist()) == set(int(t) for t in ds.batch_idxs[kinds[0]])
        assert got['session'].tolist() == [0] * len(got['trial']) and got['sums'].shape == (len(got['trial']), 4, 4)
        for k, t in enumerate(int(t) for t in got['trial']):
            if t not in reference:
                reference[t] = _per_trial_sums(model, gen, 0, t)
            refs.assert_sums_close(got['sums'][k], reference[t][0][0], reference[t][1][0], (golden, dtype, split, t))
        again = summarise_label_sums(got['sums'])
        for key in ('n', 'r2', 'mse'):
            assert np.array_equal(got[key], again[key], equal_nan=True)
        # 12 frames under an 80 % mask are at or under min_valid: no score, but the count and the sums are there
        few = np.array([LENS[t] == 12 for t in got['trial']])
        assert (got['n'][few] <= 10).all() and np.isnan(got['r2'][few]).all() and np.isnan(got['mse'][few]).all()
        assert (got['n'][few] > 0).all() and np.isfinite(got['sums'][few]).all()
        assert np.array_equal(np.isnan(got['r2']), got['n'] <= 10) and (got['n'][~few] > 10).all()
        assert (got['mse'][~few] > 0).all()
        assert few.any() == ('train' in kinds)
        assert np.isfinite(got['pooled']['r2_variance_weighted'])


def test_sessions_of_a_two_session_generator_and_the_class_check(tmp_path):
    model, meta = _model('psvae_cfg4', str(tmp_path))
    gen = _generator(meta, n_sessions=2)
    both = label_r2(gen, model, ['val', 'test'])
    assert sorted(zip(both['session'].tolist(), both['trial'].tolist())) == sorted(
        (s, int(t)) for s in (0, 1) for k in ('val', 'test') for t in gen.datasets[s].batch_idxs[k])
    for s in (0, 1):
        one = label_r2(gen, model, ['val', 'test'], sess_idx=s)
        assert one['session'].tolist() == [s] * 2
        for k, t in enumerate(one['trial']):
            at = [i for i in range(len(both['trial'])) if both['session'][i] == s and both['trial'][i] == t]
            assert len(at) == 1 and np.array_equal(one['sums'][k], both['sums'][at[0]])          # the same bits
            want, mags = _per_trial_sums(model, gen, s, int(t))
            refs.assert_sums_close(one['sums'][k], want[0], mags[0], (s, t))
    assert not np.array_equal(both['sums'][both['session'] == 0], both['sums'][both['session'] == 1])
    with pytest.raises(ValueError, match='sessions'):
        label_r2(gen, model, 'val', sess_idx=2)
    ae, ae_meta = _model('ae_cfg1', str(tmp_path))
    with pytest.raises(ValueError, match="'ae'"):
        label_r2(gen, ae, 'val')


def test_csv_and_get_label_r2(tmp_path, capsys):
    root = str(tmp_path)
    model, meta = _model('psvae_cfg4', root)
    gen = _generator(meta)
    names = ['a', 'b', 'c', 'd']
    path = export_label_r2(gen, model, label_names=names, dtype=['train', 'val'])
    assert path == os.path.join(root, 'version_0', 'r2_supervised.csv')
    scores = label_r2(gen, model, ['train', 'val'])
    at = {int(t): k for k, t in enumerate(scores['trial'])}
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Trial', 'Label', 'R2', 'MSE', 'Model', 'Session'] and len(rows) == 1 + 4 * len(at)
    for r, row in enumerate(rows[1:]):
        k = at[int(row[0])]
        assert row[1] == names[r % 4] and row[4:] == ['MSPS-VAE', '0'] and row[0] == rows[1 + r - r % 4][0]
        for cell, value in ((row[2], scores['r2'][k, r % 4]), (row[3], scores['mse'][k, r % 4])):
            assert (cell == '') if np.isnan(value) else (float(cell) == value)          # (the same bits on every call)
    pd = pytest.importorskip('pandas')
    os.remove(path)
    first = get_label_r2(model.hparams, model, gen, 0, names)
    assert 'computing from scratch' in capsys.readouterr().out
    val = label_r2(gen, model, 'val')
    assert list(first.columns) == ['Trial', 'Label', 'R2', 'MSE', 'Model', 'Session']
    assert first['Trial'].tolist() == np.repeat(val['trial'], 4).tolist() and first['Label'].tolist() == names
    assert np.array_equal(first['R2'].to_numpy(), val['r2'].reshape(-1)) and np.isfinite(val['r2']).all()
    assert np.array_equal(first['MSE'].to_numpy(), val['mse'].reshape(-1))
    second = get_label_r2(model.hparams, None, None, 0, names)          # read back: no model is needed
    assert 'loading results from' in capsys.readouterr().out
    pd.testing.assert_frame_equal(first, second)


def test_fit_writes_the_label_scores(tmp_path):
    from behavenet_amd.fitting.training import fit
    from tests.cases import case_hparams, load_case, seeded_build
    from tests.test_gpu_model import BUILDERS
    _, meta = load_case('psvae_cfg4')
    meta = dict(meta, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0, 'val_check_interval': 1,
                             'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0,
                             'export_latents': False, 'export_label_r2': True, 'progress_bar': False, 'device': 'cuda'})
    hp = case_hparams(meta)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(6, 16, meta['dim'], seed=0, n_labels=meta['n_labels'], trial_splits='4;1;1;0')
    gen = refs.MaskedSessionsGenerator([sess], device=DEV, placement='device_u8')
    model = seeded_build(BUILDERS['ps-vae'], hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    best = fit(hp, model, gen, Exp(), method='ae')
    path = os.path.join(str(tmp_path), 'version_0', 'r2_supervised.csv')
    assert os.path.exists(path)
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    want = label_r2(gen, best, 'val')
    assert len(rows) == 1 + 4 and [int(r[0]) for r in rows[1:]] == [int(want['trial'][0])] * 4
    assert [float(r[2]) for r in rows[1:]] == want['r2'][0].tolist()
