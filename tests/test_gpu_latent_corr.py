"""Latent correlation matrices per batch, trial and session, reduced on the device ("latent
correlations").

1. ``bn_segment_gram`` by direct C calls on operands between guard bands, the output pre-filled with a sentinel and the
   workspace guarded and NaN-filled, against ``tests/latent_corr_refs.gram_ref`` (numpy float64 with ``math.fsum``)
   within the derived tolerance of that file: counts exact, every sum within ``4 m 2^-53 sum|term|``, the same NaN
   positions, ``A[i][j]`` and ``A[j][i]`` the same bits.
2. The wrapper ``_hip.segment_gram``.
3. Whole models (the small golden PS-VAE, MSPS-VAE and AE): ``latent_correlations`` against ``np.corrcoef`` on the
   per-trial route's latents within the derived correlation bound; ``export_latent_correlations``,
   ``get_latent_corr`` and the ``fit`` key.
"""

import csv
import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting.eval import (encode_trial, export_latent_correlations, latent_correlations,
                                        summarise_gram)
from behavenet_amd.plotting.cond_ae_utils import get_latent_corr
from tests import latent_corr_refs as refs
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_ranges import LENS, _model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2
SENTINEL = -77.0
PAD = 7.0e7          # what lies in the columns from D to ld: finite, so a kernel that summed them would show


# ------------------------------------------------------------------------------------------ 1: the kernel
def _place(x, ld=None, offset=0):
    """The table on the device between guard bands, with leading dimension ``ld`` (PAD in the columns from D on; the
    last row ends after its D values) and ``offset`` ELEMENTS off its 16-byte boundary -> (view (n, D), whole)."""
    n, D = x.shape
    ld = D if ld is None else ld
    host = np.full(offset + (n - 1) * ld + D, PAD, dtype=np.float32)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (n, D), (4 * ld, 4))
    rows[...] = x
    whole = guarded(torch.from_numpy(host))
    assert whole.data_ptr() % 16 == 0
    return torch.as_strided(whole, (n, D), (ld, 1), whole.storage_offset() + offset), whole


def _doubles(shape, fill):
    count = int(np.prod(shape))
    t = guarded(torch.zeros(2 * max(count, 1))).view(torch.float64)[:count].view(shape)
    t.fill_(fill)
    return t


def _int64(values):
    values = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.int64)
    t = guarded(torch.zeros(2 * values.numel())).view(torch.int64)[:values.numel()]
    t.copy_(values)
    return t


def _workspace(n, S, D):
    nbytes = _hip.load().bn_segment_gram_ws_bytes(n, S, D)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def _call(z, ld, c, offsets, S, D, n, out, ws, nbytes):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())          # noqa: E731
    return _hip.load().bn_segment_gram(ptr(z), ld, ptr(c), ptr(offsets), S, D, n, ptr(out), ptr(ws), nbytes,
                                       torch.cuda.current_stream().cuda_stream)


def _run(z, offsets, shift=None, ld=None, offset=0, what=''):
    """One guarded call and a second one on the used workspace -> the matrices (numpy); the inputs keep their bits."""
    n, D = z.shape
    S = len(offsets) - 1
    ld = D if ld is None else ld
    placed = [_place(z, ld, offset), None if shift is None else _place(np.asarray(shift)[None], D, offset)]
    before = [None if p is None else p[1].view(torch.int32).clone() for p in placed]
    off_d = _int64(offsets)
    ws, nbytes = _workspace(n, S, D)
    out = _doubles((S, D + 1, D + 1), SENTINEL)
    args = (placed[0][0], ld, None if shift is None else placed[1][0], off_d, S, D, n, out, ws, nbytes)
    assert _call(*args) == 0, what
    first = out.clone()
    out.fill_(SENTINEL)
    assert _call(*args) == 0, what
    assert torch.equal(out.view(torch.int64), first.view(torch.int64)), (what, 'a second call gave other bits')
    for p, b in zip(placed, before):
        assert p is None or torch.equal(p[1].view(torch.int32), b), (what, 'an input was written')
    assert np.array_equal(off_d.cpu().numpy(), np.asarray(offsets)), what
    return first.cpu().numpy()


@pytest.mark.parametrize('D', refs.KERNEL_DS)
def test_kernel_against_the_reference(D):
    """Segments of 0, 1, 2, 10, 257, 1023, 0 and 4099 rows in one call after three leading rows and before two
    trailing ones that hold NaN; leading dimension D and D + 5; the table on and 4 bytes off a 16-byte boundary; with a
    shift and without; columns of mean 300, 0 and -40, one column constant within a segment."""
    z, offsets, shift = refs.kernel_case(D)
    for shifted in (True, False):
        want, mags = refs.kernel_case_ref(D, shifted)
        assert not np.isnan(want).any() and not want[0].any() and not want[6].any()
        assert (want[:, 0, 0] == np.array(refs.LENGTHS)).all()
        for ld in (D, D + 5):
            for offset in (0, 1):
                what = (D, shifted, ld, offset)
                got = _run(z, offsets, shift if shifted else None, ld, offset, what)
                refs.assert_gram_close(got, want, mags, what)
    # the constant column: its centred sum of squares is rounding noise, the summary reads it as constant
    got = summarise_gram(_run(z, offsets, shift, D, 0, 'summary'), shift)
    seg, col = refs.CONSTANT
    if D > 1:
        assert np.isnan(got['corr'][seg][col]).all() and np.isnan(got['corr'][seg][:, col]).all()
        assert np.isnan(got['corr'][seg]).sum() == 2 * D - 1
    for s in (3, 4, 5, 7):
        rows = z[offsets[s]:offsets[s + 1]]
        keep = [j for j in range(D) if (s, j) != refs.CONSTANT]
        if len(keep) > 1:
            refs.assert_corr_close(got['corr'][s][np.ix_(keep, keep)], rows[:, keep], shift[keep], (D, s))


# 70001 rows of 16 columns: SG_MIN_ELEMS = 2^14 elements a row block at least is 1024 rows, so ceil(70001 / 1024) = 69
# blocks of ceil(70001 / 69) = 1015 rows -- and the last block holds 70001 - 68 * 1015 = 981: ragged
LONG = 70001


def test_a_single_long_segment_is_split_over_row_blocks():
    blocks, rows = _hip._segment_gram_plan(LONG, 16)
    assert blocks == 69 and 0 < LONG - (blocks - 1) * rows < rows
    z = refs.mixed(LONG, 16, seed=7)
    shift = z[0]
    want, mags = refs.gram_ref(z, [0, LONG], shift)
    got = _run(z, [0, LONG], shift, 21, 0, 'long')
    refs.assert_gram_close(got, want, mags, 'long')
    refs.assert_corr_close(summarise_gram(got, shift)['corr'][0], z, shift, 'long')
    # segments that begin and end inside row blocks, at their boundaries and across several of them
    offsets = [5, rows - 1, rows, rows + 1, 3 * rows, 3 * rows, 40000, 5 * 10 ** 9, -3]
    want, mags = refs.gram_ref(z, offsets, shift)
    assert want[:, 0, 0].astype(bool).tolist() == [True, True, True, True, False, True, True, False]
    refs.assert_gram_close(_run(z, offsets, shift, 16, 0, 'crossing'), want, mags, 'crossing')


def test_a_nan_or_inf_reaches_its_row_and_column_alone():
    D = 16
    z, offsets, shift = (np.array(a) for a in refs.kernel_case(D))
    for value, (seg, col) in ((np.nan, (5, 7)), (np.inf, (7, 0)), (np.nan, (4, 15))):
        planted = z.copy()
        planted[int(offsets[seg]) + 11, col] = value
        want, mags = refs.gram_ref(planted, offsets, shift)
        got = _run(planted, offsets, shift, D + 5, 0, ('planted', value, seg, col))
        refs.assert_gram_close(got, want, mags, ('planted', value, seg, col))
        bad = ~np.isfinite(got)
        expect = np.zeros_like(bad)
        expect[seg, 1 + col, :] = expect[seg, :, 1 + col] = True
        assert np.array_equal(bad, expect), (value, seg, col)
        assert got[seg, 0, 0] == refs.LENGTHS[seg]


def test_refusals_write_nothing():
    z, offsets, shift = refs.kernel_case(3)
    n, S = z.shape[0], len(offsets) - 1
    p, c = _place(z, 8)[0], _place(shift[None], 3)[0]
    off_d = _int64(offsets)
    ws, nbytes = _workspace(n, S, 64)
    out = _doubles((S, 65, 65), SENTINEL)
    need = _hip.load().bn_segment_gram_ws_bytes(n, S, 3)
    assert _call(p, 8, c, off_d, S, 0, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 65, c, off_d, S, 65, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, c, off_d, S, 3, n, out, ws, need - 1) == E_SHAPE          # a workspace one byte short
    assert _call(None, 8, c, off_d, S, 3, n, out, ws, nbytes) == E_ARG
    assert _call(p, 8, c, None, S, 3, n, out, ws, nbytes) == E_ARG
    assert _call(p, 8, c, off_d, S, 3, n, None, ws, nbytes) == E_ARG
    assert _call(p, 8, c, off_d, S, 3, n, out, None, nbytes) == E_ARG
    assert _call(p, 2, c, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, c, off_d, -1, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, c, off_d, S, 3, -1, out, ws, nbytes) == E_SHAPE
    assert _call(p.data_ptr() + 2, 8, c, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, c.data_ptr() + 2, off_d, S, 3, n, out, ws, nbytes) == E_SHAPE
    assert _call(p, 8, c, off_d, S, 3, n, out, ws.data_ptr() + 4, nbytes) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(ws).all())
    # no segments: nothing to write, and that is no error
    assert _call(p, 8, c, off_d, 0, 3, n, out, ws, nbytes) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(ws).all())


# ------------------------------------------------------------------------------------------ 2: the wrapper
def test_wrapper():
    z, offsets, shift = refs.kernel_case(16)
    want, mags = refs.kernel_case_ref(16, True)
    plain, plain_mags = refs.kernel_case_ref(16, False)
    rng = np.random.default_rng(2)
    wide = rng.standard_normal((z.shape[0], 21)).astype(np.float32)
    wide[:, 3:19] = z
    wide_d, shift_d = torch.from_numpy(wide).to(DEV), torch.from_numpy(shift).to(DEV)
    for given in (offsets.tolist(), offsets, torch.from_numpy(offsets).to(DEV)):
        got = _hip.segment_gram(wide_d[:, 3:19], given, shift_d)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (8, 17, 17)
        refs.assert_gram_close(got.cpu().numpy(), want, mags, 'wrapper')
    refs.assert_gram_close(_hip.segment_gram(wide_d[:, 3:19], offsets).cpu().numpy(), plain, plain_mags, 'no shift')
    assert _hip.segment_gram(wide_d[:, 3:19], offsets[:1], shift_d).shape == (0, 17, 17)
    with pytest.raises(ValueError, match='must be contiguous'):
        _hip.segment_gram(wide_d[:, 3:19].t().contiguous().t(), offsets)
    with pytest.raises(ValueError, match='must be float32'):
        _hip.segment_gram(wide_d[:, 3:19].double(), offsets)
    with pytest.raises(ValueError, match='offsets int64'):
        _hip.segment_gram(wide_d[:, 3:19], torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match='shift float32'):
        _hip.segment_gram(wide_d[:, 3:19], offsets, shift_d[:15])
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.segment_gram(wide_d[:, 3:19].cpu(), offsets)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.segment_gram(wide_d[:, 3:19], offsets, shift_d.cpu())
    with pytest.raises(ValueError, match='1 to 64'):
        _hip.segment_gram(torch.zeros((2, 65), device=DEV), [0, 2])


# ------------------------------------------------------------------------------------------ 3: whole models
GOLDENS = {'psvae_cfg4': (4, 16), 'mspsvae_cfg1': (4, 8), 'ae_cfg1': (0, 8)}          # the default column block


def _generator(meta, n_sessions=1):
    sessions = [SyntheticSession(len(LENS), LENS, meta['dim'], seed=3 + s, n_labels=meta['n_labels'],
                                 trial_splits='4;1;1;1', name=('lab', 'expt', 'animal', 'sess%d' % s))
                for s in range(n_sessions)]
    return SyntheticSessionsGenerator(sessions, device=DEV, placement='device_u8')


def _per_trial_latents(model, gen, dtypes, sessions):
    """The per-trial route: ``encode_trial`` per trial, concatenated in the reference's order -- sessions ascending,
    within a session the trials in ``batch_idxs[dtype]`` order, split after split -> (table, [(session, trial, rows)])."""
    parts, keys = [], []
    for s in sessions:
        ds = gen.datasets[s]
        for dt in dtypes:
            for t in ds.batch_idxs[dt]:
                z = encode_trial(model, torch.from_numpy(ds.images_u8[int(t)]).to(DEV), s)
                parts.append(np.asarray(z, dtype=np.float32))
                keys.append((s, int(t), len(z)))
    return np.concatenate(parts, axis=0), keys


def _check_segments(got, table, offsets, lo, hi, what):
    assert got['rows'].tolist() == [[int(a), int(b)] for a, b in zip(offsets[:-1], offsets[1:])], what
    assert got['n'].tolist() == np.diff(offsets).tolist(), what
    D = hi - lo
    assert got['gram'].shape == (len(offsets) - 1, D + 1, D + 1) and got['shift'].shape == (D,)
    assert np.array_equal(got['shift'], table[0, lo:hi].astype(np.float64)), what
    for s in range(len(offsets) - 1):
        rows = table[offsets[s]:offsets[s + 1], lo:hi]
        assert len(rows) >= 2, what
        refs.assert_corr_close(got['corr'][s], rows, got['shift'], (what, s))
        pair = np.corrcoef(rows[:, [0, 1]].astype(np.float64).T)[0, 1]
        assert abs(got['abs_corr_01'][s] - abs(pair)) <= refs.corr_bound(rows, got['shift']), (what, s)
        assert np.allclose(got['mean'][s], rows.astype(np.float64).mean(axis=0), rtol=0, atol=1e-12 * np.abs(rows).max())
    refs.assert_corr_close(got['pooled']['corr'], table[offsets[0]:offsets[-1], lo:hi], got['shift'], (what, 'pooled'))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('golden', sorted(GOLDENS))
def test_latent_correlations_are_numpy_on_the_per_trial_route(golden, dtype, tmp_path):
    model, meta = _model(golden, str(tmp_path))
    model.hparams['hip_encode_dtype'] = dtype
    lo, hi = GOLDENS[golden]
    gen = _generator(meta, n_sessions=2)
    # (the reference stacks a session's trials in batch_idxs order, whatever order the generator serves them in)
    gen.datasets[1].batch_idxs['train'] = gen.datasets[1].batch_idxs['train'][[3, 0, 2, 1]]
    table, keys = _per_trial_latents(model, gen, ['train'], [0, 1])
    assert [k[1] for k in keys] == [0, 1, 2, 3, 3, 0, 2, 1]
    ends = np.concatenate(([0], np.cumsum([k[2] for k in keys])))
    total = int(ends[-1])
    by_session = [0, sum(k[2] for k in keys if k[0] == 0), total]
    expected = {None: [0, total], 7: list(range(0, total, 7)) + [total], 'trial': ends.tolist(), 'session': by_session}
    assert total % 7 and by_session[1] % 7          # a ragged last batch, and a batch across the session boundary
    for segments, offsets in expected.items():
        got = latent_correlations(gen, model, segments=segments)          # the default block, the train trials
        _check_segments(got, table, np.asarray(offsets), lo, hi, (golden, dtype, segments))
        assert ('trial' in got) == (segments == 'trial') and ('session' in got) == (segments in ('trial', 'session'))
        if segments == 'trial':
            assert got['session'].tolist() == [k[0] for k in keys] and got['trial'].tolist() == [k[1] for k in keys]
        if segments == 'session':
            assert got['session'].tolist() == [0, 1]
    # a general index list is gathered: the same numbers as the columns themselves
    picked = [hi - 1, lo, lo + 2]
    got = latent_correlations(gen, model, columns=picked)
    refs.assert_corr_close(got['corr'][0], table[:, picked], got['shift'], (golden, dtype, picked))
    # other splits, in the order given
    both, both_keys = _per_trial_latents(model, gen, ['val', 'test'], [1])
    got = latent_correlations(gen, model, dtype=['val', 'test'], sess_idx=1, segments='trial', columns=slice(lo, hi))
    assert got['trial'].tolist() == [k[1] for k in both_keys] and got['session'].tolist() == [1, 1]
    _check_segments(got, both, np.concatenate(([0], np.cumsum([k[2] for k in both_keys]))), lo, hi, (golden, 'val+test'))


def test_sessions_of_a_two_session_generator_and_the_errors(tmp_path):
    model, meta = _model('psvae_cfg4', str(tmp_path))
    gen = _generator(meta, n_sessions=2)
    both = latent_correlations(gen, model, segments='session')
    for s in (0, 1):
        one = latent_correlations(gen, model, sess_idx=s, segments='session')
        assert one['session'].tolist() == [s] and one['n'].tolist() == [both['n'][s]]
        assert one['rows'].tolist() == [[0, int(both['n'][s])]]
        table, _ = _per_trial_latents(model, gen, ['train'], [s])
        refs.assert_corr_close(one['corr'][0], table[:, 4:], one['shift'], s)
        refs.assert_corr_close(both['corr'][s], table[:, 4:], both['shift'], s)
        if s == 0:
            # session 0 leads both tables: the same shift, the same rows, the same bits
            assert np.array_equal(one['shift'], both['shift'])
            assert np.array_equal(one['gram'][0], both['gram'][0]) and np.array_equal(one['corr'][0], both['corr'][0])
        else:
            # session 1 on its own is shifted by ITS first row: the same covariance from other sums
            assert np.array_equal(one['shift'], table[0, 4:].astype(np.float64))
            assert not np.array_equal(one['shift'], both['shift'])
    assert not np.array_equal(both['corr'][0], both['corr'][1])
    again = latent_correlations(gen, model, segments='session')
    assert np.array_equal(again['gram'], both['gram'])          # the same bits on every call
    with pytest.raises(ValueError, match='latent_correlations: sessions'):
        latent_correlations(gen, model, sess_idx=2)
    sess = SyntheticSession(5, 16, meta['dim'], seed=0, n_labels=meta['n_labels'], trial_splits='4;1;0;0')
    empty = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    with pytest.raises(ValueError, match='latent_correlations: the sessions .* have no test trial'):
        latent_correlations(empty, model, dtype='test')


def _read(path):
    with open(path, newline='') as f:
        return list(csv.reader(f))


def test_csv_and_get_latent_corr(tmp_path, capsys):
    root = str(tmp_path)
    model, meta = _model('psvae_cfg4', root)
    gen = _generator(meta)
    path = export_latent_correlations(gen, model, segments=7)
    assert path == os.path.join(root, 'version_0', 'corr_unsupervised.csv')
    scores = latent_correlations(gen, model, segments=7)
    rows = _read(path)
    assert rows[0] == ['Segment', 'RowBegin', 'RowEnd', 'N', 'AbsCorr01', 'MeanAbsCorr']
    # 92 train rows: thirteen batches of seven and a last one of a single row, which has no correlation
    assert len(rows) == 1 + len(scores['n']) == 15 and np.isfinite(scores['abs_corr_01'][:-1]).all()
    assert scores['n'][-1] == 1 and np.isnan(scores['abs_corr_01'][-1]) and rows[-1][4:] == ['', '']
    for k, row in enumerate(rows[1:]):
        assert [int(v) for v in row[:4]] == [k, scores['rows'][k, 0], scores['rows'][k, 1], scores['n'][k]]
        if k < 13:
            assert float(row[4]) == scores['abs_corr_01'][k] and float(row[5]) == scores['mean_abs_offdiag'][k]
    assert _read(export_latent_correlations(gen, model, segments=7)) == rows          # the same bits on every call
    pd = pytest.importorskip('pandas')
    os.remove(path)
    first = get_latent_corr(model.hparams, model, gen, 0, batch_size=7)
    assert 'computing from scratch' in capsys.readouterr().out
    assert list(first.columns) == rows[0]
    assert np.array_equal(first['AbsCorr01'].to_numpy(), scores['abs_corr_01'], equal_nan=True)
    assert np.array_equal(first['MeanAbsCorr'].to_numpy(), scores['mean_abs_offdiag'], equal_nan=True)
    assert first['N'].tolist() == scores['n'].tolist()
    second = get_latent_corr(model.hparams, None, None, 0)          # read back: no model is needed
    assert 'loading results from' in capsys.readouterr().out
    pd.testing.assert_frame_equal(first, second)
    pooled = get_latent_corr(model.hparams, model, gen, 0, overwrite=True)
    assert 'overwriting' in capsys.readouterr().out and len(pooled) == 1
    assert pooled['AbsCorr01'][0] == latent_correlations(gen, model)['abs_corr_01'][0]


@pytest.mark.parametrize('batch_size', [None, 5])
def test_fit_writes_the_latent_correlations(batch_size, tmp_path):
    from behavenet_amd.fitting.training import fit
    from tests.cases import case_hparams, load_case, seeded_build
    from tests.test_gpu_model import BUILDERS
    _, meta = load_case('psvae_cfg4')
    meta = dict(meta, extra_hp=dict(meta['extra_hp']))
    meta['extra_hp'].update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0, 'val_check_interval': 1,
                             'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0,
                             'export_latents': False, 'export_latent_corr': True, 'progress_bar': False,
                             'device': 'cuda'})
    if batch_size is not None:
        meta['extra_hp']['latent_corr_batch_size'] = batch_size
    hp = case_hparams(meta)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(6, 16, meta['dim'], seed=0, n_labels=meta['n_labels'], trial_splits='4;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    model = seeded_build(BUILDERS['ps-vae'], hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    best = fit(hp, model, gen, Exp(), method='ae')
    path = os.path.join(str(tmp_path), 'version_0', 'corr_unsupervised.csv')
    assert os.path.exists(path)
    rows = _read(path)
    want = latent_correlations(gen, best, dtype='train', segments=batch_size)
    n_train = 16 * len(sess.batch_idxs['train'])
    assert int(rows[-1][2]) == n_train and len(rows) == 1 + (1 if batch_size is None else -(-n_train // batch_size))
    assert [float(r[4]) for r in rows[1:]] == want['abs_corr_01'].tolist()
    assert [float(r[5]) for r in rows[1:]] == want['mean_abs_offdiag'].tolist()
