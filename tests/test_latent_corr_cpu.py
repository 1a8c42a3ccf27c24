"""Latent correlations without a GPU ("latent correlations"): the numpy reference against
``np.cov`` / ``np.corrcoef``; ``summarise_gram`` on the reference's matrices within the derived bound, its NaN rules
and the pooled result; emulations of a device's sums on both sides of the bound; the row order, the segment builder
and the default columns of ``latent_correlations``; the csv and ``get_latent_corr``'s read-back; the refusals."""

import csv
import os
import types

import numpy as np
import pytest

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.fitting import training
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import latent_corr_refs as refs


# ------------------------------------------------------------------------------------------ reference, summary
def test_reference_against_numpy():
    z = refs.mixed(500, 5, seed=1)
    offsets = [0, 200, 500]
    shift = z[0]
    A, mags = refs.gram_ref(z, offsets, shift)
    assert A.shape == (2, 6, 6) and A[:, 0, 0].tolist() == [200, 300] and (mags >= np.abs(A)).all()
    assert np.array_equal(A, np.swapaxes(A, 1, 2))
    for s in range(2):
        rows = z[offsets[s]:offsets[s + 1]].astype(np.float64)
        n, sums, G = A[s, 0, 0], A[s, 0, 1:], A[s, 1:, 1:]
        cov = (G - np.outer(sums, sums) / n) / (n - 1)
        assert np.allclose(cov, np.cov(rows.T), rtol=1e-10, atol=0)
        assert np.allclose(shift + sums / n, rows.mean(axis=0), rtol=0, atol=1e-13 * np.abs(rows).max())


@pytest.mark.parametrize('shifted', [True, False])
def test_summary_within_the_bound(shifted):
    lens = [2, 10, 257, 4099]
    for D, means in ((3, 0), (16, None), (2, 300)):
        z = refs.mixed(sum(lens), D, seed=2, means=means)
        offsets = np.concatenate(([0], np.cumsum(lens)))
        shift = z[0] if shifted else None
        A, _ = refs.gram_ref(z, offsets, shift)
        got = bn_eval.summarise_gram(A, shift)
        assert sorted(got) == ['corr', 'cov', 'mean', 'mean_abs_offdiag', 'n', 'pooled']
        assert got['n'].tolist() == lens and got['n'].dtype == np.int64
        assert got['mean'].shape == (4, D) and got['cov'].shape == got['corr'].shape == (4, D, D)
        for s in range(len(lens)):
            rows = z[offsets[s]:offsets[s + 1]]
            refs.assert_corr_close(got['corr'][s], rows, shift, (D, means, s))
            r64 = rows.astype(np.float64)
            scale = np.sqrt(np.outer(r64.var(axis=0, ddof=1), r64.var(axis=0, ddof=1)))
            assert (np.abs(got['cov'][s] - np.cov(r64.T).reshape(D, D)) <= refs.corr_bound(rows, shift) * scale).all()
            assert np.allclose(got['mean'][s], r64.mean(axis=0), rtol=1e-12, atol=1e-12)
            iu = np.triu_indices(D, 1)
            assert abs(got['mean_abs_offdiag'][s] - np.abs(got['corr'][s][iu]).mean()) <= 1e-15
            assert (np.abs(got['corr'][s]) <= 1).all() and (np.diag(got['corr'][s]) == 1).all()
        # pooled: the matrices added over the segments are the one-segment matrix
        refs.assert_corr_close(got['pooled']['corr'], z, shift, (D, means, 'pooled'))
        one = bn_eval.summarise_gram(A.sum(axis=0)[None], shift)
        for key in ('n', 'mean', 'cov', 'corr', 'mean_abs_offdiag'):
            assert np.array_equal(np.asarray(one[key])[0], got['pooled'][key]), key
            assert np.array_equal(np.asarray(one['pooled'][key]), got['pooled'][key]), key
        assert got['pooled']['n'] == sum(lens)


def test_nan_rules():
    z = refs.mixed(40, 3, seed=3)
    z[10:30, 1] = np.float32(317.25)          # constant within the second segment
    offsets = [0, 0, 1, 10, 30, 40]           # empty, one row, nine, twenty, ten
    for shift in (None, z[0]):
        A, _ = refs.gram_ref(z, offsets, shift)
        got = bn_eval.summarise_gram(A, shift)
        assert got['n'].tolist() == [0, 1, 9, 20, 10]
        assert np.isnan(got['corr'][:2]).all() and np.isnan(got['cov'][:2]).all()          # n < 2
        assert np.isnan(got['mean'][0]).all() and np.array_equal(got['mean'][1], z[0].astype(np.float64))
        assert np.isnan(got['mean_abs_offdiag'][:2]).all()
        assert np.isfinite(got['corr'][2]).all() and np.isfinite(got['corr'][4]).all()
        nan = np.isnan(got['corr'][3])
        assert nan[1].all() and nan[:, 1].all() and nan.sum() == 5          # the constant column, and nothing else
        assert np.isnan(got['mean_abs_offdiag'][3]) and abs(got['cov'][3][1, 1]) < 1e-6
        assert np.isfinite(got['pooled']['corr']).all()
    # D = 1: a matrix of one, no pair
    A, _ = refs.gram_ref(z[:, :1], [0, 40], z[0, :1])
    got = bn_eval.summarise_gram(A, z[0, :1])
    assert got['corr'].tolist() == [[[1.0]]] and np.isnan(got['mean_abs_offdiag']).all()
    assert np.isnan(got['pooled']['mean_abs_offdiag'])
    with pytest.raises(ValueError, match='summarise_gram'):
        bn_eval.summarise_gram(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match='summarise_gram'):
        bn_eval.summarise_gram(np.zeros((2, 3, 3)), np.zeros(3))


@pytest.mark.parametrize('n, D, mean', refs.EMULATION_CASES)
def test_emulated_sums_on_both_sides_of_the_bound(n, D, mean):
    """Float64 sums in another order stay inside the correlation bound, with and without the shift; the same sums
    accumulated in fp32 (blockwise, the kindest order) miss it a hundred times over: the bound has teeth."""
    z = refs.mixed(n, D, seed=5, means=mean)
    for shift in (z[0], None):
        got = bn_eval.summarise_gram(refs.gram_emulated(z, shift, np.float64), shift)['corr'][0]
        refs.assert_corr_close(got, z, shift, (n, D, mean, shift is None))
    low = bn_eval.summarise_gram(refs.gram_emulated(z, z[0], np.float32), z[0])['corr'][0]
    want = np.corrcoef(z.astype(np.float64).T)
    with np.errstate(invalid='ignore'):
        err = np.nanmax(np.abs(low - want)) if np.isfinite(low).any() else np.inf
    assert err > 100 * refs.corr_bound(z, z[0]), (err, refs.corr_bound(z, z[0]))


# ------------------------------------------------------------------------------------------ order, segments, columns
def test_row_order_is_the_reference_stack():
    idxs = [{'train': np.array([5, 0, 3]), 'val': np.array([1]), 'test': np.array([4])},
            {'train': np.array([2, 7]), 'val': np.array([0]), 'test': np.array([], dtype=int)}]
    order = bn_eval._corr_trial_order
    assert order(idxs, ['train'], {0, 1}) == [(0, 5), (0, 0), (0, 3), (1, 2), (1, 7)]
    assert order(idxs, ['val', 'train'], {0, 1}) == [(0, 1), (0, 5), (0, 0), (0, 3), (1, 0), (1, 2), (1, 7)]
    assert order(idxs, ['train', 'test'], {1}) == [(1, 2), (1, 7)]


def test_segment_builder():
    keys = [(0, 5), (0, 0), (0, 3), (1, 2), (1, 7)]
    lens = [20, 33, 12, 27, 16]          # 65 rows of session 0, 43 of session 1: 108
    seg = bn_eval._corr_segments
    offsets, sess, trial = seg('t', keys, lens, None)
    assert offsets.tolist() == [0, 108] and offsets.dtype == np.int64 and sess is None and trial is None
    offsets, sess, trial = seg('t', keys, lens, 25)
    # batches cross the trial boundaries at 20, 53, 65 (a session boundary too), 92; the last one holds 8 rows
    assert offsets.tolist() == [0, 25, 50, 75, 100, 108] and sess is None and trial is None
    assert seg('t', keys, lens, 108)[0].tolist() == [0, 108] and seg('t', keys, lens, 1000)[0].tolist() == [0, 108]
    assert seg('t', keys, lens, 1)[0].tolist() == list(range(109))
    assert seg('t', keys, lens, np.int64(54))[0].tolist() == [0, 54, 108]
    offsets, sess, trial = seg('t', keys, lens, 'trial')
    assert offsets.tolist() == [0, 20, 53, 65, 92, 108]
    assert sess.tolist() == [0, 0, 0, 1, 1] and trial.tolist() == [5, 0, 3, 2, 7]
    offsets, sess, trial = seg('t', keys, lens, 'session')
    assert offsets.tolist() == [0, 65, 108] and sess.tolist() == [0, 1] and trial is None
    offsets, sess, _ = seg('t', keys[3:], lens[3:], 'session')
    assert offsets.tolist() == [0, 43] and sess.tolist() == [1]
    for bad in (0, -3, 'batch', 2.5, True, [4]):
        with pytest.raises(ValueError, match='^t: '):
            seg('t', keys, lens, bad)


def test_default_columns_per_class():
    cols = bn_eval._corr_columns
    assert cols('t', {'model_class': 'ps-vae', 'n_labels': 4}, 16, None) == (4, 16)
    assert cols('t', {'model_class': 'msps-vae', 'n_labels': 2, 'n_background': 2}, 8, None) == (4, 8)
    for model_class in ('ae', 'vae', 'beta-tcvae', 'cond-ae', 'cond-vae', 'cond-ae-msp'):
        assert cols('t', {'model_class': model_class, 'n_labels': 4}, 8, None) == (0, 8)
    hp = {'model_class': 'ae'}
    assert cols('t', hp, 16, slice(3, None)) == (3, 16) and cols('t', hp, 16, [5, 6, 7]) == (5, 8)
    assert cols('t', hp, 16, slice(-2, None)) == (14, 16) and cols('t', hp, 16, np.arange(4)) == (0, 4)
    assert cols('t', hp, 16, [7, 5, 6]).tolist() == [7, 5, 6] and cols('t', hp, 16, slice(0, 8, 2)).tolist() == [0, 2, 4, 6]
    assert cols('t', hp, 100, slice(10, 74)) == (10, 74)
    for bad, match in (([16], '16 latents'), ([-1, 0], '16 latents'), ([], 'at least one'), ([0.5], 'at least one'),
                       (slice(4, 4), 'at least one')):
        with pytest.raises(ValueError, match=match):
            cols('t', hp, 16, bad)
    with pytest.raises(ValueError, match='1 to 64'):
        cols('t', hp, 100, None)
    with pytest.raises(ValueError, match='1 to 64'):
        cols('t', hp, 100, list(range(0, 100, 2)) + list(range(1, 31, 2)))


def test_the_entry_points_name_themselves_in_their_errors():
    model = types.SimpleNamespace(hparams={'model_class': 'ps-vae', 'n_labels': 4, 'n_ae_latents': 16})
    for kwargs, match in (({'segments': 0}, 'latent_correlations: batches of 0 rows'),
                          ({'segments': 'frames'}, 'latent_correlations: segments must be'),
                          ({'columns': [16]}, 'latent_correlations: columns'),
                          ({'dtype': 'all'}, 'latent_correlations: dtype must be')):
        with pytest.raises(ValueError, match=match):
            bn_eval.latent_correlations(None, model, **kwargs)
    wide = types.SimpleNamespace(hparams={'model_class': 'ae', 'n_ae_latents': 65})
    with pytest.raises(ValueError, match='latent_correlations: 65 columns'):
        bn_eval.latent_correlations(None, wide)
    assert {'summarise_gram', 'latent_correlations', 'export_latent_correlations'} <= set(bn_eval.__all__)
    assert 'get_latent_corr' in cau.__all__


def test_fit_refuses_a_bad_batch_size_before_the_first_epoch():
    hp = {'export_latent_corr': True, 'latent_corr_batch_size': 0}
    model = types.SimpleNamespace(hparams={'model_class': 'ae'})
    with pytest.raises(ValueError, match='latent_corr_batch_size'):
        training._fit(hp, model, None, None, method='ae')


# ------------------------------------------------------------------------------------------ csv
def test_csv_and_read_back(tmp_path, capsys):
    z = refs.mixed(60, 3, seed=8)
    z[20:22] = z[20]          # a segment of two equal rows: every column constant
    offsets = np.array([0, 20, 22, 22, 60])
    A, _ = refs.gram_ref(z, offsets, z[0])
    scores = bn_eval.summarise_gram(A, z[0])
    scores['rows'] = np.stack([offsets[:-1], offsets[1:]], axis=1)
    scores['abs_corr_01'] = np.abs(scores['corr'][:, 0, 1])
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'version_3'))
    path = os.path.join(root, 'version_3', 'corr_unsupervised.csv')
    assert bn_eval._write_latent_corr_csv(path, scores) == path
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Segment', 'RowBegin', 'RowEnd', 'N', 'AbsCorr01', 'MeanAbsCorr'] and len(rows) == 5
    assert [r[:4] for r in rows[1:]] == [['0', '0', '20', '20'], ['1', '20', '22', '2'], ['2', '22', '22', '0'],
                                         ['3', '22', '60', '38']]
    assert rows[2][4:] == ['', ''] and rows[3][4:] == ['', '']          # NaN: an empty field
    for k in (0, 3):
        assert float(rows[1 + k][4]) == scores['abs_corr_01'][k] and rows[1 + k][4] == repr(float(scores['abs_corr_01'][k]))
        assert float(rows[1 + k][5]) == scores['mean_abs_offdiag'][k]
    pytest.importorskip('pandas')
    frame = cau.get_latent_corr({'expt_dir': root}, None, None, 3)          # read back: no model is needed
    assert 'loading results from' in capsys.readouterr().out
    assert list(frame.columns) == rows[0] and frame['N'].tolist() == [20, 2, 0, 38]
    assert np.array_equal(frame['AbsCorr01'].to_numpy(), scores['abs_corr_01'], equal_nan=True)          # the same bits
    assert np.array_equal(frame['MeanAbsCorr'].to_numpy(), scores['mean_abs_offdiag'], equal_nan=True)


# ------------------------------------------------------------------------------------------ the library's side
def test_plan_and_workspace_query_agree():
    lib = _hip.load()
    for n, D in ((1, 1), (255, 64), (256, 64), (257, 64), (70001, 16), (10 ** 6, 16), (10 ** 6, 64), (10 ** 6, 2),
                 (2 ** 31 - 1, 64), (4099, 33)):
        blocks, rows = _hip._segment_gram_plan(n, D)
        assert (blocks - 1) * rows < n <= blocks * rows
        for S in (0, 1, 4000):
            assert lib.bn_segment_gram_ws_bytes(n, S, D) == \
                (4 * (S + 1) + 15) // 16 * 16 + blocks * 2 * (D + 1) ** 2 * 8, (n, D, S)
        assert blocks * 2 * (D + 1) ** 2 * 8 <= 32 << 20
    assert _hip._segment_gram_plan(70001, 16) == (69, 1015) and _hip._segment_gram_plan(10 ** 6, 64)[0] == 496
    assert _hip._segment_gram_plan(0, 16) == (0, 1) and lib.bn_segment_gram_ws_bytes(0, 3, 16) == 16
    for n, S, D in ((-1, 1, 16), (10, -1, 16), (10, 1, 0), (10, 1, 65)):
        assert lib.bn_segment_gram_ws_bytes(n, S, D) == 0


def test_host_side_refusals_of_the_c_entry_point():
    """The checks that come before any launch run without a GPU: nothing is dereferenced."""
    lib = _hip.load()
    z, c, off, out, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    need = lib.bn_segment_gram_ws_bytes(10, 2, 3)

    def call(z=z, ld=3, c=c, off=off, S=2, D=3, n=10, out=out, ws=ws, nbytes=need):
        return lib.bn_segment_gram(z, ld, c, off, S, D, n, out, ws, nbytes, None)
    E_ARG, E_SHAPE = -1, -2
    assert call(D=0) == E_SHAPE and call(D=65, ld=65) == E_SHAPE and call(ld=2) == E_SHAPE
    assert call(n=-1) == E_SHAPE and call(S=-1) == E_SHAPE
    assert call(z=None) == E_ARG and call(off=None) == E_ARG and call(out=None) == E_ARG and call(ws=None) == E_ARG
    assert call(z=z + 2) == E_SHAPE and call(c=c + 1) == E_SHAPE and call(off=off + 4) == E_SHAPE
    assert call(out=out + 4) == E_SHAPE and call(ws=ws + 8) == E_SHAPE and call(nbytes=need - 1) == E_SHAPE
