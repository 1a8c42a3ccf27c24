"""The host half of the ranges ("ranges"), without a GPU:

* ``percentile_plan`` + ``percentile_lerp`` on ``np.sort`` against the installed ``np.nanpercentile``, exactly (NaN
  positions included): the sizes and percentiles the rule was restated on plus n = 1,000,003, where float32 virtual
  indices lie 0.06 apart and a wrong association of the arithmetic shows;
* ``compute_range``'s argument handling with the two device calls replaced by ``tests/ranges_refs``;
* ``get_input_range``'s errors; the partition ``_hip.column_select_plan`` restates against the library's workspace query.
"""

import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import ranges_refs as refs

E_ARG, E_SHAPE = -1, -2


def _table(n, seed):
    """Six columns: normal, 10 % NaN, heavy ties, all NaN, ties and NaN, wide dynamic range."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 6)).astype(np.float32)
    x[rng.random(n) < 0.1, 1] = np.nan
    x[:, 2] = rng.integers(0, 4, size=n).astype(np.float32)
    x[:, 3] = np.nan
    x[:, 4] = np.round(x[:, 4] * 2) / 2
    x[rng.random(n) < 0.3, 4] = np.nan
    x[:, 5] = np.exp(x[:, 5] * 10).astype(np.float32)
    return x


def _by_the_plan(x, ps):
    ranks, gammas = bn_eval.percentile_plan(refs.count_ref(x), ps)
    sel = refs.select_ref(x, ranks)
    return bn_eval.percentile_lerp(sel[0::2], sel[1::2], gammas)


@pytest.mark.parametrize('n', refs.SIZES + [1000003])
def test_plan_and_lerp_are_numpys_nanpercentile(n):
    x = _table(n, n)
    got = _by_the_plan(x, refs.PERCENTILES)
    assert got.dtype == np.float32 and got.shape == (len(refs.PERCENTILES), 6)
    for i, p in enumerate(refs.PERCENTILES):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)          # (the all-NaN column)
            want = np.nanpercentile(x, p, axis=0)
        assert want.dtype == np.float32
        assert np.array_equal(np.isnan(got[i]), np.isnan(want)), (n, p)
        ok = ~np.isnan(want)
        assert np.array_equal(got[i][ok], want[ok]), (n, p, got[i], want)
    assert np.isnan(got[:, 3]).all() and not np.isnan(got[:, [0, 1, 2, 5]]).any()


def test_plan_shapes_and_edges():
    ranks, gammas = bn_eval.percentile_plan([1, 0, 5], [0, 50, 100])
    assert ranks.dtype == np.int64 and ranks.shape == (6, 3) and gammas.dtype == np.float32 and gammas.shape == (3, 3)
    assert ranks[:, 0].tolist() == [0] * 6                           # a single valid value: every rank is 0
    assert ranks[:, 1].tolist() == [-1] * 6                          # none: NaN from the selection
    assert ranks[:, 2].tolist() == [0, 1, 2, 3, 4, 4]                # p = 100: both neighbours are the maximum
    assert gammas[:, 2].tolist() == [0.0, 0.0, 0.0]
    one, _ = bn_eval.percentile_plan(np.array([7]), 50)              # a scalar percentile
    assert one.tolist() == [[3], [4]]
    # two equal infinities interpolate to NaN, as numpy's lerp does
    inf = np.array([[np.inf]], dtype=np.float32)
    assert np.isnan(bn_eval.percentile_lerp(inf, inf, np.array([[0.25]], dtype=np.float32)))
    with np.errstate(invalid='ignore'):
        assert np.isnan(np.percentile(np.array([np.inf, np.inf], dtype=np.float32), 25))


# ------------------------------------------------------------------------------------------ compute_range
@pytest.fixture
def host_select(monkeypatch):
    """The two device calls answered by tests/ranges_refs on host tensors; -> the list of calls made."""
    calls = []

    def count(x):
        calls.append(('count', tuple(x.shape)))
        return torch.from_numpy(refs.count_ref(x.numpy()))

    def select(x, ranks):
        calls.append(('select', tuple(x.shape), tuple(ranks.shape)))
        return torch.from_numpy(refs.select_ref(x.numpy(), ranks.numpy()))
    monkeypatch.setattr(_hip, 'column_count', count)
    monkeypatch.setattr(_hip, 'column_select', select)
    monkeypatch.setattr(bn_eval, '_ranges_device', lambda: torch.device('cpu'))
    return calls


def _want(values, min_p=5, max_p=95):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return {'min': np.nanpercentile(values, min_p, axis=0), 'max': np.nanpercentile(values, max_p, axis=0),
                'med': np.nanpercentile(values, 50, axis=0)}


def _same(got, want):
    assert sorted(got) == ['max', 'med', 'min']
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])


def test_compute_range_arguments(host_select):
    rng = np.random.default_rng(0)
    trials = [rng.standard_normal((t, 5)).astype(np.float32) for t in (20, 100, 37, 64)]
    trials[1][::7, 2] = np.nan
    # a latents pickle: empty entries among the trials, of the pickle's own kinds
    listed = [trials[0], np.array([]), trials[1], np.empty((0, 5), dtype=np.float32), trials[2], trials[3]]
    _same(cau.compute_range(listed), _want(np.vstack(trials)))
    assert host_select == [('count', (221, 5)), ('select', (221, 5), (6, 5))]          # ONE count, ONE select, r = 6
    _same(cau.compute_range(listed, min_p=15, max_p=85), _want(np.vstack(trials), 15, 85))
    _same(bn_eval.compute_range(listed), _want(np.vstack(trials)))
    # tensors and arrays mixed; float64 entries are made float32
    mixed = [torch.from_numpy(trials[0]), trials[1].astype(np.float64), torch.from_numpy(trials[2]).double(), trials[3]]
    _same(cau.compute_range(mixed), _want(np.vstack(trials)))
    # a single row: every percentile is that row
    row = trials[0][:1]
    got = cau.compute_range([row])
    _same(got, _want(row))
    assert np.array_equal(got['min'], row[0]) and np.array_equal(got['max'], row[0])
    with pytest.raises(ValueError, match='no values'):
        cau.compute_range([np.array([]), np.empty((0, 5))])
    with pytest.raises(ValueError, match='expected entries'):
        cau.compute_range([trials[0], trials[1][:, :4]])
    with pytest.raises(ValueError, match='expected entries'):
        cau.compute_range([np.zeros(5, dtype=np.float32)])


class _Session(object):
    lab, expt, animal, session = 'lab', 'expt', 'animal', 'sess'

    def __init__(self, labels, masks=None, name='sess'):
        self.session = name
        self.labels, self.n_trials = labels, len(labels)
        if masks is not None:
            self.labels_masks = masks
        self.batch_idxs = {'train': np.array([0, 2]), 'val': np.array([3]), 'test': np.array([], dtype=int)}


class _Gen(object):
    def __init__(self, datasets):
        self.datasets = datasets


def test_get_input_range_labels_pickles_and_errors(host_select, tmp_path):
    rng = np.random.default_rng(1)
    labels = [[rng.standard_normal((t, 3)).astype(np.float32) for t in (9, 4, 12, 7)] for _ in range(2)]
    masks = [[(rng.random(l.shape) < 0.8).astype(np.float32) for l in sess] for sess in labels]
    gen = _Gen([_Session(labels[0], masks[0], 'a'), _Session(labels[1], None, 'b')])
    used = [0, 2, 3]          # trial 1 is in no split
    hp = {'expt_dir': str(tmp_path), 'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'a'}
    _same(cau.get_input_range('labels', hp, data_gen=gen), _want(np.vstack([labels[0][t] for t in used])))
    _same(cau.get_input_range('labels', hp, sess_idx=[1, 0], data_gen=gen, min_p=15, max_p=85),
          _want(np.vstack([labels[s][t] for s in (1, 0) for t in used]), 15, 85))
    masked = np.vstack([np.where(masks[0][t] == 0, np.nan, labels[0][t]) for t in used]).astype(np.float32)
    assert np.isnan(masked).any()
    _same(cau.get_input_range('labels', hp, data_gen=gen, apply_label_masks=True), _want(masked))
    assert not np.isnan(labels[0][0]).any()          # the generator's arrays are not written
    # a session without masks: said, then the plain labels
    _same(cau.get_input_range('labels', hp, sess_idx=1, data_gen=gen, apply_label_masks=True),
          _want(np.vstack([labels[1][t] for t in used])))
    with pytest.raises(ValueError, match='data_gen'):
        cau.get_input_range('labels', hp)
    with pytest.raises(ValueError, match='data_gen'):
        cau.get_input_range('labels_sc', hp, model=object())
    with pytest.raises(ValueError, match='labels_sc'):
        cau.get_input_range('labels_sc', hp, data_gen=gen)
    with pytest.raises(NotImplementedError):
        cau.get_input_range('neural', hp, data_gen=gen)
    # latents: from the pickle where it is there, named by hparams or by sess_ids
    os.makedirs(os.path.join(str(tmp_path), 'version_3'))
    lat = [labels[0][0], np.array([]), labels[0][2]]
    with open(os.path.join(str(tmp_path), 'version_3', 'lab_expt_animal_a_latents.pkl'), 'wb') as f:
        pickle.dump({'latents': lat, 'trials': None}, f)
    want = _want(np.vstack([lat[0], lat[2]]))
    _same(cau.get_input_range('latents', hp, sess_idx=None, version=3), want)
    ids = [{'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'a'}]
    _same(cau.get_input_range('latents', {'expt_dir': str(tmp_path)}, sess_ids=ids, sess_idx=0, version=3), want)
    _same(cau.get_input_range('latents', {'expt_dir': str(tmp_path)}, sess_ids=ids, sess_idx=[0, 0], version=3),
          _want(np.vstack([lat[0], lat[2]] * 2)))
    with pytest.raises(ValueError, match='model and data_gen'):
        cau.get_input_range('latents', hp, version=0)


def test_no_cpu_fallback():
    x = torch.zeros((4, 3))
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.column_count(x)
    with pytest.raises(ValueError, match='no CPU fallback'):
        _hip.column_select(x, np.zeros((1, 3), dtype=np.int64))
    with pytest.raises(ValueError, match='float32'):
        _hip.column_count(x.double())
    with pytest.raises(ValueError, match='expected a table'):
        _hip.column_count(x[0])


# ------------------------------------------------------------------------------------------ the entry points
def test_the_symbols_and_the_partition():
    for name in ('bn_column_count', 'bn_column_select_ws_bytes', 'bn_column_select'):
        assert name in _hip.SIGNATURES
    assert {'latent_ranges', 'latent_ranges_device', 'percentile_plan', 'percentile_lerp'} <= set(bn_eval.__all__)
    assert {'get_input_range', 'compute_range'} <= set(cau.__all__)
    lib = _hip.load()
    q = lib.bn_column_select_ws_bytes
    # the refusals of the query
    assert q(0, 4, 1) == 0 and q(5, 0, 1) == 0 and q(5, 1025, 1) == 0 and q(5, 4, 0) == 0 and q(5, 4, 9) == 0
    # the restated partition gives the library's workspace: two copies of the slots' state (8 + 4 bytes a slot, to
    # a 16-byte boundary) and (d r) histograms of 1 KiB per row block -- or the count pass's d counters per block
    for n, d, r in [(1, 1, 1), (4099, 65, 6), (4099, 16, 8), (32770, 4, 6), (10 ** 6, 16, 6), (2 * 10 ** 5, 64, 6),
                    (2 ** 31 - 1, 1024, 8), (70001, 1024, 1), (300, 3, 1)]:
        cols, col_groups, slabs, rows = _hip.column_select_plan(n, d, r)
        assert cols * r <= _hip.COLUMN_SELECT_HISTS and cols * col_groups >= d and (slabs - 1) * rows < n <= slabs * rows
        state = (d * r * 2 * 12 + 15) // 16 * 16
        count = _hip.column_select_plan(n, d, 0)[2] * d * 4
        assert q(n, d, r) == max(state + slabs * d * r * 1024, count), (n, d, r)
    p = 4096          # (a pointer that is never followed: every call below returns before a launch)
    assert lib.bn_column_count(None, 5, 4, 4, p, p, 1 << 20, None) == E_ARG
    assert lib.bn_column_count(p, 5, 4, 3, p, p, 1 << 20, None) == E_SHAPE
    assert lib.bn_column_count(p, 5, 4, 4, p, p, 3, None) == E_SHAPE
    assert lib.bn_column_select(p, 5, 4, 4, None, 2, p, p, 1 << 20, None) == E_ARG
    assert lib.bn_column_select(p, 5, 4, 4, p, 9, p, p, 1 << 20, None) == E_SHAPE
    assert lib.bn_column_select(p, 0, 4, 4, p, 2, p, p, 1 << 20, None) == E_SHAPE
    assert lib.bn_column_select(p, 5, 4, 4, p, 2, p, p, q(5, 4, 2) - 1, None) == E_SHAPE
    assert lib.bn_column_select(p + 2, 5, 4, 4, p, 2, p, p, 1 << 20, None) == E_SHAPE
