"""The helpers the table consumers of ``fitting.eval`` share: the gatherer of encoded trials (``_latent_trials``), the
table put together from its parts (``_parts_table``), the opening of the ARHMM stage (``_arhmm_stage``) and the csv
writer (``_write_csv``).  A fake generator serves host frames and a deterministic function of the frames stands in for
the encoder.  No GPU."""

import types

import numpy as np
import pytest
import torch

from behavenet_amd.fitting import eval as bn_eval

SPLITS = ('train', 'val', 'test')
# per session the frames of each trial and the trials of each split, in serving order: trial 3 of session 0 is in
# no split, trial 1 of session 1 has no frames
LENGTHS = ([5, 3, 7, 4, 6], [2, 0, 9, 4])
BATCH_IDXS = ({'train': [4, 0], 'val': [2], 'test': [1]}, {'train': [2, 1], 'val': [3], 'test': [0]})
N_LABELS = 2


class _Gen(object):
    """Two sessions of ragged trials, served one trial a batch with the sessions taking turns, session 1 first."""

    def __init__(self, labels=True):
        self.datasets = [types.SimpleNamespace(n_trials=len(n), batch_idxs=b,
                                               n_batches={k: len(v) for k, v in b.items()})
                         for n, b in zip(LENGTHS, BATCH_IDXS)]
        self.n_datasets = 2
        self.n_tot_batches = {dt: sum(len(b[dt]) for b in BATCH_IDXS) for dt in SPLITS}
        self.serve_uint8 = False
        self.labels = labels
        self.served, self.serving_uint8, self._queue = [], [], {}

    def reset_iterators(self, dtype):
        per_sess = [[(s, t) for t in BATCH_IDXS[s][dtype]] for s in (1, 0)]
        self._queue[dtype] = [per_sess[i % 2][i // 2] for i in range(2 * max(map(len, per_sess)))
                              if i // 2 < len(per_sess[i % 2])]

    def next_batch(self, dtype):
        if not self._queue[dtype]:
            return None, None
        sess, trial = self._queue[dtype].pop(0)
        self.served.append((sess, trial))
        self.serving_uint8.append(self.serve_uint8)
        data = {'images': [_frames(sess, trial)], 'batch_idx': torch.tensor(trial)}
        if self.labels:
            data['labels'] = [_frames(sess, trial).flatten(1)[:, :N_LABELS].numpy()]
        return data, sess


def _frames(sess, trial):
    n = LENGTHS[sess][trial]
    return (torch.arange(n * 8, dtype=torch.float32).reshape(n, 1, 2, 4) + 100.0 * trial + 1000.0 * sess) / 4096.0


def _latents(sess, trial):
    """What the stand-in encoder makes of a trial, as fp32."""
    y = _frames(sess, trial)
    return (y.flatten(1)[:, ::2] * (sess + 1)).to(torch.float32)


class _Model(torch.nn.Module):
    def __init__(self, **hp):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.hparams = dict({'model_class': 'ae', 'model_type': 'conv', 'n_ae_latents': 4}, **hp)
        self.version = 0


@pytest.fixture
def encoder(monkeypatch):
    """``encode_trial`` replaced by a deterministic function of the frames -> the list of its calls."""
    calls = []

    def encode_trial(model, y, sess=None, labels_2d=None, chunk_size=200):
        calls.append((sess, int(y.shape[0])))
        # float64 and not contiguous: the gatherer has to make contiguous fp32 of it
        return (y.flatten(1).double().numpy() * (sess + 1))[:, ::2]

    class NoDeviceTrials(object):
        def __init__(self, model):
            pass

        def __call__(self, *args):
            raise AssertionError('host frames go through encode_trial')
    monkeypatch.setattr(bn_eval, 'encode_trial', encode_trial)
    monkeypatch.setattr(bn_eval, '_GraphedTrialEncoder', NoDeviceTrials)
    return calls


WALK = [(1, 2), (0, 4), (1, 1), (0, 0), (1, 3), (0, 2), (1, 0), (0, 1)]          # split after split, sessions in turn


# ------------------------------------------------------------------------------------------ the gatherer
def test_keys_walk_order_and_host_results(encoder):
    gen, model = _Gen(), _Model()
    parts = bn_eval._latent_trials('t', gen, model, SPLITS, {0, 1})
    assert gen.served == WALK
    assert list(parts) == [k for k in WALK if k != (1, 1)]          # the trial without frames is dropped
    assert (0, 3) not in parts                                         # in no split: never served
    for (sess, trial), z in parts.items():
        assert z.dtype == torch.float32 and z.is_contiguous() and z.device == model.w.device
        assert z.shape == (LENGTHS[sess][trial], 4) and torch.equal(z, _latents(sess, trial))
    assert all(type(k[1]) is int for k in parts)
    # left on the host for a caller that uploads once (latent_ranges): the arrays as ``encode_trial`` returned them
    raw = bn_eval._latent_trials('t', _Gen(), model, SPLITS, {0, 1}, upload=False)
    assert list(raw) == list(parts)
    for key, z in raw.items():
        assert isinstance(z, np.ndarray) and z.dtype == np.float64 and np.array_equal(z, _latents(*key).numpy())
    assert all(gen.serving_uint8) and gen.serve_uint8 is False          # a conv model: stored frames, then as it was


def test_unwanted_sessions_and_other_splits_are_not_encoded(encoder):
    gen = _Gen()
    parts = bn_eval._latent_trials('t', gen, _Model(), ['val', 'train'], {1})
    assert gen.served == [(1, 3), (0, 2), (1, 2), (0, 4), (1, 1), (0, 0)]          # no test trial is read
    assert encoder == [(1, 4), (1, 9), (1, 0)]                                       # session 0 is served, not encoded
    assert list(parts) == [(1, 3), (1, 2)]


def test_the_zero_row_filter_on_and_off(encoder):
    kept = bn_eval._latent_trials('t', _Gen(), _Model(), SPLITS, {0, 1}, keep_empty=True)
    assert list(kept) == WALK and kept[(1, 1)].shape == (0, 4) and kept[(1, 1)].dtype == torch.float32
    assert (1, 1) not in bn_eval._latent_trials('t', _Gen(), _Model(), SPLITS, {0, 1}, keep_empty=False)


def test_per_trial_sees_every_kept_trial_once_and_its_error_stops_the_walk(encoder):
    gen, seen = _Gen(), []

    def per_trial(sess, trial, z, data):
        assert torch.equal(z, _latents(sess, trial)) and int(data['batch_idx']) == trial and 'labels' in data
        seen.append((sess, trial))
    parts = bn_eval._latent_trials('t', gen, _Model(), SPLITS, {0, 1}, per_trial=per_trial)
    assert seen == list(parts) == [k for k in WALK if k != (1, 1)]
    seen_all = []
    bn_eval._latent_trials('t', _Gen(), _Model(), SPLITS, {0}, per_trial=lambda s, t, z, d: seen_all.append((s, t)),
                           keep_empty=True)
    assert seen_all == [k for k in WALK if k[0] == 0]

    gen, seen = _Gen(), []

    def failing(sess, trial, z, data):
        seen.append((sess, trial))
        if (sess, trial) == (0, 0):
            raise ValueError('trial (0, 0) is refused')
    del encoder[:]
    with pytest.raises(ValueError, match=r'trial \(0, 0\) is refused'):
        bn_eval._latent_trials('t', gen, _Model(), SPLITS, {0, 1}, per_trial=failing)
    assert seen == [(1, 2), (0, 4), (0, 0)] and gen.served == WALK[:4] and len(encoder) == 4
    assert gen.serve_uint8 is False and all(gen.serving_uint8)          # restored after the exception


def test_label_r2_raises_during_the_walk(encoder):
    gen = _Gen(labels=False)
    model = _Model(model_class='cond-ae-msp', n_labels=N_LABELS)
    with pytest.raises(ValueError, match=r'label_r2: the generator serves no labels \(session 1, trial 2\)'):
        bn_eval.label_r2(gen, model, dtype=['train', 'val'])
    assert gen.served == WALK[:1] and gen.serve_uint8 is False


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('dtypes', (['train'], ['val', 'train']))
def test_table_rows_are_in_the_references_order(encoder, dtypes):
    gen = _Gen()
    parts = bn_eval._latent_trials('t', gen, _Model(), SPLITS, {0, 1})
    idxs = [ds.batch_idxs for ds in gen.datasets]
    for wanted in ({0, 1}, {1}):
        order = [k for k in bn_eval._corr_trial_order(idxs, dtypes, wanted) if k != (1, 1)]
        whole = torch.cat([_latents(*k) for k in order], dim=0)
        keys, table = bn_eval._parts_table(parts, gen, dtypes, wanted, (1, 3))
        assert keys == order and torch.equal(table, whole[:, 1:3])
        assert not table.is_contiguous()          # a range is read in place
        keys, table = bn_eval._parts_table(parts, gen, dtypes, wanted, np.asarray([3, 0, 2], dtype=np.int64))
        assert keys == order and torch.equal(table, whole[:, [3, 0, 2]])
    assert [k[0] for k in bn_eval._parts_table(parts, gen, ['val', 'train'], {0, 1}, (0, 4))[0]] == [0, 0, 0, 1, 1]
    assert bn_eval._parts_table({}, gen, dtypes, {0, 1}, (0, 4)) == ([], None)


# ------------------------------------------------------------------------------------------ the ARHMM stage
def test_arhmm_stage_refuses_bad_arguments_before_any_trial_is_read(encoder):
    gen = _Gen()
    with pytest.raises(ValueError, match='hip_encode_dtype'):
        bn_eval.fit_arhmm(gen, _Model(hip_encode_dtype='half'), 2)
    with pytest.raises(ValueError, match="fit_arhmm: data_key must be 'ae_latents' or 'labels', got 'pixels'"):
        bn_eval.fit_arhmm(gen, _Model(), 2, data_key='pixels')
    with pytest.raises(ValueError, match='fit_arhmm: sessions \\[2\\] of a generator with 2'):
        bn_eval.fit_arhmm(gen, _Model(), 2, sess_idx=2)
    with pytest.raises(ValueError, match='arhmm_predictions: dtype must be'):
        bn_eval.arhmm_predictions(gen, _Model(), None, dtype='all')
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        bn_eval.arhmm_predictions(gen, _Model(hip_decode_dtype='fp16'), None)
    with pytest.raises(ValueError, match="arhmm_predictions: data_key must be 'ae_latents' or 'labels', got 'pixels'"):
        bn_eval.arhmm_predictions(gen, _Model(), None, data_key='pixels')
    assert gen.served == [] and encoder == []


@pytest.mark.parametrize('data_key', ('ae_latents', 'labels'))
def test_arhmm_stage_tables(encoder, data_key):
    want = (lambda s, t: _latents(s, t)) if data_key == 'ae_latents' else \
        (lambda s, t: _frames(s, t).flatten(1)[:, :N_LABELS])
    model = _Model()
    idxs = [dict(b) for b in BATCH_IDXS]

    def check(split, order):
        table, offsets, sessions, trials = split
        order = [k for k in order if k in kept]
        assert list(zip(sessions.tolist(), trials.tolist())) == order
        assert offsets.tolist() == np.concatenate(([0], np.cumsum([LENGTHS[s][t] for s, t in order]))).tolist()
        assert table.is_contiguous() and torch.equal(table, torch.cat([want(*k) for k in order], dim=0))

    wanted, parts, splits = bn_eval._arhmm_stage('t', _Gen(), model, data_key, SPLITS, None, True)
    # (the labels of a trial without frames are kept, its latents are not)
    kept = set(WALK) - ({(1, 1)} if data_key == 'ae_latents' else set())
    assert wanted == {0, 1} and list(splits) == list(SPLITS) and set(parts) == kept
    for dt in SPLITS:
        check(splits[dt], bn_eval._corr_trial_order(idxs, [dt], wanted))
    wanted, _, split = bn_eval._arhmm_stage('t', _Gen(), model, data_key, ['test', 'train'], [1], False)
    assert wanted == {1}
    check(split, [(1, 0), (1, 2), (1, 1)])
    # the states exporters' form: every session, sorted, and trials gathered already are taken as they are
    gen = _Gen()
    wanted, parts, split = bn_eval._arhmm_stage('t', gen, model, data_key, SPLITS, 'unread', False, every=True)
    assert wanted == {0, 1}
    check(split, sorted(WALK))
    del gen.served[:]
    again = bn_eval._arhmm_stage('t', gen, model, data_key, SPLITS, None, False, every=True, parts=parts)
    assert again[1] is parts and gen.served == [] and torch.equal(again[2][0], split[0])
    # a split without frames: no table
    empty = bn_eval._arhmm_split({(1, 1): torch.zeros(0, 4)}, [(1, 1)])
    assert empty[0] is None and empty[1].tolist() == [0, 0]


def test_the_data_key_of_a_model_class_and_the_version_path():
    assert [bn_eval._arhmm_data_key({'model_class': c}) for c in ('arhmm', 'hmm', 'arhmm-labels', 'hmm-labels')] == \
        ['ae_latents', 'ae_latents', 'labels', 'labels']
    assert bn_eval._arhmm_data_key({}) == 'ae_latents'
    model = types.SimpleNamespace(hparams={'expt_dir': '/e', 'version': 9}, version=3)
    assert bn_eval._version_path(model, 'a.csv') == '/e/version_3/a.csv'
    assert bn_eval._version_path({'expt_dir': '/e', 'version': 7}, 'arhmm_grid', 'model_001') == \
        '/e/version_7/arhmm_grid/model_001'
    assert bn_eval._grid_model_dir({'expt_dir': '/e', 'version': 7}, 1) == '/e/version_7/arhmm_grid/model_001'
    ds = types.SimpleNamespace(lab='l', expt='x', animal='a', session='s')
    assert bn_eval._session_filename(model, ds, None, 'latents.pkl') == '/e/version_3/l_x_a_s_latents.pkl'
    hparams = {'expt_dir': '/e', 'version': 7}
    assert bn_eval._session_filename(hparams, ds, None, 'states.pkl', 'arhmm_grid', 'model_000') \
        == '/e/version_7/arhmm_grid/model_000/l_x_a_s_states.pkl'
    assert bn_eval._session_filename(model, ds, 'named.pkl', 'latents.pkl') == 'named.pkl'


# ------------------------------------------------------------------------------------------ csv
NAN = float('nan')
LABEL_SCORES = {'session': np.asarray([0, 1]), 'trial': np.asarray([3, 0]),
                'r2': np.asarray([[0.5, NAN], [-1.25, 1.0 / 3.0]]),
                'mse': np.asarray([[NAN, 2.0], [1e-7, 0.1]], dtype=np.float32)}
CORR_SCORES = {'rows': np.asarray([[0, 20], [20, 22], [22, 60]]), 'n': np.asarray([20, 2, 38]),
               'abs_corr_01': np.asarray([0.1, NAN, 1.0]), 'mean_abs_offdiag': np.asarray([1.0 / 3.0, NAN, 2e-17])}
_MEASURES = {'mse': [[0.5, NAN], [1e22, 0.30000000000000004]], 'r2': [[1.0 / 3.0, NAN], [-0.0, 1.0]],
             'mse_persistence': [[1.25, 2.5], [NAN, 5e-324]], 'r2_persistence': [[NAN, NAN], [0.75, -7.0]]}
PREDICTION_SCORES = dict({'session': np.asarray([0, 1]), 'trial': np.asarray([7, 3]),
                          'n': np.asarray([[20, 5], [18, 11]])}, **{k: np.asarray(v) for k, v in _MEASURES.items()})
FORECAST_SCORES = dict({'session': np.asarray([0, 1]), 'trial': np.asarray([7, 3]),
                        'n': np.asarray([[[20, 5], [18, 11]], [[19, 4], [17, 10]]])},
                       **{k: np.stack([np.asarray(v), 2.0 * np.asarray(v)]) for k, v in _MEASURES.items()})

# what the four writers wrote before they shared ``_write_csv``, recorded from them
LABEL_CSV = (b'Trial,Label,R2,MSE,Model,Session\n3,"paw, left",0.5,,MSPS-VAE,0\n3,nose,,2.0,MSPS-VAE,0\n'
             b'0,"paw, left",-1.25,1.0000000116860974e-07,MSPS-VAE,1\n'
             b'0,nose,0.3333333333333333,0.10000000149011612,MSPS-VAE,1\n')
CORR_CSV = (b'Segment,RowBegin,RowEnd,N,AbsCorr01,MeanAbsCorr\n0,0,20,20,0.1,0.3333333333333333\n1,20,22,2,,\n'
            b'2,22,60,38,1.0,2e-17\n')
PREDICTION_CSV = (b'Session,Trial,Dim,N,MSE,R2,MSE_persistence,R2_persistence\n0,7,0,20,0.5,0.3333333333333333,1.25,\n'
                  b'0,7,1,5,,,2.5,\n1,3,0,18,1e+22,-0.0,,0.75\n1,3,1,11,0.30000000000000004,1.0,5e-324,-7.0\n')
FORECAST_CSV = (b'Horizon,Session,Trial,Dim,N,MSE,R2,MSE_persistence,R2_persistence\n'
                b'1,0,7,0,20,0.5,0.3333333333333333,1.25,\n1,0,7,1,5,,,2.5,\n1,1,3,0,18,1e+22,-0.0,,0.75\n'
                b'1,1,3,1,11,0.30000000000000004,1.0,5e-324,-7.0\n2,0,7,0,19,1.0,0.6666666666666666,2.5,\n'
                b'2,0,7,1,4,,,5.0,\n2,1,3,0,17,2e+22,-0.0,,1.5\n2,1,3,1,10,0.6000000000000001,2.0,1e-323,-14.0\n')


def _written(tmp_path, monkeypatch):
    monkeypatch.setattr(bn_eval, 'label_r2', lambda *args, **kwargs: LABEL_SCORES)
    monkeypatch.setattr(bn_eval, 'arhmm_predictions', lambda *args, **kwargs: PREDICTION_SCORES)
    paths = [str(tmp_path / name) for name in ('r2.csv', 'corr.csv', 'pred.csv', 'fore.csv')]
    assert bn_eval.export_label_r2(None, None, label_names=['paw, left', 'nose'], filename=paths[0]) == paths[0]
    assert bn_eval._write_latent_corr_csv(paths[1], CORR_SCORES) == paths[1]
    assert bn_eval.export_arhmm_predictions({}, None, None, filename=paths[2]) == paths[2]
    assert bn_eval.write_forecasts_csv(paths[3], FORECAST_SCORES) is None
    out = []
    for path in paths:
        with open(path, 'rb') as f:
            out.append(f.read())
    return out


def test_the_four_csv_files_byte_for_byte(tmp_path, monkeypatch):
    got = _written(tmp_path, monkeypatch)
    assert got == [LABEL_CSV, CORR_CSV, PREDICTION_CSV, FORECAST_CSV]


def test_write_csv_fields(tmp_path):
    path = str(tmp_path / 't.csv')
    rows = ([1, 'a,b', NAN, 0.1, np.float32(0.1), np.float64(NAN), np.int64(3)], [2, '', -0.0, 1e22, 5e-324, 1.0, 0])
    assert bn_eval._write_csv(path, ['A', 'B', 'C', 'D', 'E', 'F', 'G'], iter(rows)) == path
    with open(path, 'rb') as f:
        assert f.read() == (b'A,B,C,D,E,F,G\n1,"a,b",,0.1,0.10000000149011612,,3\n'
                            b'2,,-0.0,1e+22,5e-324,1.0,0\n')
