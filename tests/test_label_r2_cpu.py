"""Label scores without a GPU ("label scores"): ``summarise_label_sums`` on the reference sums
against a two-pass float64 R^2, against sklearn on the float32 arrays as the reference calls it, its degenerate and
``n <= 10`` rules and the pooled scalar; the host paths of ``label_r2`` / ``export_label_r2`` / ``get_label_r2`` with
``_hip.segment_label_sums`` replaced by the numpy reference; the ``fit`` key; the entry points' refusals."""

import csv
import os

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting import eval as bn_eval
from behavenet_amd.fitting import training
from behavenet_amd.models.vaes import _r2_variance_weighted
from behavenet_amd.plotting import cond_ae_utils as cau
from tests import label_r2_refs as refs

E_ARG, E_SHAPE = -1, -2


# ------------------------------------------------------------------------------------------ summarise_label_sums
def _segments(name, lens, L, seed=0):
    n = sum(lens)
    pred, truth = refs.family(name, n, L, seed)
    offsets = np.concatenate(([0], np.cumsum(lens)))
    return pred, truth, offsets


def _two_pass(y, p):
    """(SStot, R^2, MSE) of one column in float64, SStot from the deviations about the mean."""
    y, p = y.astype(np.float64), p.astype(np.float64)
    ss_tot = float(np.sum((y - y.mean()) ** 2))
    ss_res = float(np.sum((y - p) ** 2))
    return ss_tot, 1 - ss_res / ss_tot, ss_res / len(y)


@pytest.mark.parametrize('name', refs.FAMILIES)
def test_summary_against_two_pass_float64(name):
    lens = [12, 250, 4099, 100000]
    L = 3
    pred, truth, offsets = _segments(name, lens, L)
    sums, _ = refs.sums_ref(pred, truth, None, offsets, L)
    got = bn_eval.summarise_label_sums(sums)
    assert sorted(got) == ['mse', 'n', 'pooled', 'r2'] and got['n'].dtype == np.int64
    assert got['r2'].shape == got['mse'].shape == got['n'].shape == (len(lens), L)
    for s in range(len(lens)):
        rows = slice(offsets[s], offsets[s + 1])
        for j in range(L):
            ss_tot, r2, mse = _two_pass(truth[rows, j], pred[rows, j])
            # the raw-moment SStot, recovered from the sums as summarise_label_sums forms it: 1e-9 relative (at
            # mean / std = 1000 the two sums it subtracts agree in their first six digits)
            n, sy, syy, sd = sums[s, j]
            assert abs((syy - sy * sy / n) - ss_tot) <= 1e-9 * ss_tot, (name, s, j)
            assert got['n'][s, j] == lens[s]
            # 1 - R^2 = SSres / SStot inherits SStot's relative error
            assert abs((1 - got['r2'][s, j]) - (1 - r2)) <= 1.1e-9 * abs(1 - r2), (name, s, j)
            assert abs(got['mse'][s, j] - mse) <= 1e-12 * mse, (name, s, j)


@pytest.mark.parametrize('name', refs.FAMILIES)
def test_summary_against_sklearn_on_float32(name):
    metrics = pytest.importorskip('sklearn.metrics')
    lens = [12, 20, 250, 4099, 100000]
    L = 2
    pred, truth, offsets = _segments(name, lens, L, seed=1)
    rng = np.random.default_rng(4)
    mask = (rng.random(truth.shape) < 0.8).astype(np.float32)
    sums, _ = refs.sums_ref(pred, truth, mask, offsets, L)
    got = bn_eval.summarise_label_sums(sums)
    for s in range(len(lens)):
        rows = slice(offsets[s], offsets[s + 1])
        for j in range(L):
            # the reference's lines: apply_masks, r2_score, np.mean(np.square(...)), all on float32
            y_true = truth[rows, j][mask[rows, j] == 1]
            y_pred = pred[rows, j][mask[rows, j] == 1]
            if len(y_true) <= 10:
                assert np.isnan(got['r2'][s, j]) and np.isnan(got['mse'][s, j])
                continue
            r2 = metrics.r2_score(y_true, y_pred, multioutput='variance_weighted')
            mse = np.mean(np.square(y_true - y_pred))
            assert abs(got['r2'][s, j] - r2) <= 1e-6 * max(1.0, abs(1 - r2)), (name, s, j, got['r2'][s, j], r2)
            assert abs(got['mse'][s, j] - mse) <= 1e-6 * mse, (name, s, j, got['mse'][s, j], mse)


def test_degenerate_rule_is_sklearns():
    y = np.full((40, 3), 317.25, dtype=np.float32)
    p = y.copy()
    p[:, 1] += 1.5          # constant labels, imperfect prediction
    y[:, 2] = p[:, 2] = np.linspace(0, 1, 40, dtype=np.float32)          # (not degenerate: a perfect prediction)
    sums, _ = refs.sums_ref(p, y, None, [0, 40], 3)
    got = bn_eval.summarise_label_sums(sums)
    assert got['r2'][0, 0] == 1.0 and got['r2'][0, 1] == 0.0 and got['r2'][0, 2] == 1.0
    assert got['mse'][0, 0] == 0.0 and got['mse'][0, 1] == 2.25
    metrics = pytest.importorskip('sklearn.metrics')
    for j in range(3):          # as the installed sklearn returns
        assert metrics.r2_score(y[:, j], p[:, j], multioutput='variance_weighted') == got['r2'][0, j]
    # a constant that its sums do not represent exactly (0.1f squared, 1000 times) is still a constant (sklearn's own
    # float32 mean is off there and its score with it; the float64 two-pass value is what is restated)
    y = np.full((1000, 2), 0.1, dtype=np.float32)
    p = y.copy()
    p[:, 1] = 0.3
    sums, _ = refs.sums_ref(p, y, None, [0, 1000], 2)
    got = bn_eval.summarise_label_sums(sums)
    assert got['r2'][0, 0] == 1.0 and got['r2'][0, 1] == 0.0
    assert _r2_variance_weighted(y[:, 1], p[:, 1]) == 0.0 and _r2_variance_weighted(y[:, 0], p[:, 0]) == 1.0


def test_ten_valid_entries_are_too_few_and_eleven_are_not():
    pred, truth = refs.family('mean 300 std 50', 21, 2)
    sums, _ = refs.sums_ref(pred, truth, None, [0, 10, 21, 21], 2)
    got = bn_eval.summarise_label_sums(sums)
    assert got['n'].tolist() == [[10, 10], [11, 11], [0, 0]]
    assert np.isnan(got['r2'][0]).all() and np.isnan(got['mse'][0]).all()
    assert np.isfinite(got['r2'][1]).all() and np.isfinite(got['mse'][1]).all()
    assert np.isnan(got['r2'][2]).all() and np.isnan(got['mse'][2]).all()
    # min_valid is the reference's 10 by default and can be lowered
    low = bn_eval.summarise_label_sums(sums, min_valid=9)
    assert np.isfinite(low['r2'][0]).all() and np.array_equal(low['r2'][1], got['r2'][1])
    # the pooled numbers take every valid entry
    assert got['pooled']['n'].tolist() == [21, 21]
    with pytest.raises(ValueError, match=r'\(S, L, 4\)'):
        bn_eval.summarise_label_sums(np.zeros((3, 4)))


@pytest.mark.parametrize('name', refs.FAMILIES)
def test_pooled_scalar_is_the_training_metric(name):
    lens = [12, 33, 250, 7]
    L = 4
    pred, truth, offsets = _segments(name, lens, L, seed=2)
    truth[:, 3] = truth[0, 3]                              # a constant label weighs nothing
    rng = np.random.default_rng(8)
    rows_ok = rng.random(truth.shape[0]) < 0.8             # whole rows: the masked arrays stay (n, L)
    mask = np.repeat(rows_ok[:, None], L, axis=1).astype(np.float32)
    sums, _ = refs.sums_ref(pred, truth, mask, offsets, L)
    pooled = bn_eval.summarise_label_sums(sums)['pooled']
    want = _r2_variance_weighted(truth[rows_ok], pred[rows_ok])
    assert abs((1 - pooled['r2_variance_weighted']) - (1 - want)) <= 1e-9 * abs(1 - want)
    assert pooled['r2'].shape == pooled['mse'].shape == (L,) and pooled['n'].tolist() == [int(rows_ok.sum())] * L
    for j in range(3):
        _, r2, mse = _two_pass(truth[rows_ok, j], pred[rows_ok, j])
        assert abs((1 - pooled['r2'][j]) - (1 - r2)) <= 1.1e-9 * abs(1 - r2) and abs(pooled['mse'][j] - mse) <= 1e-12 * mse
    assert pooled['r2'][3] == 0.0
    # every label constant: the plain mean of the degenerate scores, as there
    flat = np.full((20, 2), 2.0, dtype=np.float32)
    off = flat.copy()
    off[:, 1] = 3.0
    sums, _ = refs.sums_ref(off, flat, None, [0, 20], 2)
    assert bn_eval.summarise_label_sums(sums)['pooled']['r2_variance_weighted'] == _r2_variance_weighted(flat, off) == 0.5


def test_sums_ref_reads_its_offsets_as_the_kernel_does():
    pred, truth = refs.family('unit', 30, 1)
    sums, _ = refs.sums_ref(pred, truth, None, [-4, 10, 7, 12, 99], 1)
    assert sums[:, 0, 0].tolist() == [10, 0, 2, 18]
    assert refs.safe_offsets([5, 3, 40, 8], 30).tolist() == [5, 5, 30, 30]


# ------------------------------------------------------------------------------------------ the host paths
class _Model(torch.nn.Module):
    """A stand-in with a PS-VAE's interface on the CPU: 'latents' are pixel means through a fixed map.  As
    ``cond-ae-msp`` it has an AE-MSP's: ``encoding`` returns the plain latents, ``U`` (not idempotent) maps them to the
    transformed space, and ``get_transformed_latents`` applies ``U`` to whatever 2-d table it is given."""

    def __init__(self, model_class='ps-vae', n_labels=2, n_latents=5, root=None):
        super().__init__()
        self.hparams = {'model_class': model_class, 'n_labels': n_labels, 'n_ae_latents': n_latents, 'expt_dir': root}
        self.version = 0
        self.w = torch.nn.Parameter(torch.linspace(-1, 1, 16 * n_latents).view(16, n_latents))
        self.n_calls = 0
        self.U = torch.nn.Linear(n_latents, n_latents, bias=False)
        with torch.no_grad():
            self.U.weight.copy_(torch.linspace(-2, 3, n_latents * n_latents).view(n_latents, n_latents))

    def encoding(self, x, dataset=None):
        self.n_calls += 1
        z = x.float().reshape(x.shape[0], -1)[:, :16] @ self.w * (1 + (dataset or 0))
        n = self.hparams['n_labels']
        if self.hparams['model_class'] == 'cond-ae-msp':
            return z, None, None
        return z[:, :n], z[:, n:], None, None, None

    def get_transformed_latents(self, inputs, dataset=None, as_numpy=True):
        if inputs.dim() != 2:          # images: the reference's call
            out = self.encoding(inputs, dataset=dataset)
            inputs = out[0] if self.hparams['model_class'] == 'cond-ae-msp' else torch.cat(out[:2], dim=1)
        if self.hparams['model_class'] == 'cond-ae-msp':
            out = self.U(inputs)
        else:
            n = self.hparams['n_labels']
            out = torch.cat([3 * inputs[:, :n] + 1, inputs[:, n:]], dim=1)
        return out.detach().numpy() if as_numpy else out


LENS = [20, 33, 12, 27, 16, 40, 12, 25, 18]


def _generator(n_sessions=1, n_labels=2, masks=True):
    sessions = [SyntheticSession(len(LENS), LENS, (1, 4, 4), seed=3 + s, n_labels=n_labels, trial_splits='4;1;1;1',
                                 name=('lab', 'expt', 'animal', 'sess%d' % s)) for s in range(n_sessions)]
    rng = np.random.default_rng(9)
    for sess in sessions[:1] if masks else []:          # (the second session serves none)
        sess.labels_masks = [(rng.random(l.shape) < 0.8).astype(np.float32) for l in sess.labels]
    return refs.MaskedSessionsGenerator(sessions, device='cpu', placement='host')


@pytest.fixture
def host_sums(monkeypatch):
    calls = []

    def sums(pred, truth, mask, offsets):
        assert pred.shape == truth.shape and pred.dtype == truth.dtype == torch.float32
        calls.append((pred, truth, mask, np.asarray(offsets)))
        return torch.from_numpy(refs.sums_ref(pred.numpy(), truth.numpy(), None if mask is None else mask.numpy(),
                                              offsets, pred.shape[1])[0])
    monkeypatch.setattr(_hip, 'segment_label_sums', sums)
    return calls


def _per_trial(model, gen, sess, trial):
    """One trial's sums by the reference's route: ``get_transformed_latents(images)``, the session's own labels and
    masks."""
    ds = gen.datasets[sess]
    images = torch.from_numpy(ds.images_u8[trial].astype(np.float32) / 255)
    with torch.no_grad():
        pred = model.get_transformed_latents(images, dataset=sess)
    L = model.hparams['n_labels']
    masks = getattr(ds, 'labels_masks', None)
    return refs.sums_ref(pred[:, :L], ds.labels[trial], None if masks is None else masks[trial], [0, len(pred)], L)[0][0]


@pytest.mark.parametrize('model_class', ['ps-vae', 'cond-ae-msp'])
@pytest.mark.parametrize('dtype', ['val', 'test', ['train', 'val']])
def test_label_r2_walks_the_named_splits(host_sums, dtype, model_class):
    model, gen = _Model(model_class), _generator()
    ds = gen.datasets[0]
    got = bn_eval.label_r2(gen, model, dtype)
    kinds = [dtype] if isinstance(dtype, str) else dtype
    assert sorted(got['trial'].tolist()) == sorted(int(t) for k in kinds for t in ds.batch_idxs[k])
    assert got['session'].tolist() == [0] * len(got['trial'])
    assert model.n_calls == len(got['trial']) and len(host_sums) == 1          # other splits are not encoded; one launch
    pred, truth, mask, offsets = host_sums[0]
    assert pred.shape[1] == 2 and pred.stride(0) == 5 and mask is not None          # the first columns of the (n, D) table
    assert offsets.tolist() == np.concatenate(([0], np.cumsum([LENS[t] for t in got['trial']]))).tolist()
    if 'train' in kinds:          # the walk goes split by split
        n_train = len(ds.batch_idxs['train'])
        assert set(got['trial'][:n_train].tolist()) == set(int(t) for t in ds.batch_idxs['train'])
    for k, t in enumerate(got['trial']):
        assert np.array_equal(got['sums'][k], _per_trial(model, gen, 0, int(t)))
    assert sorted(got) == ['mse', 'n', 'pooled', 'r2', 'session', 'sums', 'trial']
    again = bn_eval.summarise_label_sums(got['sums'])
    for key in ('n', 'r2', 'mse'):
        assert np.array_equal(got[key], again[key], equal_nan=True)
    few = np.array([LENS[t] == 12 for t in got['trial']])
    if few.any():          # 12 frames under an 80 % mask: at most ten valid entries almost surely
        assert (got['n'][few] <= 12).all() and (got['sums'][few][..., 0] > 0).all()
    assert np.array_equal(np.isnan(got['r2']), got['n'] <= 10)


def test_label_r2_sessions_and_errors(host_sums):
    model, gen = _Model(), _generator(n_sessions=2)
    both = bn_eval.label_r2(gen, model, 'val')
    assert sorted(both['session'].tolist()) == [0, 1] and len(host_sums[-1]) == 4 and host_sums[-1][2] is not None
    for s in (0, 1):
        one = bn_eval.label_r2(gen, model, 'val', sess_idx=s)
        assert one['session'].tolist() == [s]
        k = both['session'].tolist().index(s)
        assert one['trial'][0] == both['trial'][k] and np.array_equal(one['sums'][0], both['sums'][k])
        assert np.array_equal(one['sums'][0], _per_trial(model, gen, s, int(one['trial'][0])))
    assert host_sums[-1][2] is None          # session 1 serves no masks: none is made up
    assert sorted(bn_eval.label_r2(gen, model, 'val', sess_idx=[1, 0])['session'].tolist()) == [0, 1]
    with pytest.raises(ValueError, match='sessions'):
        bn_eval.label_r2(gen, model, 'val', sess_idx=2)
    with pytest.raises(ValueError, match='dtype'):
        bn_eval.label_r2(gen, model, 'validation')
    with pytest.raises(ValueError, match='dtype'):
        bn_eval.label_r2(gen, model, [])
    for cls in ('ae', 'vae', 'beta-tcvae', 'cond-ae', 'cond-vae'):
        with pytest.raises(ValueError, match="'%s'" % cls):
            bn_eval.label_r2(gen, _Model(cls), 'val')
    for cls in ('msps-vae', 'cond-ae-msp'):
        bn_eval._check_label_r2_class('label_r2', cls)
    with pytest.raises(ValueError, match='labels'):
        bn_eval.label_r2(gen, _Model(n_labels=3), 'val')
    unlabelled = SyntheticSessionsGenerator([SyntheticSession(4, 12, (1, 4, 4), trial_splits='2;1;1;0')], device='cpu',
                                            placement='host')
    with pytest.raises(ValueError, match='serves no labels'):
        bn_eval.label_r2(unlabelled, model, 'val')


def test_export_label_r2_and_get_label_r2(host_sums, tmp_path, capsys):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'version_0'))
    model, gen = _Model(root=root), _generator(n_sessions=2)
    scores = bn_eval.label_r2(gen, model, ['train', 'val'])          # (trial 2, a training trial, has 12 frames)
    path = bn_eval.export_label_r2(gen, model, dtype=['train', 'val'])
    assert path == os.path.join(root, 'version_0', 'r2_supervised.csv')
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['Trial', 'Label', 'R2', 'MSE', 'Model', 'Session']
    assert len(rows) == 1 + 2 * len(scores['trial'])
    # (training trials come in a fresh random order on every walk: rows are matched by session and trial)
    at = {(int(sess), int(trial)): k for k, (sess, trial) in enumerate(zip(scores['session'], scores['trial']))}
    assert len(at) == len(scores['trial']) == (len(rows) - 1) // 2
    for r in range(len(at)):
        for i in range(2):
            row = rows[1 + 2 * r + i]
            k = at[(int(row[5]), int(row[0]))]
            assert row[0] == rows[1 + 2 * r][0] and row[1] == 'label_%d' % i and row[4] == 'MSPS-VAE'
            for cell, value in ((row[2], scores['r2'][k, i]), (row[3], scores['mse'][k, i])):
                assert (cell == '') if np.isnan(value) else (float(cell) == value)
    assert any(r[2] == '' for r in rows[1:]) and any(r[2] != '' for r in rows[1:])
    other = bn_eval.export_label_r2(gen, model, label_names=['x', 'y'], filename=os.path.join(root, 'mine.csv'))
    assert other == os.path.join(root, 'mine.csv')
    with open(other, newline='') as f:
        assert [r[1] for r in list(csv.reader(f))[1:3]] == ['x', 'y']
    with pytest.raises(ValueError, match='label names'):
        bn_eval.export_label_r2(gen, model, label_names=['x'])
    # the reference's signature, messages and frame
    pd = pytest.importorskip('pandas')
    os.remove(path)
    capsys.readouterr()
    hp = {'expt_dir': root}
    first = cau.get_label_r2(hp, model, gen, 0, ['x', 'y'])
    out = capsys.readouterr().out
    assert 'R^2 metrics do not exist; computing from scratch' in out and 'saving results to %s' % path in out
    assert list(first.columns) == ['Trial', 'Label', 'R2', 'MSE', 'Model', 'Session']
    val = bn_eval.label_r2(gen, model, 'val')
    assert first['Label'].tolist() == ['x', 'y'] * len(val['trial'])
    # (which session serves its trial first is drawn anew on every walk)
    by_session = first.sort_values(['Session', 'Label'], kind='stable')
    order = np.argsort(val['session'], kind='stable')
    assert by_session['Session'].tolist() == np.repeat(val['session'][order], 2).tolist()
    assert by_session['Trial'].tolist() == np.repeat(val['trial'][order], 2).tolist()
    assert np.array_equal(by_session['R2'].to_numpy(), val['r2'][order].reshape(-1), equal_nan=True)
    assert np.array_equal(by_session['MSE'].to_numpy(), val['mse'][order].reshape(-1), equal_nan=True)
    assert set(first['Model']) == {'MSPS-VAE'}
    calls = model.n_calls
    second = cau.get_label_r2(hp, None, None, 0, ['x', 'y'])          # read: neither model nor generator is touched
    assert 'loading results from %s' % path in capsys.readouterr().out
    pd.testing.assert_frame_equal(first, second)
    third = cau.get_label_r2(hp, model, gen, 0, ['x', 'y'], dtype='test', overwrite=True)
    assert 'overwriting metrics at %s' % path in capsys.readouterr().out and model.n_calls > calls
    assert sorted(third['Trial'].tolist()) == sorted(np.repeat(bn_eval.label_r2(gen, model, 'test')['trial'], 2).tolist())


# ------------------------------------------------------------------------------------------ fit()
class _ListExp(object):
    version = 0

    def log(self, row):
        raise AssertionError('an epoch ran')

    def save(self):
        pass


def test_fit_refuses_the_key_for_a_class_without_labels_before_the_first_epoch(tmp_path):
    from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
    from oracle import ref_cpu
    from tests.golden_utils import base_hparams
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    hp = base_hparams(arch, 'ae', None)
    hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 1, 'min_n_epochs': 0, 'val_check_interval': 1,
               'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0, 'export_latents': False,
               'export_label_r2': True, 'progress_bar': False})
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    gen = SyntheticSessionsGenerator([SyntheticSession(4, 8, dim, seed=0, trial_splits='2;1;1;0')], device='cpu',
                                     placement='host')
    torch.manual_seed(0)
    model = ref_cpu.AE(hp)
    model.version = 0
    served = []
    gen.next_batch = lambda *a, **k: served.append(a) or (None, None)
    with pytest.raises(ValueError, match="export_label_r2.*'ae'"):
        training.fit(hp, model, gen, _ListExp(), method='ae', optimizer=ref_cpu.make_optimizer(model, hp))
    assert not served and os.listdir(os.path.join(str(tmp_path), 'version_0')) == []


# ------------------------------------------------------------------------------------------ the entry points
def test_no_cpu_fallback_and_argument_checks():
    x = torch.zeros((4, 3))
    off = np.array([0, 4])
    with pytest.raises(ValueError, match='no CPU fallback'):
        bn_eval._hip.segment_label_sums(x, x, None, off)
    with pytest.raises(ValueError, match='float32'):
        _hip.segment_label_sums(x.double(), x, None, off)
    with pytest.raises(ValueError, match='expected a table'):
        _hip.segment_label_sums(x[0], x, None, off)


def test_the_symbols_and_the_partition():
    for name in ('bn_segment_label_sums', 'bn_segment_label_sums_ws_bytes'):
        assert name in _hip.SIGNATURES
    assert {'label_r2', 'export_label_r2', 'summarise_label_sums'} <= set(bn_eval.__all__)
    assert 'get_label_r2' in cau.__all__
    lib = _hip.load()
    q = lib.bn_segment_label_sums_ws_bytes
    assert q(5, 2, 0) == 0 and q(5, 2, 65) == 0 and q(5, -1, 4) == 0 and q(-1, 2, 4) == 0
    # the restated partition gives the library's workspace: S + 1 int32 offsets to a 16-byte boundary, then a head and
    # a tail slab of (L, 4) doubles per row block
    for n, S, L in [(0, 3, 4), (1, 1, 1), (5406, 8, 16), (70001, 1, 16), (10 ** 6, 4000, 16), (10 ** 6, 1, 64),
                    (2 ** 31 - 1, 7, 64), (2 ** 31 - 1, 10 ** 6, 1), (300, 0, 3)]:
        blocks, rows = _hip._segment_sums_plan(n, L)
        assert blocks <= _hip._SEGMENT_SUMS_TARGET_GROUPS and (blocks - 1) * rows < max(n, 1) <= max(blocks, 1) * rows
        assert q(n, S, L) == ((S + 1) * 4 + 15) // 16 * 16 + blocks * 2 * L * 4 * 8, (n, S, L)
    # the single long segment of the GPU test is cut into 69 row blocks with a ragged last one: SL_MIN_ELEMS / 16 =
    # 1024 rows at least a block -> ceil(70001 / 1024) = 69 blocks of ceil(70001 / 69) = 1015 rows, the last of 981
    assert _hip._segment_sums_plan(70001, 16) == (69, 1015) and 70001 - 68 * 1015 == 981
    p = 4096          # (a pointer that is never followed: every call below returns before a launch)
    big = 1 << 30
    call = lib.bn_segment_label_sums
    assert call(None, 4, p, 4, p, 4, p, 2, 4, 9, p, p, big, None) == E_ARG
    assert call(p, 4, None, 4, p, 4, p, 2, 4, 9, p, p, big, None) == E_ARG
    assert call(p, 4, p, 4, p, 4, None, 2, 4, 9, p, p, big, None) == E_ARG
    assert call(p, 4, p, 4, p, 4, p, 2, 4, 9, None, p, big, None) == E_ARG
    assert call(p, 4, p, 4, p, 4, p, 2, 4, 9, p, None, big, None) == E_ARG
    assert call(p, 4, p, 4, p, 4, p, 2, 0, 9, p, p, big, None) == E_SHAPE
    assert call(p, 65, p, 65, p, 65, p, 2, 65, 9, p, p, big, None) == E_SHAPE
    assert call(p, 3, p, 4, p, 4, p, 2, 4, 9, p, p, big, None) == E_SHAPE          # a leading dimension below L
    assert call(p, 4, p, 4, p, 3, p, 2, 4, 9, p, p, big, None) == E_SHAPE
    assert call(p, 4, p, 4, p, 4, p, 2, 4, 9, p, p, q(9, 2, 4) - 1, None) == E_SHAPE
    assert call(p + 2, 4, p, 4, p, 4, p, 2, 4, 9, p, p, big, None) == E_SHAPE
    assert call(p, 4, p, 4, p, 4, p + 4, 2, 4, 9, p, p, big, None) == E_SHAPE
    assert call(p, 4, p, 4, p, 4, p, 2, 4, 9, p, p + 8, big, None) == E_SHAPE
