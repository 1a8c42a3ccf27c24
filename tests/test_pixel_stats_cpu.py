"""Host logic of ``export_pixel_stats`` (a stub accumulator stands in for the device), ``summarise_pixel_stats``
against numpy and sklearn, the order-independence the GPU tests' tolerance rests on, and the host-side refusals of the
C entry point.  No GPU."""

import os
import pickle

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.fitting import eval as ev
from behavenet_amd.fitting import training
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from oracle import ref_cpu
from tests.golden_utils import base_hparams
from tests.pixel_stats_refs import pixel_sums
from tests.test_distributed_cpu import _free_port

DIM = [1, 32, 32]
SPLITS = ('train', 'val', 'test')
REAL_DEVICE_FN = ev.pixel_stats_device


def _two_sessions():
    """The two-session generator of tests/test_frame_errors_cpu.py, with gap trials."""
    sessions = [SyntheticSession(10, [4 + (t % 3) for t in range(10)], DIM, seed=20 + i,
                                 trial_splits='5;1;1;1', name=('lab', 'expt', 'animal', 's%d' % i))
                for i in range(2)]
    return SyntheticSessionsGenerator(sessions, device='cpu', placement='host')


class _StubModel(torch.nn.Module):
    """What export_pixel_stats touches when the accumulator is replaced: hparams, version, eval()."""

    def __init__(self, expt_dir, **hp):
        super().__init__()
        self.hparams = dict({'model_class': 'ae', 'model_type': 'conv', 'expt_dir': expt_dir}, **hp)
        self.version = 0


def _stub_sums(y, sess):
    """Integers that name the trial: its grey levels summed over the frames, its frame count, its session, and a one
    that counts the trials.  Integers below 2^53: float64 adds them exactly in any order."""
    y = y.detach().cpu()
    levels = y.double() if y.dtype == torch.uint8 else torch.round(y.double() * 255)
    out = torch.empty((4,) + tuple(y.shape[1:]), dtype=torch.float64)
    out[0] = levels.sum(dim=0)
    out[1] = y.shape[0]
    out[2] = float(sess or 0) + 1
    out[3] = 1
    return out


def _stub_device_fn(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200, out=None):
    add = _stub_sums(y, sess)
    if out is None:
        return add
    out += add
    return out


def _read(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def _expected(gen):
    """{(session, split): (sums, frames)} from a walk of our own over a generator in its initial state."""
    want = {}
    for dtype in SPLITS:
        gen.reset_iterators(dtype)
        for _ in range(gen.n_tot_batches[dtype]):
            data, sess = gen.next_batch(dtype)
            assert int(data['batch_idx']) in [int(t) for t in gen.datasets[sess].batch_idxs[dtype]]
            sums, frames = want.get((sess, dtype), (0, 0))
            want[(sess, dtype)] = (sums + _stub_sums(data['images'][0], sess).numpy(), frames + data['images'][0].shape[0])
    return want


def _check_pickles(files, gen):
    assert [os.path.basename(f) for f in files] == ['lab_expt_animal_s%d_pixel_stats.pkl' % i for i in range(2)]
    want = _expected(_two_sessions())
    for sess, path in enumerate(files):
        assert os.path.dirname(path).endswith('version_0')
        got = _read(path)
        assert sorted(got) == ['n_frames', 'stats', 'summary', 'trials']
        ds = gen.datasets[sess]
        assert set(got['trials']) == set(SPLITS)
        for k in SPLITS:
            assert np.array_equal(np.asarray(got['trials'][k]), np.asarray(ds.batch_idxs[k]))
        used = set(int(t) for k in SPLITS for t in ds.batch_idxs[k])
        assert 0 < len(used) < ds.n_trials == 10                       # (there ARE trials in no split)
        for k in SPLITS:
            sums, frames = want[(sess, k)]
            assert set(got['stats']) == set(got['n_frames']) == set(got['summary']) == set(SPLITS)
            assert got['stats'][k].dtype == np.float64 and got['stats'][k].shape == (4,) + tuple(DIM)
            assert type(got['n_frames'][k]) is int and got['n_frames'][k] == frames
            # each trial in its own split's accumulator and nowhere else, gap trials nowhere: exact
            assert np.array_equal(got['stats'][k], sums), (sess, k)
            assert np.all(got['stats'][k][1] == sum(4 + (int(t) % 3) for t in ds.batch_idxs[k]))
            assert np.all(got['stats'][k][3] == len(ds.batch_idxs[k])) and np.all(got['stats'][k][2] % (sess + 1) == 0)
            full = ev.summarise_pixel_stats(got['stats'][k], frames)
            # (the stub's sums are no statistics: r2 may be NaN, which assert_equal takes as equal to itself)
            np.testing.assert_equal(got['summary'][k], {'mse': full['mse'], 'r2': full['r2']})
            assert type(got['summary'][k]['mse']) is float and type(got['summary'][k]['r2']) is float


def test_exporter_schema_file_names_splits_and_gap_trials(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'pixel_stats_device', _stub_device_fn)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    gen = _two_sessions()
    files = ev.export_pixel_stats(gen, _StubModel(str(tmp_path)))
    _check_pickles(files, gen)
    # one file for all sessions when a name is given (as export_latents)
    one = os.path.join(str(tmp_path), 'named.pkl')
    assert ev.export_pixel_stats(_two_sessions(), _StubModel(str(tmp_path)), filename=one) == [one, one]
    for name in ('export_pixel_stats', 'pixel_stats', 'pixel_stats_device', 'summarise_pixel_stats'):
        assert name in ev.__all__


def test_an_empty_split_has_no_summary(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'pixel_stats_device', _stub_device_fn)
    sess = SyntheticSession(8, 5, DIM, seed=1, trial_splits='4;1;0;1', name=('lab', 'expt', 'animal', 's0'))
    gen = SyntheticSessionsGenerator([sess], device='cpu', placement='host')
    assert len(gen.datasets[0].batch_idxs['test']) == 0
    got = _read(ev.export_pixel_stats(gen, _StubModel(str(tmp_path)), filename=os.path.join(str(tmp_path), 'e.pkl'))[0])
    assert got['summary']['test'] is None and got['n_frames']['test'] == 0
    assert got['stats']['test'].shape == (4,) + tuple(DIM) and not got['stats']['test'].any()
    assert got['summary']['train'] is not None and got['n_frames']['train'] == 20 and got['n_frames']['val'] == 5


def test_exporter_raises_when_the_generator_ends_early(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'pixel_stats_device', _stub_device_fn)
    gen = _two_sessions()
    gen.n_tot_batches['val'] += 1
    with pytest.raises(RuntimeError, match='export_pixel_stats: the generator ended'):
        ev.export_pixel_stats(gen, _StubModel(str(tmp_path)), filename=os.path.join(str(tmp_path), 'x.pkl'))


def test_invalid_dtype_keys_are_value_errors_before_any_trial(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(ev, 'pixel_stats_device', lambda *a, **k: calls.append(a))
    out = os.path.join(str(tmp_path), 'x.pkl')
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        ev.export_pixel_stats(_two_sessions(), _StubModel(str(tmp_path), hip_decode_dtype='fp16'), filename=out)
    with pytest.raises(ValueError, match='hip_encode_dtype'):
        ev.export_pixel_stats(_two_sessions(), _StubModel(str(tmp_path), hip_encode_dtype='half'), filename=out)
    assert not os.path.exists(out) and not calls
    # ... and in the device function itself, before anything runs
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        REAL_DEVICE_FN(_StubModel(str(tmp_path), hip_decode_dtype='fp16'), torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError, match='hip_encode_dtype'):
        REAL_DEVICE_FN(_StubModel(str(tmp_path), hip_encode_dtype='half'), torch.zeros(2, 1, 4, 4))


def _export_worker(rank, world, port, tmp, out):
    os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'RANK': str(rank),
                       'WORLD_SIZE': str(world)})
    torch.set_num_threads(1)
    bdist.init_from_env(backend='gloo')
    ev.pixel_stats_device = _stub_device_fn
    gen = _two_sessions()
    torch.manual_seed(100 + rank)          # the ranks' generators are deliberately in DIFFERENT random states
    np.random.seed(100 + rank)
    os.makedirs(os.path.join(tmp, 'version_0'), exist_ok=True)
    out.put((rank, ev.export_pixel_stats(gen, _StubModel(tmp))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_write_what_one_process_writes(tmp_path, monkeypatch):
    tmp = str(tmp_path)
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_export_worker, args=(r, 2, port, tmp, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(out.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1] == [] and len(res[0]) == 2
    _check_pickles(res[0], _two_sessions())
    monkeypatch.setattr(ev, 'pixel_stats_device', _stub_device_fn)
    ref_dir = os.path.join(tmp, 'ref')
    os.makedirs(os.path.join(ref_dir, 'version_0'))
    want_files = ev.export_pixel_stats(_two_sessions(), _StubModel(ref_dir))
    for got_f, want_f in zip(res[0], want_files):
        got, want = _read(got_f), _read(want_f)
        assert got['n_frames'] == want['n_frames']
        np.testing.assert_equal(got['summary'], want['summary'])
        for k in SPLITS:
            assert got['stats'][k].dtype == want['stats'][k].dtype and np.array_equal(got['stats'][k], want['stats'][k])


# ------------------------------------------------------------------------------------------ summarise_pixel_stats
def _random_case(n=23, dim=(2, 5, 7), seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, size=(n,) + dim, dtype=np.uint8)
    x_hat = ((y.astype(np.float32) / np.float32(255)) * np.float32(0.8) +
             rng.random((n,) + dim, dtype=np.float32) * np.float32(0.2))
    return x_hat, y


def test_summary_against_numpy_and_sklearn():
    from sklearn.metrics import r2_score
    x_hat, y = _random_case()
    n = y.shape[0]
    acc = pixel_sums(x_hat, y)
    got = ev.summarise_pixel_stats(acc, n)
    assert sorted(got) == ['mean_map', 'mse', 'mse_map', 'r2', 'r2_map', 'var_map']
    t = (y.astype(np.float32) / np.float32(255)).astype(np.float64)
    xh = x_hat.astype(np.float64)
    rtol = 1e-12
    for k in ('mse_map', 'mean_map', 'var_map', 'r2_map'):
        assert got[k].dtype == np.float64 and got[k].shape == y.shape[1:]
    np.testing.assert_allclose(got['mean_map'], t.mean(axis=0), rtol=rtol, atol=0)
    # (the variance and the R^2 denominators are differences of sums: 1e-12 of the sums they are differences of)
    np.testing.assert_allclose(got['var_map'], t.var(axis=0), rtol=0, atol=rtol * float((t * t).mean(axis=0).max()))
    # (x_hat went through float32 terms in the yardstick, float64 ones here: 2^-23 relative)
    np.testing.assert_allclose(got['mse_map'], ((xh - t) ** 2).mean(axis=0), rtol=3e-7, atol=0)
    assert got['mse'] == pytest.approx(float(((xh - t) ** 2).mean()), rel=3e-7)
    # sklearn on the float32-term sums' own definition: feed it x_hat and t, compare at the float32 terms' accuracy,
    # and at 1e-12 against the same formulas evaluated from float64 terms throughout
    flat_t, flat_x = t.reshape(n, -1), xh.reshape(n, -1)
    raw = r2_score(flat_t, flat_x, multioutput='raw_values').reshape(y.shape[1:])
    weighted = r2_score(flat_t, flat_x, multioutput='variance_weighted')
    np.testing.assert_allclose(got['r2_map'], raw, rtol=0, atol=3e-7 * float(np.abs(1 - raw).max()))
    assert got['r2'] == pytest.approx(weighted, abs=3e-7 * abs(1 - weighted))
    acc64 = np.stack([((xh - t) ** 2).sum(axis=0), np.full(y.shape[1:], float(n)), t.sum(axis=0), (t * t).sum(axis=0)])
    got64 = ev.summarise_pixel_stats(acc64, n)
    np.testing.assert_allclose(got64['r2_map'], raw, rtol=rtol, atol=0)
    assert got64['r2'] == pytest.approx(weighted, rel=rtol)
    assert got64['mse'] == pytest.approx(float(((xh - t) ** 2).mean()), rel=rtol)
    np.testing.assert_allclose(got64['mse_map'], ((xh - t) ** 2).mean(axis=0), rtol=rtol, atol=0)


def test_zero_variance_pixel_is_nan_in_the_map_and_leaves_the_scalar_finite():
    x_hat, y = _random_case(seed=1)
    y[:, 1, 2, 3] = 77
    y[:, 0, 0, 0] = 0
    n = y.shape[0]
    got = ev.summarise_pixel_stats(pixel_sums(x_hat, y), n)
    nan = np.isnan(got['r2_map'])
    assert nan[1, 2, 3] and nan[0, 0, 0] and int(nan.sum()) == 2
    assert np.isfinite(got['r2']) and np.isfinite(got['mse'])
    assert got['var_map'][1, 2, 3] <= 1e-15 and got['var_map'][0, 0, 0] == 0
    assert got['mean_map'][1, 2, 3] == pytest.approx(float(np.float32(77) / np.float32(255)), rel=1e-12)
    # the scalar: every pixel's error over the pixels' variances (the constant ones have none to add)
    t = (y.astype(np.float32) / np.float32(255)).astype(np.float64)
    acc = pixel_sums(x_hat, y)
    denom = (n * t.var(axis=0)).sum()
    assert got['r2'] == pytest.approx(1 - acc[0].sum() / denom, rel=1e-12)
    with pytest.raises(ValueError, match='n_frames'):
        ev.summarise_pixel_stats(acc, 0)


def test_masked_summary_uses_the_mask_weights_and_the_full_denominator():
    x_hat, y = _random_case(seed=2)
    n = y.shape[0]
    rng = np.random.default_rng(5)
    mask = (rng.random(y.shape[1:]) > 0.3).astype(np.float32)
    mask[0, 0, 0] = 0                                               # a pixel the mask never lets in
    got = ev.summarise_pixel_stats(pixel_sums(x_hat, y, mask), n)
    t = (y.astype(np.float32) / np.float32(255)).astype(np.float64)
    on = mask > 0
    np.testing.assert_allclose(got['mean_map'][on], t.mean(axis=0)[on], rtol=1e-12, atol=0)
    assert np.isnan(got['mean_map'][0, 0, 0]) and np.isnan(got['var_map'][0, 0, 0]) and np.isnan(got['r2_map'][0, 0, 0])
    assert got['mse_map'][0, 0, 0] == 0
    # the reference's losses.mse: masked squared error over the FULL C H W, averaged over the frames
    want = np.mean([float(ref_cpu.mse(torch.from_numpy(x_hat[i]).double(), torch.from_numpy(t[i]),
                                      torch.from_numpy(mask).double())) for i in range(n)])
    assert got['mse'] == pytest.approx(want, rel=3e-7)


@pytest.mark.parametrize('n', [300, 4096])
def test_the_order_of_float64_additions_is_worth_far_less_than_the_tolerance(n):
    """What the GPU tests' rtol of 1e-12 rests on: left to right, in blocks and in numpy's order differ by less than
    N * 2^-53 relative on non-negative terms (3.3e-14 at the N = 300 the GPU tests go up to)."""
    rng = np.random.default_rng(n)
    terms = rng.random((n, 64), dtype=np.float32).astype(np.float64) ** 2
    ref = terms.sum(axis=0)
    left = np.zeros(64)
    for row in terms:
        left = left + row
    worst = float((np.abs(left - ref) / ref).max())
    for block in (11, 16, 200):
        parts = [np.add.reduce(terms[b:b + block][::-1], axis=0) for b in range(0, n, block)]
        blocked = np.zeros(64)
        for p in parts:
            blocked = blocked + p
        worst = max(worst, float((np.abs(blocked - ref) / ref).max()))
    assert worst <= n * 2.0 ** -53 < 1e-12


# ------------------------------------------------------------------------------------------ the C entry point, host side
def test_entry_point_reports_argument_errors_and_sizes_its_workspace_by_n_and_d():
    from behavenet_amd import _hip
    lib = _hip.load()
    assert lib.bn_pixel_stats_accum(None, None, 0, None, 0, None, 4, 16, None, 0, None) == -1
    # refusals come before anything touches the device: nothing here is a device pointer
    acc = np.full(4 * 64, 7.0)
    tgt = np.zeros(5 * 64, dtype=np.float32)
    a = acc.ctypes.data + (-acc.ctypes.data) % 16
    for n, d in [(0, 16), (-3, 16), (5, 0)]:
        assert lib.bn_pixel_stats_accum(None, tgt.ctypes.data, 0, None, 0, a, n, d, None, 0, None) == -2
    assert lib.bn_pixel_stats_accum(None, tgt.ctypes.data, 0, tgt.ctypes.data, 2, a, 5, 16, None, 0, None) == -2
    assert lib.bn_pixel_stats_accum(None, tgt.ctypes.data, 0, None, 0, a + 8, 5, 16, None, 0, None) == -2
    assert np.all(acc == 7.0)
    # the workspace: none while one frame block serves the call, else (blocks, 4, D) doubles; a function of (N, D)
    assert lib.bn_pixel_stats_ws_bytes(0, 16) == lib.bn_pixel_stats_ws_bytes(4, 0) == 0
    assert lib.bn_pixel_stats_ws_bytes(1, 35) == lib.bn_pixel_stats_ws_bytes(16, 3072) == 0
    for n, d in [(33, 35), (67, 780), (300, 3072), (256, 16384), (256, 61440)]:
        nbytes = lib.bn_pixel_stats_ws_bytes(n, d)
        assert nbytes > 0 and nbytes % (4 * d * 8) == 0 and 2 <= nbytes // (4 * d * 8) <= n
    # a 256-frame 128x128 trial covers the chip: 16 tiles of 1024 pixels times 16 frame blocks
    assert lib.bn_pixel_stats_ws_bytes(256, 16384) // (4 * 16384 * 8) * 16 >= 256


# ------------------------------------------------------------------------------------------ fit()
class _ListExp(object):
    version = 0

    def log(self, row):
        pass

    def save(self):
        pass


@pytest.mark.parametrize('key', [True, False, None])
def test_fit_calls_the_exporter_once_after_training_when_asked(tmp_path, monkeypatch, key):
    calls = []
    monkeypatch.setattr(ev, 'export_pixel_stats', lambda gen, model, filename=None: calls.append(('pixel', gen, model)))
    monkeypatch.setattr(ev, 'export_frame_errors', lambda gen, model, filename=None: calls.append(('frames', gen, model)))
    torch.set_num_threads(8)
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    hp = base_hparams(arch, 'ae', None)
    hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 1, 'min_n_epochs': 0, 'val_check_interval': 1,
               'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0, 'export_latents': False,
               'export_frame_errors': True, 'progress_bar': False})
    if key is not None:
        hp['export_pixel_stats'] = key
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(4, 8, dim, seed=0, trial_splits='2;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device='cpu', placement='host')
    torch.manual_seed(0)
    model = ref_cpu.AE(hp)
    model.save = lambda path: torch.save(model.state_dict(), path)
    model.version = 0
    best = training.fit(hp, model, gen, _ListExp(), method='ae', optimizer=ref_cpu.make_optimizer(model, hp))
    assert os.path.exists(os.path.join(str(tmp_path), 'version_0', 'best_val_model.pt'))     # training is over
    if key:
        assert [c[0] for c in calls] == ['frames', 'pixel'] and calls[1][1] is gen and calls[1][2] is best
    else:
        assert [c[0] for c in calls] == ['frames']
