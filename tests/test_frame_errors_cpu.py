"""Host logic of ``export_frame_errors`` (a stub scorer stands in for the device) and the float64 yardstick of the GPU
tests.  No GPU."""

import os
import pickle

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.fitting import eval as ev
from oracle import ref_cpu
from tests.frame_error_refs import per_frame_mse
from tests.test_distributed_cpu import _free_port
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator

DIM = [1, 32, 32]
REAL_SCORER = ev.frame_errors_device


def _two_sessions():
    """The two-session generator of tests/test_distributed_fit_cpu.py, with gap trials."""
    sessions = [SyntheticSession(10, [4 + (t % 3) for t in range(10)], DIM, seed=20 + i,
                                 trial_splits='5;1;1;1', name=('lab', 'expt', 'animal', 's%d' % i))
                for i in range(2)]
    return SyntheticSessionsGenerator(sessions, device='cpu', placement='host')


class _StubModel(torch.nn.Module):
    """What export_frame_errors touches when the scorer is replaced: hparams, version, eval()."""

    def __init__(self, expt_dir, **hp):
        super().__init__()
        self.hparams = dict({'model_class': 'ae', 'model_type': 'conv', 'expt_dir': expt_dir}, **hp)
        self.version = 0


def _stub_scorer(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200):
    """One float per frame that names the frame: its mean grey value plus the session."""
    return y.reshape(y.shape[0], -1).float().mean(dim=1) + float(sess or 0)


def _read(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def _check_pickles(files, gen):
    assert [os.path.basename(f) for f in files] == ['lab_expt_animal_s%d_frame_errors.pkl' % i for i in range(2)]
    for sess, path in enumerate(files):
        assert os.path.dirname(path).endswith('version_0')
        got = _read(path)
        assert sorted(got) == ['mse', 'trials']
        ds = gen.datasets[sess]
        assert set(got['trials']) == {'train', 'val', 'test'}
        for k in got['trials']:
            assert np.array_equal(np.asarray(got['trials'][k]), np.asarray(ds.batch_idxs[k]))
        used = set(int(t) for k in ('train', 'val', 'test') for t in ds.batch_idxs[k])
        assert len(got['mse']) == ds.n_trials == 10 and 0 < len(used) < 10
        for i, arr in enumerate(got['mse']):
            if i not in used:
                assert arr.size == 0
                continue
            assert arr.dtype == np.float32 and arr.shape == (4 + (i % 3),)


def test_exporter_schema_file_names_and_gap_trials(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'frame_errors_device', _stub_scorer)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    gen = _two_sessions()
    files = ev.export_frame_errors(gen, _StubModel(str(tmp_path)))
    _check_pickles(files, gen)
    # the values are the scorer's, trial by trial
    gen2 = _two_sessions()
    for sess in range(2):
        got = _read(files[sess])['mse']
        for dtype in ('train', 'val', 'test'):
            gen2.reset_iterators(dtype)
        for dtype in ('train', 'val', 'test'):
            for _ in range(gen2.n_tot_batches[dtype]):
                data, s_ = gen2.next_batch(dtype)
                if s_ != sess:
                    continue
                want = _stub_scorer(None, data['images'][0], s_).numpy()
                assert np.array_equal(got[int(data['batch_idx'])], want)
    # one file for all sessions when a name is given (as export_latents)
    one = os.path.join(str(tmp_path), 'named.pkl')
    assert ev.export_frame_errors(_two_sessions(), _StubModel(str(tmp_path)), filename=one) == [one, one]
    assert 'export_frame_errors' in ev.__all__ and 'frame_errors_device' in ev.__all__


def test_exporter_raises_when_the_generator_ends_early(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'frame_errors_device', _stub_scorer)
    gen = _two_sessions()
    gen.n_tot_batches['val'] += 1
    with pytest.raises(RuntimeError, match='export_frame_errors: the generator ended'):
        ev.export_frame_errors(gen, _StubModel(str(tmp_path)), filename=os.path.join(str(tmp_path), 'x.pkl'))


def test_invalid_dtype_keys_are_still_value_errors(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'frame_errors_device', _stub_scorer)
    out = os.path.join(str(tmp_path), 'x.pkl')
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        ev.export_frame_errors(_two_sessions(), _StubModel(str(tmp_path), hip_decode_dtype='fp16'), filename=out)
    with pytest.raises(ValueError, match='hip_encode_dtype'):
        ev.export_frame_errors(_two_sessions(), _StubModel(str(tmp_path), hip_encode_dtype='half'), filename=out)
    assert not os.path.exists(out)
    # ... and in the scorer itself, before anything runs
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        REAL_SCORER(_StubModel(str(tmp_path), hip_decode_dtype='fp16'), torch.zeros(2, 1, 4, 4))


def _export_worker(rank, world, port, tmp, out):
    os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'RANK': str(rank),
                       'WORLD_SIZE': str(world)})
    torch.set_num_threads(1)
    bdist.init_from_env(backend='gloo')
    ev.frame_errors_device = _stub_scorer
    gen = _two_sessions()
    torch.manual_seed(100 + rank)          # the ranks' generators are deliberately in DIFFERENT random states
    np.random.seed(100 + rank)
    os.makedirs(os.path.join(tmp, 'version_0'), exist_ok=True)
    out.put((rank, ev.export_frame_errors(gen, _StubModel(tmp))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_every_trial_once_on_rank_0(tmp_path, monkeypatch):
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
    monkeypatch.setattr(ev, 'frame_errors_device', _stub_scorer)
    ref_dir = os.path.join(tmp, 'ref')
    os.makedirs(os.path.join(ref_dir, 'version_0'))
    want_files = ev.export_frame_errors(_two_sessions(), _StubModel(ref_dir))
    for got_f, want_f in zip(res[0], want_files):
        for a, b in zip(_read(got_f)['mse'], _read(want_f)['mse']):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('masked', ['none', 'trial', 'frame'])
def test_float64_yardstick_is_the_oracle_mse_frame_by_frame(u8, masked):
    g = torch.Generator().manual_seed(3)
    n, dim = 5, (2, 7, 5)
    x_hat = torch.rand((n,) + dim, generator=g)
    tu = torch.randint(0, 256, (n,) + dim, generator=g, dtype=torch.uint8)
    target = tu if u8 else tu.float() / 255
    mask = {'none': None, 'trial': (torch.rand(dim, generator=g) > 0.3).float(),
            'frame': (torch.rand((n,) + dim, generator=g) > 0.3).float()}[masked]
    got = per_frame_mse(x_hat, target, mask, torch.float64)
    assert got.dtype == torch.float64 and got.shape == (n,)
    tf = (tu.float() / 255).double()
    for i in range(n):
        m = None if mask is None else (mask if mask.dim() == 3 else mask[i]).double()
        want = ref_cpu.mse(x_hat[i].double(), tf[i], m)
        assert abs(float(got[i]) - float(want)) <= 1e-15 * float(want), (i, float(got[i]), float(want))
    got32 = per_frame_mse(x_hat, target, mask, torch.float32)
    assert got32.dtype == torch.float32 and float((got32.double() - got).abs().max()) <= 1e-6 * float(got.max())
    # a sum with another scale (the kernels' `scale` argument)
    assert torch.allclose(per_frame_mse(x_hat, target, mask, torch.float64, scale=1.0) / 70, got, rtol=1e-14, atol=0)


def test_entry_points_report_argument_errors_and_size_their_workspace_per_frame():
    """Host only: null pointers are BN_E_BADARG, and the workspace is N times what ONE frame needs -- the pieces a
    frame is cut into do not depend on the batch."""
    from behavenet_amd import _hip
    lib = _hip.load()
    assert lib.bn_frame_sq_err(None, None, 0, None, None, 1, 16, 1.0, None, 0, None) == -1
    assert lib.bn_convT2d_last_bf16_sqerr(None, None, None, None, 0, None, None, *([1] * 12), 0, 0.0, 1.0, None, 0,
                                          None) == -1
    assert lib.bn_frame_sq_err_ws_bytes(7, 35) == lib.bn_frame_sq_err_ws_bytes(7, 4096) == 0
    assert lib.bn_frame_sq_err_ws_bytes(1, 61440) == 15 * 4
    assert lib.bn_frame_sq_err_ws_bytes(7, 61440) == 7 * 15 * 4
    assert lib.bn_frame_sq_err_ws_bytes(0, 16) == 0
    for geom in [(1, 32, 64, 64, 1, 5, 5, 2, 1, 1, 128, 128), (1, 16, 14, 15, 3, 5, 5, 3, 1, 2, 42, 44)]:
        one = lib.bn_convT2d_last_bf16_sqerr_ws_bytes(*geom)
        assert one > 0 and one % 4 == 0
        for n in (3, 7, 256):
            assert lib.bn_convT2d_last_bf16_sqerr_ws_bytes(n, *geom[1:]) == n * one
    assert lib.bn_convT2d_last_bf16_sqerr_ws_bytes(4, 8, 8, 8, 1, 5, 5, 2, 1, 1, 16, 16) == 0          # not served
