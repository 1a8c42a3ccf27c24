"""The rounding rule's yardstick, the trial-by-trial store writer and the host logic of ``export_reconstructions`` (a
stub stands in for the device).  No GPU."""

import inspect
import io
import os
import threading
import zipfile

import numpy as np
import pytest
import torch

from behavenet_amd.data import trial_store
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.data.trial_store import NpzSessionWriter, open_trial_store, write_npz_session
from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.fitting import eval as ev
from behavenet_amd import hip_functions as hf
from tests.recon_u8_refs import SPECIALS, quantise_u8, with_specials

DIM = [1, 32, 32]


# ------------------------------------------------------------------------------------------ the rule
def test_quantise_u8_table():
    for v, want in SPECIALS:
        assert int(quantise_u8(np.array([v]))[0]) == want, (v, want)
    got = quantise_u8(np.array([[0.2, np.nan], [2.0, -1.0]]))
    assert got.dtype == np.uint8 and got.shape == (2, 2) and got.tolist() == [[51, 0], [255, 0]]


def test_quantise_u8_round_trip():
    k = np.arange(256)
    assert np.array_equal(quantise_u8(k.astype(np.float32) / np.float32(255)), k)
    # torch's division is the one bn_u8_to_unit_float performs
    assert np.array_equal(quantise_u8((torch.arange(256, dtype=torch.uint8).float() / 255).numpy()), k)


def test_with_specials_places_every_special():
    x = with_specials(np.full(35, 0.25, dtype=np.float32), seed=3)
    assert x.size == 35 and int(np.isnan(x).sum()) == 1 and int(np.isinf(x).sum()) == 2
    assert with_specials(np.zeros(1, dtype=np.float32)).size == 1


# ------------------------------------------------------------------------------------------ the writer
def _trials(rng, lens, dim=(1, 8, 6)):
    return [rng.integers(0, 256, size=(t,) + tuple(dim), dtype=np.uint8) for t in lens]


def test_writer_out_of_order_with_an_empty_member(tmp_path):
    path = os.path.join(str(tmp_path), 'sub', 'recon.npz')
    trials = _trials(np.random.default_rng(0), [5, 0, 3, 7])
    labels = [np.random.default_rng(1).normal(size=(t, 4)).astype(np.float32) for t in (5, 0, 3, 7)]
    w = NpzSessionWriter(path)
    for t in (2, 0, 3, 1):
        w.write('images', t, trials[t])
        assert not os.path.exists(path)          # no half store under the final name
    for t in (3, 1, 0, 2):
        w.write('labels', t, labels[t])
    assert os.path.exists(path + '.tmp') and not os.path.exists(path)
    assert w.close() == path
    assert os.path.exists(path) and not os.path.exists(path + '.tmp')
    w.close()          # (idempotent)
    with pytest.raises(ValueError):
        w.write('images', 4, trials[0])
    store = open_trial_store(path)
    try:
        assert store.signals() == ['images', 'labels'] and store.n_trials('images') == 4
        for t in range(4):
            assert store.layout('images', t) == (np.dtype(np.uint8), trials[t].shape)          # the pread path
            got = store.read('images', t)
            assert got.dtype == np.uint8 and got.shape == trials[t].shape and np.array_equal(got, trials[t])
            assert store.layout('labels', t) is not None and np.array_equal(store.read('labels', t), labels[t])
        assert store.read('images', 1).shape == (0, 1, 8, 6)
        buf = np.empty((0, 1, 8, 6), dtype=np.uint8)
        assert store.read_into('images', 1, buf) is buf
    finally:
        store.close()


def test_zero_frame_member_of_write_npz_session_reads_as_empty(tmp_path):
    """``_NpzStore.read`` raised TypeError (memoryview: cannot cast view with zeros in shape) on such a member."""
    path = write_npz_session(os.path.join(str(tmp_path), 'data.npz'),
                             {'images': [np.zeros((0, 1, 8, 6), dtype=np.uint8), np.ones((2, 1, 8, 6), dtype=np.uint8)]})
    store = open_trial_store(path)
    try:
        got = store.read('images', 0)
        assert got.shape == (0, 1, 8, 6) and got.dtype == np.uint8
        assert store.read('images', 1).sum() == 96
    finally:
        store.close()


def test_writer_as_context_manager_discards_on_error(tmp_path):
    path = os.path.join(str(tmp_path), 'r.npz')
    with pytest.raises(RuntimeError):
        with NpzSessionWriter(path) as w:
            w.write('images', 0, np.zeros((2, 1, 4, 4), dtype=np.uint8))
            raise RuntimeError('interrupted')
    assert os.listdir(str(tmp_path)) == []
    with NpzSessionWriter(path) as w:
        w.write('images', 0, np.zeros((2, 1, 4, 4), dtype=np.uint8))
    assert os.listdir(str(tmp_path)) == ['r.npz']


def test_writer_refuses_a_member_twice(tmp_path):
    path = os.path.join(str(tmp_path), 'r.npz')
    with NpzSessionWriter(path) as w:
        w.write('images', 3, np.zeros((2, 1, 4, 4), dtype=np.uint8))
        w.write('labels', 3, np.zeros((2, 2), dtype=np.float32))          # (another signal: another member)
        with pytest.raises(ValueError, match='already written'):
            w.write('images', 3, np.ones((2, 1, 4, 4), dtype=np.uint8))
    with zipfile.ZipFile(path) as zf:
        assert sorted(zf.namelist()) == ['images/trial_0003.npy', 'labels/trial_0003.npy']
    store = open_trial_store(path)
    try:
        assert not store.read('images', 3).any()
    finally:
        store.close()


def test_write_npz_session_output_is_unchanged(tmp_path, monkeypatch):
    """Byte for byte what the recipe it has always used gives (zip members carry the clock: it is held still)."""
    import time
    monkeypatch.setattr(time, 'localtime', lambda *a: time.struct_time((2024, 1, 2, 3, 4, 6, 1, 2, 0)))
    rng = np.random.default_rng(5)
    signals = {'images': _trials(rng, [3, 1, 4]), 'labels': [rng.normal(size=(t, 2)).astype(np.float32) for t in (3, 1, 4)]}
    path = write_npz_session(os.path.join(str(tmp_path), 'a', 'data.npz'), signals)
    want = io.BytesIO()
    with zipfile.ZipFile(want, 'w', zipfile.ZIP_STORED, allowZip64=True) as zf:
        for signal, trials in signals.items():
            for i, arr in enumerate(trials):
                with zf.open('%s/trial_%04i.npy' % (signal, i), 'w', force_zip64=True) as f:
                    np.lib.format.write_array(f, np.ascontiguousarray(arr), allow_pickle=False)
    with open(path, 'rb') as f:
        got = f.read()
    assert got == want.getvalue()
    # ... and the trial-by-trial writer, fed in the same order, stores the same bytes
    other = os.path.join(str(tmp_path), 'b.npz')
    with NpzSessionWriter(other) as w:
        for signal, trials in signals.items():
            for i, arr in enumerate(trials):
                w.write(signal, i, arr)
    with open(other, 'rb') as f:
        assert f.read() == got


# ------------------------------------------------------------------------------------------ the public surface
def test_get_reconstruction_signature_ends_in_as_uint8():
    params = list(inspect.signature(ev.get_reconstruction).parameters.values())
    assert params[-1].name == 'as_uint8' and params[-1].default is False
    assert [p.name for p in params[:-1]] == ['model', 'inputs', 'dataset', 'return_latents', 'labels', 'labels_2d',
                                             'apply_inverse_transform', 'use_mean']
    sig = inspect.signature(ev.reconstruct_trial_device)
    assert list(sig.parameters) == ['model', 'y', 'sess', 'labels', 'labels_2d', 'chunk_size']
    assert sig.parameters['chunk_size'].default == 200
    assert list(inspect.signature(ev.reconstruct_trial).parameters) == list(sig.parameters)


def test_requests_are_thread_local_and_exclusive():
    assert hf.frame_u8_request() is None
    with hf.quantising_frames() as req:
        assert hf.frame_u8_request() is req and req.frames is None
        with hf.quantising_frames() as inner:
            assert hf.frame_u8_request() is inner
        assert hf.frame_u8_request() is req
    assert hf.frame_u8_request() is None
    # both requests at once: an error before anything is looked at, let alone launched
    with hf.scoring_frames(torch.zeros(1), None, 1.0):
        with pytest.raises(RuntimeError, match='scoring request is open'):
            with hf.quantising_frames():
                pass
    with hf.quantising_frames():
        with pytest.raises(RuntimeError, match='quantising request is open'):
            with hf.scoring_frames(torch.zeros(1), None, 1.0):
                pass
    assert hf.frame_u8_request() is None and hf.frame_err_request() is None
    # another thread sees neither this thread's request nor its conflict, and leaves nothing behind here
    seen = {}

    def other():
        seen['outer'] = hf.frame_u8_request()
        with hf.scoring_frames(torch.zeros(1), None, 1.0):          # (would raise if the request were shared)
            seen['scoring'] = hf.frame_err_request() is not None
        with hf.quantising_frames() as theirs:
            seen['theirs'] = theirs
            seen['inside'] = hf.frame_u8_request()
    with hf.quantising_frames() as req:
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert hf.frame_u8_request() is req and hf.frame_err_request() is None
    assert seen['outer'] is None and seen['scoring'] and seen['inside'] is seen['theirs'] is not req
    assert hf.frame_u8_request() is None
    with pytest.raises(RuntimeError, match='at once'):
        hf.convT_stack_bf16([], torch.zeros(1), [], frame_err=hf.FrameErrRequest(None, None, 1.0),
                            frame_u8=hf.FrameU8Request())


# ------------------------------------------------------------------------------------------ the export's host logic
def _two_sessions():
    sessions = [SyntheticSession(10, [4 + (t % 3) for t in range(10)], DIM, seed=20 + i,
                                 trial_splits='5;1;1;1', name=('lab', 'expt', 'animal', 's%d' % i))
                for i in range(2)]
    return SyntheticSessionsGenerator(sessions, device='cpu', placement='host')


class _StubModel(torch.nn.Module):
    def __init__(self, expt_dir, **hp):
        super().__init__()
        self.hparams = dict({'model_class': 'ae', 'model_type': 'conv', 'expt_dir': expt_dir}, **hp)
        self.version = 0


def _stub_reconstruct(model, y, sess=None, labels=None, labels_2d=None, chunk_size=200):
    """Grey levels that name the frame and the session."""
    y = y if y.dtype == torch.uint8 else (y * 255).round().to(torch.uint8)
    return (y.to(torch.int32) + 1 + int(sess or 0)).remainder(256).to(torch.uint8)


def _trial_frames(gen, sess, trial):
    for dt in ('train', 'val', 'test'):
        gen.reset_iterators(dt)
        for _ in range(gen.n_tot_batches[dt]):
            data, s_ = gen.next_batch(dt)
            if s_ == sess and int(data['batch_idx']) == trial:
                return data['images'][0]
    raise KeyError((sess, trial))


def test_export_reconstructions_host_walk(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'reconstruct_trial_device', _stub_reconstruct)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    gen = _two_sessions()
    files = ev.export_reconstructions(gen, _StubModel(str(tmp_path)))
    assert [os.path.basename(f) for f in files] == ['lab_expt_animal_s%d_reconstructions.npz' % i for i in range(2)]
    assert sorted(os.listdir(os.path.join(str(tmp_path), 'version_0'))) == sorted(os.path.basename(f) for f in files)
    n_gap = 0
    for sess, path in enumerate(files):
        ds = gen.datasets[sess]
        used = set(int(t) for k in ('train', 'val', 'test') for t in ds.batch_idxs[k])
        store = open_trial_store(path)
        try:
            assert store.signals() == ['images'] and store.n_trials('images') == ds.n_trials
            for t in range(ds.n_trials):
                got = store.read('images', t)
                assert got.dtype == np.uint8 and store.layout('images', t) is not None
                if t not in used:
                    n_gap += 1
                    assert got.shape == (0,) + tuple(DIM)
                    continue
                want = _stub_reconstruct(None, _trial_frames(gen, sess, t), sess).numpy()
                assert np.array_equal(got, want), (sess, t)
        finally:
            store.close()
    assert n_gap > 0


def test_export_reconstructions_takes_a_filename_for_one_session_only(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'reconstruct_trial_device', _stub_reconstruct)
    path = os.path.join(str(tmp_path), 'one.npz')
    with pytest.raises(ValueError, match='one file per session'):
        ev.export_reconstructions(_two_sessions(), _StubModel(str(tmp_path)), filename=path)
    assert os.listdir(str(tmp_path)) == []
    one = SyntheticSessionsGenerator([SyntheticSession(10, 5, DIM, seed=3, trial_splits='5;1;1;1')], device='cpu',
                                     placement='host')
    assert ev.export_reconstructions(one, _StubModel(str(tmp_path)), filename=path) == [path]
    assert os.listdir(str(tmp_path)) == ['one.npz']


def test_export_reconstructions_is_rank_zeros_alone(tmp_path, monkeypatch):
    monkeypatch.setattr(ev, 'reconstruct_trial_device', _stub_reconstruct)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    gen = _two_sessions()
    asked = []
    real = gen.next_batch
    monkeypatch.setattr(gen, 'next_batch', lambda *a, **k: (asked.append(a), real(*a, **k))[1])
    monkeypatch.setattr(bdist, 'world_size', lambda: 2)
    monkeypatch.setattr(bdist, 'rank', lambda: 1)
    assert ev.export_reconstructions(gen, _StubModel(str(tmp_path))) == [] and asked == []
    assert os.listdir(os.path.join(str(tmp_path), 'version_0')) == []
    monkeypatch.setattr(bdist, 'rank', lambda: 0)
    files = ev.export_reconstructions(gen, _StubModel(str(tmp_path)))          # (no process group: no collective)
    assert len(files) == 2 and asked
    for sess, path in enumerate(files):
        ds = gen.datasets[sess]
        store = open_trial_store(path)
        try:
            for k in ('train', 'val', 'test'):
                for t in ds.batch_idxs[k]:
                    assert store.read('images', int(t)).shape[0] > 0          # every trial, not every second one
        finally:
            store.close()


def test_an_interrupted_export_leaves_no_store(tmp_path, monkeypatch):
    calls = []

    def failing(model, y, sess=None, labels=None, labels_2d=None, chunk_size=200):
        calls.append(1)
        if len(calls) == 4:
            raise RuntimeError('device lost')
        return _stub_reconstruct(model, y, sess)
    monkeypatch.setattr(ev, 'reconstruct_trial_device', failing)
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    with pytest.raises(RuntimeError, match='device lost'):
        ev.export_reconstructions(_two_sessions(), _StubModel(str(tmp_path)))
    assert os.listdir(os.path.join(str(tmp_path), 'version_0')) == []


def test_trial_store_module_exports_the_writer():
    assert 'NpzSessionWriter' in trial_store.__all__ and 'export_reconstructions' in ev.__all__
