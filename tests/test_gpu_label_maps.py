"""One-hot label maps built on the device (csrc/cond_input.hip, _hip.cond_encoder_input, models.aes.encoder_input,
hparams['hip_label_maps'] = 'device').

The yardstick is tests/label_map_refs.py: ``torch.cat((frames as float32, MakeOneHot2D(H, W)(coords)), 1)`` built by
numpy.  Every comparison is ``torch.equal``: the kernel copies, divides a byte by 255.f as ``u8_to_unit_float`` does,
and writes zeros and ones.  On the model, dense maps and coordinates of the same labels feed the same kernels the
same bits, so every result is compared for identity too.

Operands of the direct calls sit between NaN guard bands, and so does the output, which starts as NaN: an element the
kernel does not write fails the comparison, a write outside fails the band check; LDS starts poisoned (conftest)."""

import os
import pickle

import numpy as np
import pytest
import torch

import behavenet_amd.fitting.eval as ev
from behavenet_amd import _hip
from behavenet_amd.data.data_generator import ConcatSessionsGenerator
from behavenet_amd.data.transforms import MakeOneHot2D
from behavenet_amd.data.trial_store import write_npz_session
from behavenet_amd.data.utils import get_data_generator_inputs
from behavenet_amd.fitting.graph_step import GraphedLoss
from behavenet_amd.models.aes import encoder_input
from tests.cases import case_data
from tests.label_map_refs import encoder_input_ref, probe_coords, random_coords
from tests.test_gpu_encode_bf16 import _small, guarded_u8
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_SHAPE = -2


# ------------------------------------------------------------------------------------------ operands
def _frames(t, c, h, w, u8, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (t, c, h, w), generator=g, dtype=torch.uint8)
    return x if u8 else x.float() / 255


def _place(t, offset=0):
    """A device copy of the CPU tensor ``t`` between guard bands, starting ``offset`` ELEMENTS off its boundary."""
    make = guarded_u8 if t.dtype == torch.uint8 else guarded
    if not offset:
        return make(t)
    flat = torch.cat([t.flatten()[:offset], t.flatten()])
    return make(flat)[offset:].view(t.shape)


def _run_guarded(frames, coords, n_maps, offset=0, out_offset=0):
    """The C entry point itself on guarded operands -> the output, a device view between NaN bands."""
    t, c, h, w = frames.shape
    x = _place(frames, offset)
    cd = guarded(torch.from_numpy(np.ascontiguousarray(coords)))
    flat = guarded(torch.zeros(t * (c + n_maps) * h * w + out_offset))
    flat.fill_(float('nan'))
    out = flat[out_offset:].view(t, c + n_maps, h, w)
    rc = _hip.load().bn_cond_encoder_input(x.data_ptr(), int(frames.dtype == torch.uint8), cd.data_ptr(),
                                           int(coords.shape[1]), t, c, h, w, n_maps, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out


def _both_ways(frames, coords, n_maps=None, want=None, **where):
    """The wrapper and the guarded direct call against the reference."""
    cols = coords.shape[1] // 2 if n_maps is None else n_maps
    if want is None:
        want = encoder_input_ref(frames, coords[:, :2 * cols])
    got = _hip.cond_encoder_input(frames.to(DEV), torch.from_numpy(coords).to(DEV), n_maps)
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_run_guarded(frames, coords, cols, **where).cpu(), want)
    return got


# ------------------------------------------------------------------------------------------ 1: the kernel
SHAPES = [(1, 1, 1, 1, 1),          # the smallest case
          (3, 1, 5, 7, 2),          # H W % 4 != 0: element by element
          (5, 2, 8, 12, 3),         # 16-byte stores, two image channels
          (2, 1, 128, 128, 4),      # the workload's plane: four segments a plane
          (257, 1, 4, 4, 1),        # more frames than one grid row
          (4, 1, 6, 6, 0),          # no maps: the plain conversion
          (0, 1, 8, 8, 2)]          # an empty result and no error


@pytest.mark.parametrize('u8', [True, False], ids=['u8', 'fp32'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_kernel_against_the_reference(shape, u8):
    t, c, h, w, n_maps = shape
    frames = _frames(t, c, h, w, u8, seed=sum(shape))
    coords = random_coords(t, n_maps, h, w, seed=1 + sum(shape))
    got = _both_ways(frames, coords)
    if u8 and t:
        # the image channels are u8_to_unit_float's, bit for bit
        assert torch.equal(got[:, :c], _hip.u8_to_unit_float(frames.to(DEV)))
    if n_maps and t:
        assert torch.equal(got[:, c:].sum(dim=(2, 3)), torch.ones((t, n_maps), device=DEV))


@pytest.mark.parametrize('u8', [True, False], ids=['u8', 'fp32'])
def test_views_off_alignment_take_the_other_loads_and_match(u8):
    # x[1:] of frames with an odd H W starts 35 bytes / 35 floats into its buffer
    t, c, h, w, n_maps = 4, 1, 5, 7, 2
    frames = _frames(t + 1, c, h, w, u8, seed=3)
    coords = random_coords(t, n_maps, h, w, seed=4)
    view = frames.to(DEV)[1:]
    assert view.data_ptr() % (4 if u8 else 16) != 0 and view.is_contiguous()
    got = _hip.cond_encoder_input(view, torch.from_numpy(coords).to(DEV))
    assert torch.equal(got.cpu(), encoder_input_ref(frames[1:], coords))
    # planes the vector path serves (H W % 4 == 0) from frames, or into an output, one element off their boundary
    frames = _frames(3, 2, 4, 8, u8, seed=5)
    coords = random_coords(3, n_maps, 4, 8, seed=6)
    _both_ways(frames, coords)
    _both_ways(frames, coords, offset=1)
    _both_ways(frames, coords, out_offset=1)


def test_odd_and_strided_coordinate_columns():
    t, c, h, w = 6, 1, 8, 12
    frames = _frames(t, c, h, w, True, seed=7)
    coords = random_coords(t, 2, h, w, seed=8, extra_cols=1)          # 5 columns: two maps, the fifth is ignored
    assert coords.shape[1] == 5
    want = encoder_input_ref(frames, coords)
    assert tuple(want.shape) == (t, 3, h, w)
    _both_ways(frames, coords, want=want)
    # a row-strided view of a wider tensor
    wide = torch.full((t, 9), 3.0e5)
    wide[:, :5] = torch.from_numpy(coords)
    view = wide.to(DEV)[:, :5]
    assert not view.is_contiguous()
    assert torch.equal(_hip.cond_encoder_input(frames.to(DEV), view).cpu(), want)
    # fewer maps than the columns would give: y comes from column n_maps + l
    _both_ways(frames, coords, n_maps=1, want=encoder_input_ref(frames, coords[:, :2]))
    # float64 coordinates are converted, as the generator's float32 cast does
    assert torch.equal(_hip.cond_encoder_input(frames.to(DEV), torch.from_numpy(coords).double().to(DEV)).cpu(), want)


@pytest.mark.parametrize('u8', [True, False], ids=['u8', 'fp32'])
@pytest.mark.parametrize('h, w', [(5, 7), (8, 12)])
def test_probe_rows(h, w, u8):
    n_maps = 3
    coords = probe_coords(h, w, n_maps)
    frames = _frames(coords.shape[0], 1, h, w, u8, seed=h)
    _both_ways(frames, coords)


def test_refused_calls_write_nothing():
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    x = guarded(torch.zeros((3, 1, 4, 8)))
    cd = guarded(torch.zeros((3, 4)))
    out = guarded(torch.full((3, 3, 4, 8), 7.0))

    def call(xp=None, cp=None, op=None, ld=4, n=3, c=1, h=4, w=8, n_maps=2):
        return lib.bn_cond_encoder_input(xp or x.data_ptr(), 0, cp or cd.data_ptr(), ld, n, c, h, w, n_maps,
                                         op or out.data_ptr(), st)
    assert call(ld=3) == E_SHAPE and call(c=0) == E_SHAPE and call(h=-4) == E_SHAPE and call(n_maps=-1) == E_SHAPE
    assert call(xp=x.data_ptr() + 2) == E_SHAPE and call(cp=cd.data_ptr() + 1) == E_SHAPE
    assert call(op=out.data_ptr() + 2) == E_SHAPE
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the same call with nothing wrong is accepted, and writes
    assert call() == 0
    assert not bool((out == 7.0).any())


def test_one_graph_follows_its_static_coordinates():
    t, c, h, w, n_maps = 6, 1, 16, 20, 2
    frames = _frames(t, c, h, w, True, seed=9)
    first, second = random_coords(t, n_maps, h, w, seed=10), random_coords(t, n_maps, h, w, seed=11)
    assert not torch.equal(encoder_input_ref(frames, first), encoder_input_ref(frames, second))
    static_x = frames.to(DEV)
    static_c = torch.from_numpy(first).to(DEV)
    _hip.cond_encoder_input(static_x, static_c)          # (code object loaded before the recording)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _hip.cond_encoder_input(static_x, static_c)
    graph.replay()
    assert torch.equal(out.cpu(), encoder_input_ref(frames, first))
    static_c.copy_(torch.from_numpy(second).to(DEV))
    graph.replay()
    assert torch.equal(out.cpu(), encoder_input_ref(frames, second))


# ------------------------------------------------------------------------------------------ 2: the model
N = 16
GOLDEN = 'condae_enc_cfg1'          # cond-ae, conditional_encoder, 1x32x32, four labels = two maps


class _Case(object):
    """The golden cond-ae architecture on ``N`` frames with the same labels as dense maps and as coordinates."""

    def __init__(self, extra=None):
        self.model, self.meta = _small(golden=GOLDEN, n=N, extra=extra)
        _, self.h, self.w = self.meta['dim']
        data = case_data(self.meta, device=DEV)
        self.x = data['images'][0].contiguous()
        self.labels = data['labels'][0]
        g = torch.Generator().manual_seed(12)
        self.xu = torch.randint(0, 256, tuple(self.x.shape), generator=g, dtype=torch.uint8).to(DEV)
        coords = random_coords(N, self.meta['n_labels'] // 2, self.h, self.w, seed=13)
        self.coords = torch.from_numpy(coords).to(DEV)
        self.dense = torch.from_numpy(MakeOneHot2D(self.h, self.w)(coords).astype(np.float32)).to(DEV)
        assert tuple(self.dense.shape) == (N, 2, self.h, self.w)

    def data(self, labels_sc):
        return {'images': self.x[None], 'labels': self.labels[None], 'labels_sc': labels_sc[None]}


@pytest.fixture(scope='module')
def case():
    return _Case()


def test_helper_gives_the_concatenation(case):
    for x in (case.x, case.xu):
        want = torch.cat((x if x.dtype == torch.float32 else _hip.u8_to_unit_float(x), case.dense), 1)
        for labels_2d in (case.dense, case.coords):
            got = encoder_input(x, labels_2d)
            assert torch.equal(got, want) and not got.requires_grad
    assert encoder_input(case.xu, None) is case.xu


def test_forward_outputs_are_identical(case):
    for train in (False, True):
        case.model.train(train)
        with torch.no_grad():
            dense = case.model(case.x, dataset=0, labels=case.labels, labels_2d=case.dense)
            coords = case.model(case.x, dataset=0, labels=case.labels, labels_2d=case.coords)
        assert len(dense) == len(coords) == 2
        for a, b in zip(dense, coords):
            assert torch.equal(a, b)
    case.model.eval()


def _loss_and_grads(model, data, chunk_size):
    model.train()
    model.zero_grad()
    out = dict(model.loss(data, dataset=0, accumulate_grad=True, chunk_size=chunk_size))
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert grads
    return out, grads


@pytest.mark.parametrize('schedule', ['whole batch', 'whole batch, batch norm', 'chunks, batch norm'])
def test_loss_and_gradients_are_identical(schedule, monkeypatch):
    case = _Case({'ae_batch_norm': True} if 'batch norm' in schedule else None)
    if schedule.startswith('chunks'):
        monkeypatch.setenv('BN_WHOLE_BATCH', '0')
        assert case.model._pass_groups(case.x, 6) is None
    else:
        assert case.model._pass_groups(case.x, 6) == [(0, N)]
    loss_d, grads_d = _loss_and_grads(case.model, case.data(case.dense), 6)          # chunks of 6, 6 and 4 frames
    loss_c, grads_c = _loss_and_grads(case.model, case.data(case.coords), 6)
    assert loss_d == loss_c and np.isfinite(loss_d['loss'])
    assert sorted(grads_d) == sorted(grads_c)
    for k in grads_d:
        assert torch.equal(grads_d[k], grads_c[k]), k
        assert bool(grads_d[k].abs().max() > 0) or k.endswith('bias'), k


def test_graphed_step_takes_coordinates_as_a_static_tensor():
    case = _Case()
    # a freshly initialised model hardly looks at two pixels of a map (moving them leaves the fp32 loss where it is):
    # give the first layer's taps on the map channels a weight that shows
    w0 = next(p for p in case.model.encoding.parameters() if p.dim() == 4 and p.shape[1] == 3)
    with torch.no_grad():
        w0[:, 1:] = 20.0
    eager = dict(case.model.loss(case.data(case.coords), dataset=0, accumulate_grad=False))
    fn = GraphedLoss(case.model, warmup=1)
    other = torch.from_numpy(random_coords(N, 2, case.h, case.w, seed=14)).to(DEV)
    want_other = dict(case.model.loss(case.data(other), dataset=0, accumulate_grad=False))
    assert want_other != eager
    got = [dict(fn(case.data(c), dataset=0, accumulate_grad=False)) for c in (case.coords, case.coords, other)]
    assert fn.n_replays >= 1
    assert got[0] == got[1] == eager and got[2] == want_other


@pytest.fixture
def u8_conversions(monkeypatch):
    """Counts the calls of ``_hip.u8_to_unit_float``: with coordinates the stored frames are never converted apart."""
    calls = []
    real = _hip.u8_to_unit_float

    def counted(u8):
        calls.append(tuple(u8.shape))
        return real(u8)
    monkeypatch.setattr(_hip, 'u8_to_unit_float', counted)
    return calls


def test_inference_entry_points_are_identical_from_uint8_frames(case, u8_conversions):
    model, xu, labels = case.model, case.xu, case.labels
    g = torch.Generator().manual_seed(15)
    mask = (torch.rand((N,) + tuple(xu.shape[1:]), generator=g) > 0.3).float().to(DEV)
    calls = {
        'encode_trial': lambda l2d: ev.encode_trial(model, xu, 0, l2d),
        'encode_trial chunks': lambda l2d: ev.encode_trial(model, xu, 0, l2d, chunk_size=5),
        'frame_errors': lambda l2d: ev.frame_errors(model, xu, 0, mask, labels, l2d),
        'frame_errors chunks': lambda l2d: ev.frame_errors(model, xu, 0, mask, labels, l2d, chunk_size=5),
        'reconstruct_trial': lambda l2d: ev.reconstruct_trial(model, xu, 0, labels, l2d),
        'reconstruct_trial chunks': lambda l2d: ev.reconstruct_trial(model, xu, 0, labels, l2d, chunk_size=5),
        'pixel_stats': lambda l2d: ev.pixel_stats(model, xu, 0, mask, labels, l2d),
        'pixel_stats chunks': lambda l2d: ev.pixel_stats(model, xu, 0, mask, labels, l2d, chunk_size=5),
    }
    for name, call in calls.items():
        dense = call(case.dense)
        assert u8_conversions, name          # (dense maps: the frames are converted first, as before)
        del u8_conversions[:]
        coords = call(case.coords)
        assert not u8_conversions, (name, u8_conversions)
        assert dense.shape == coords.shape and dense.size > 0 and np.array_equal(dense, coords), name
    # ... and from fp32 frames
    xf = _hip.u8_to_unit_float(xu)
    assert np.array_equal(ev.encode_trial(model, xf, 0, case.dense), ev.encode_trial(model, xf, 0, case.coords))
    assert np.array_equal(ev.encode_trial(model, xf, 0, case.coords), ev.encode_trial(model, xu, 0, case.coords))


def test_get_reconstruction_takes_coordinates(case):
    for as_uint8 in (False, True):
        dense = ev.get_reconstruction(case.model, case.x, dataset=0, return_latents=True, labels=case.labels,
                                      labels_2d=case.dense, as_uint8=as_uint8)
        coords = ev.get_reconstruction(case.model, case.x, dataset=0, return_latents=True, labels=case.labels,
                                       labels_2d=case.coords, as_uint8=as_uint8)
        for a, b in zip(dense, coords):
            assert a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ 3: generator and exporters
def test_generator_feed_and_export_latents_under_both_settings(tmp_path, monkeypatch):
    monkeypatch.delenv('BN_LABEL_MAPS', raising=False)
    root = str(tmp_path)
    case = _Case({'expt_dir': root})
    model, (h, w) = case.model, (case.h, case.w)
    model.version = 0
    os.makedirs(os.path.join(root, 'version_0'))
    lens = [12, 16]
    rng = np.random.default_rng(16)
    store = {'images': [rng.integers(0, 256, size=(t, 1, h, w), dtype=np.uint8) for t in lens],
             'labels': [rng.standard_normal((t, 4)).astype(np.float32) for t in lens],
             'labels_sc': [random_coords(t, 2, h, w, seed=17 + t) for t in lens]}
    ids = [{'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess'}]
    write_npz_session(os.path.join(root, 'lab', 'expt', 'animal', 'sess', 'data.npz'), store)

    seen = []
    real = ev.encode_trial_device

    def recorded(model_, y, sess=None, labels_2d=None, chunk_size=200):
        seen.append((y.dtype, None if labels_2d is None else labels_2d.dim()))
        return real(model_, y, sess, labels_2d, chunk_size)
    monkeypatch.setattr(ev, 'encode_trial_device', recorded)

    def export(where):
        model.hparams.pop('hip_label_maps', None)
        if where is not None:
            model.hparams['hip_label_maps'] = where
        hp = dict(model.hparams, data_dir=root, y_pixels=h, x_pixels=w)
        _, signals, transforms, paths = get_data_generator_inputs(hp, ids)
        gen = ConcatSessionsGenerator(root, ids, signals_list=signals, transforms_list=transforms, paths_list=paths,
                                      device='cuda', trial_splits={'train_tr': 1, 'val_tr': 1, 'test_tr': 0,
                                                                   'gap_tr': 0})
        gen.reset_iterators('train')
        data, _ = gen.next_batch('train')
        t = lens[int(data['batch_idx'])]
        sc = data['labels_sc']
        gen.reset_iterators('train')
        del seen[:]
        with open(ev.export_latents(gen, model, filename=os.path.join(root, '%s.pkl' % where))[0], 'rb') as f:
            return pickle.load(f), sc, t, list(seen), data

    host, sc_h, t_h, seen_h, _ = export('host')
    assert tuple(sc_h.shape) == (1, t_h, 2, h, w)
    assert seen_h == [(torch.float32, 4)] * 2
    dev, sc_d, t_d, seen_d, data = export('device')
    assert sc_d.is_cuda and sc_d.dtype == torch.float32 and tuple(sc_d.shape) == (1, t_d, 4)
    trial = int(data['batch_idx'])
    assert np.array_equal(sc_d[0].cpu().numpy(), store['labels_sc'][trial], equal_nan=True)
    assert seen_d == [(torch.uint8, 2)] * 2
    # what the generator keeps per trial: the coordinates, 16 bytes a frame
    assert sc_d.numel() * 4 == t_d * 16 and sc_h.numel() * 4 == t_h * 2 * h * w * 4
    for k in ('train', 'val', 'test'):
        assert np.array_equal(np.asarray(host['trials'][k]), np.asarray(dev['trials'][k]))
    assert len(host['latents']) == len(dev['latents']) == 2
    for a, b, t in zip(host['latents'], dev['latents'], lens):
        assert a.shape == (t, model.hparams['n_ae_latents']) and np.array_equal(a, b)
    # the default is the host path
    assert export(None)[3] == seen_h
