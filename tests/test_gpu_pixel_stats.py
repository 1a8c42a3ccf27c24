"""Per-pixel error and moment sums on the GPU (csrc/pixel_stats.hip, fitting.eval.pixel_stats_device /
export_pixel_stats).

The yardstick is tests/pixel_stats_refs.py: the kernel's own fp32 terms, summed in float64 by numpy.  Only the order of
the float64 additions differs, at most N * 2^-53 relative on non-negative sums -- 3.3e-14 at the N <= 300 used here --
so the kernel is held to rtol 1e-12 on planes 0, 2 and 3 and EXACTLY on plane 1 for 0/1 masks and no mask.

Float operands sit between NaN guard bands, LDS starts poisoned (conftest).  A mask pixel that is zero in every frame
makes every sum of that pixel zero in the yardstick, and then zero is what the kernel must give: the comparison has no
absolute part.  Where a summary divides by the weights (the whole-path and end-to-end tests) every mask has a
non-zero entry per pixel, and the random frames give every pixel variance.
"""

import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.data.data_generator import ConcatSessionsGenerator, SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.data.trial_store import write_npz_session
from behavenet_amd.fitting.eval import (encode_trial_device, export_frame_errors, export_pixel_stats,
                                        frame_errors_device, get_reconstruction, pixel_stats, pixel_stats_device,
                                        summarise_pixel_stats)
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from tests.cases import case_data
from tests.golden_utils import base_hparams
from tests.pixel_stats_refs import RTOL, assert_close, pixel_sums
from tests.test_gpu_encode_bf16 import _frames, _small, guarded_u8
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_model import BUILDERS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_SHAPE = -2
ACC_GUARD = 512          # doubles of NaN on either side of an accumulator (the view stays 16-byte aligned)


# ------------------------------------------------------------------------------------------ operands
def _place(t, offset=0):
    """A device copy of the CPU tensor ``t`` between guard bands, starting ``offset`` ELEMENTS off its 16-byte
    boundary."""
    make = guarded_u8 if t.dtype == torch.uint8 else guarded
    if not offset:
        return make(t)
    flat = torch.cat([t.flatten()[:offset], t.flatten()])
    return make(flat)[offset:].view(t.shape)


class _Acc(object):
    """A float64 (4,) + frame accumulator on the device between NaN bands, holding ``values``."""

    def __init__(self, values):
        values = torch.as_tensor(values, dtype=torch.float64)
        self.n = values.numel()
        self.flat = torch.full((self.n + 2 * ACC_GUARD,), float('nan'), dtype=torch.float64, device=DEV)
        self.view = self.flat[ACC_GUARD:ACC_GUARD + self.n].view(values.shape)
        self.view.copy_(values)
        assert self.view.data_ptr() % 16 == 0

    def numpy(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.flat[:ACC_GUARD]).all()), 'write before the accumulator'
        assert bool(torch.isnan(self.flat[ACC_GUARD + self.n:]).all()), 'write past the accumulator'
        return self.view.cpu().numpy()


MASKS = ['none', 'trial01', 'trialfrac', 'frame01', 'framefrac']


def _operands(n, shape, seed, u8, mask_kind):
    """x_hat uniform in (0, 1), uniform random uint8 frames (as uint8 or as fp32 value / 255) and a mask, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x_hat = torch.rand((n,) + shape, generator=g)
    tu = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
    mshape = shape if mask_kind.startswith('trial') else (n,) + shape
    mask = None
    if mask_kind.endswith('01'):
        mask = (torch.rand(mshape, generator=g) > 0.3).float()
    elif mask_kind.endswith('frac'):
        mask = torch.rand(mshape, generator=g) * 0.75 + 0.25
    return x_hat, (tu if u8 else tu.float() / 255), mask


def _run(x_hat, target, mask, acc0=None, offset=0):
    """``_hip.pixel_stats_accum`` between guard bands -> (4,) + frame float64 numpy."""
    acc = _Acc(torch.zeros((4,) + tuple(target.shape[1:]), dtype=torch.float64) if acc0 is None else acc0)
    got = _hip.pixel_stats_accum(None if x_hat is None else _place(x_hat, offset), _place(target, offset),
                                 None if mask is None else _place(mask, offset), acc.view)
    assert got is acc.view
    return acc.numpy()


# ------------------------------------------------------------------------------------------ 1: the kernel
SHAPES = [(1, 5, 7), (1, 30, 26), (1, 64, 48)]          # D = 35 (no vector path), 780 (4 | D, 16 does not), 3072
NS = [1, 2, 7, 33, 67, 300]                              # one frame, a part block, several blocks


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_kernel_against_the_yardstick(shape, n):
    d = int(np.prod(shape))
    for u8 in (False, True):
        for mask_kind in MASKS:
            x_hat, target, mask = _operands(n, shape, d + n + 7 * u8 + MASKS.index(mask_kind), u8, mask_kind)
            want = pixel_sums(x_hat, target, mask)
            got = _run(x_hat, target, mask)
            assert_close(got, want, exact_w=not mask_kind.endswith('frac'),
                         name='%s N=%d %s %s' % (shape, n, 'u8' if u8 else 'fp32', mask_kind))
            if mask is None:
                assert np.all(got[1] == n)


@pytest.mark.parametrize('n', [7, 67])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_without_xhat_plane_0_keeps_its_bits(shape, n):
    d = int(np.prod(shape))
    for u8, mask_kind in [(True, 'trial01'), (False, 'framefrac'), (True, 'none')]:
        _, target, mask = _operands(n, shape, d + n, u8, mask_kind)
        acc0 = torch.zeros((4,) + shape, dtype=torch.float64)
        acc0[0] = -12345.678
        got = _run(None, target, mask, acc0=acc0)
        assert np.array_equal(got[0], acc0[0].numpy())
        want = pixel_sums(None, target, mask)
        want[0] = acc0[0].numpy()
        assert_close(got, want, exact_w=not mask_kind.endswith('frac'), name='no xhat %s N=%d' % (shape, n))


@pytest.mark.parametrize('n', [7, 67])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_accumulator_is_added_to(shape, n):
    d = int(np.prod(shape))
    g = torch.Generator().manual_seed(d)
    for u8, mask_kind in [(False, 'trial01'), (True, 'framefrac')]:
        x_hat, target, mask = _operands(n, shape, d + 2 * n, u8, mask_kind)
        acc0 = torch.rand((4,) + shape, generator=g, dtype=torch.float64) * 50 + 1
        acc0[1] = torch.randint(1, 1000, shape, generator=g).double()          # (integers: plane 1 stays exact)
        got = _run(x_hat, target, mask, acc0=acc0)
        want = acc0.numpy() + pixel_sums(x_hat, target, mask)
        assert_close(got, want, exact_w=mask_kind.endswith('01'), name='accumulate %s N=%d' % (shape, n))


@pytest.mark.parametrize('n', [2, 33, 300])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_two_halves_of_a_trial_give_the_whole(shape, n):
    d = int(np.prod(shape))
    for u8, mask_kind in [(True, 'none'), (False, 'frame01'), (True, 'trialfrac')]:
        x_hat, target, mask = _operands(n, shape, d + 3 * n, u8, mask_kind)
        per_frame = mask is not None and mask.dim() == 4
        h = n // 2
        first = _run(x_hat[:h], target[:h], mask[:h] if per_frame else mask)
        both = _run(x_hat[h:], target[h:], mask[h:] if per_frame else mask, acc0=torch.from_numpy(first))
        assert_close(both, pixel_sums(x_hat, target, mask), exact_w=not mask_kind.endswith('frac'),
                     name='halves %s N=%d' % (shape, n))


@pytest.mark.parametrize('n', [7, 67])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_misaligned_operands_and_repetition_give_the_same_bits(shape, n):
    d = int(np.prod(shape))
    for u8, mask_kind in [(False, 'none'), (True, 'frame01'), (False, 'trialfrac'), (True, 'framefrac')]:
        x_hat, target, mask = _operands(n, shape, d + 5 * n, u8, mask_kind)
        full = _run(x_hat, target, mask)
        assert np.array_equal(full, _run(x_hat, target, mask)), 'repetition'
        # one element off the 16-byte boundary: other loads, the same arithmetic in the same order
        assert np.array_equal(full, _run(x_hat, target, mask, offset=1)), ('offset', shape, n, u8, mask_kind)


def test_refused_calls_write_nothing():
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    n, d = 33, 35
    target = torch.rand((n, d), device=DEV)
    mask = torch.ones((n, d), device=DEV)
    acc = _Acc(torch.full((4, d + 1), 7.0, dtype=torch.float64))
    need = lib.bn_pixel_stats_ws_bytes(n, d)
    assert need > 0
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(n_=n, d_=d, mask_frames=0, ws_bytes=need, accp=None, wsp=None, m=None):
        return lib.bn_pixel_stats_accum(target.data_ptr(), target.data_ptr(), 0, m, mask_frames,
                                        accp or acc.view.data_ptr(), n_, d_, wsp or ws.data_ptr(), ws_bytes, st)
    assert call(n_=0) == E_SHAPE and call(n_=-1) == E_SHAPE
    assert call(d_=0) == E_SHAPE
    assert call(n_=5, mask_frames=2, m=mask.data_ptr()) == E_SHAPE
    assert call(ws_bytes=need - 1) == E_SHAPE
    assert call(accp=acc.view.data_ptr() + 8) == E_SHAPE
    assert call(wsp=ws.data_ptr() + 8) == E_SHAPE
    assert call(m=mask.data_ptr() + 2, mask_frames=n) == E_SHAPE          # fp32 operands off a 4-byte boundary
    assert np.all(acc.numpy() == 7.0)
    # ... and the same call with nothing wrong is accepted, and writes
    assert call(m=mask.data_ptr(), mask_frames=n) == 0
    assert not np.all(acc.numpy() == 7.0)


def test_wrapper_checks_shapes_dtypes_and_devices():
    target = torch.zeros((3, 1, 4, 4), device=DEV)
    acc = torch.zeros((4, 1, 4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(_hip.HipLibraryError, match='share a shape'):
        _hip.pixel_stats_accum(torch.zeros((3, 1, 4, 5), device=DEV), target, None, acc)
    with pytest.raises(_hip.HipLibraryError, match='mask'):
        _hip.pixel_stats_accum(None, target, torch.zeros((2, 1, 4, 4), device=DEV), acc)
    with pytest.raises(_hip.HipLibraryError, match='acc'):
        _hip.pixel_stats_accum(None, target, None, acc[:3])
    with pytest.raises(_hip.HipLibraryError, match='dtype'):
        _hip.pixel_stats_accum(None, target, None, acc.float())
    with pytest.raises(_hip.HipLibraryError, match='GPU'):
        _hip.pixel_stats_accum(None, target, None, acc.cpu())
    with pytest.raises(_hip.HipLibraryError, match='float32 or uint8'):
        _hip.pixel_stats_accum(None, target.double(), None, acc)
    assert not bool(acc.any())


# ------------------------------------------------------------------------------------------ 2: the whole path
CLASSES = ['ae', 'vae', 'ps-vae', 'cond-ae']
TRIALS = [12, 67]
DIM = (1, 64, 48)


def _case(model_class, n):
    """(model, frames on the device, forward kwargs, labels, frame dimensions): the default architecture at 1x64x48
    on random uint8 frames; cond-ae at its golden case's own size, with labels."""
    if model_class == 'cond-ae':
        model, meta = _small(golden='condae_cfg1', n=n)
        data = case_data(meta, device=DEV)
        x, labels = data['images'][0].contiguous(), data['labels'][0]
        kwargs = {'dataset': 0, 'labels': labels, 'labels_2d': None}
    else:
        model, meta = _small(model_class, DIM, n)
        x, labels = _frames(n, DIM, 7 + n).to(DEV), None
        kwargs = {'dataset': 0, 'use_mean': True} if model_class in ('vae', 'ps-vae') else {'dataset': 0}
    model.eval()
    return model, x, kwargs, labels, tuple(x.shape[1:])


def _masks(dim, n, seed):
    """None, a fractional mask for the trial, 0/1 masks per frame -- each pixel non-zero in at least one frame."""
    g = torch.Generator().manual_seed(seed)
    frame01 = (torch.rand((n,) + tuple(dim), generator=g) > 0.3).float()
    frame01[0][frame01.sum(dim=0) == 0] = 1
    return [(None, True), (torch.rand(tuple(dim), generator=g) * 0.75 + 0.25, False), (frame01, True)]


def _x_hat(model, x, kwargs, dtypes=('f32', 'f32')):
    with torch.no_grad(), hf.encode_precision(dtypes[0]), hf.decode_precision(dtypes[1]):
        return model(x, **kwargs)[0].view(x.shape).cpu()


@pytest.mark.parametrize('n', TRIALS)
@pytest.mark.parametrize('model_class', CLASSES)
def test_fp32_lane(model_class, n):
    model, x, kwargs, labels, dim = _case(model_class, n)
    x_hat = _x_hat(model, x, kwargs)
    for mask, exact_w in _masks(dim, n, 5):
        want = pixel_sums(x_hat, x, mask)
        md = None if mask is None else mask.to(DEV)
        with warnings.catch_warnings():
            warnings.simplefilter('error', UserWarning)
            got = pixel_stats_device(model, x, 0, md, labels=labels)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (4,) + dim
        assert_close(got, want, exact_w, name='fp32 lane %s N=%d' % (model_class, n))
        # chunks change the order of the float64 additions and nothing else
        chunked = pixel_stats(model, x, 0, md, labels=labels, chunk_size=16)
        assert chunked.dtype == np.float64
        np.testing.assert_allclose(chunked, got.cpu().numpy(), rtol=RTOL, atol=0)
        # ``out`` is returned and added to
        out = got.clone()
        assert pixel_stats_device(model, x, 0, md, labels=labels, out=out) is out
        np.testing.assert_allclose(out.cpu().numpy(), 2 * got.cpu().numpy(), rtol=RTOL, atol=0)
    if x.dtype == torch.uint8:
        # the same from fp32 frames: the target's value / 255 is the kernel's own division
        xf = (x.float() / 255).contiguous()
        assert_close(pixel_stats_device(model, xf, 0, labels=labels), pixel_sums(_x_hat(model, xf, kwargs), xf, None),
                     True, name='fp32 frames %s' % model_class)


@pytest.mark.parametrize('n', TRIALS)
@pytest.mark.parametrize('model_class', ['ae', 'vae', 'ps-vae'])
def test_both_bf16_keys_on_a_served_architecture(model_class, n):
    model, x, kwargs, labels, dim = _case(model_class, n)
    f32 = _x_hat(model, x, kwargs)
    model.hparams.update(hip_encode_dtype='bf16', hip_decode_dtype='bf16')
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)          # (served: no warning)
        x_hat = _x_hat(model, x, kwargs, ('bf16', 'bf16'))
        assert not torch.equal(x_hat, f32)                   # the bf16 code ran
        for mask, exact_w in _masks(dim, n, 6):
            got = pixel_stats_device(model, x, 0, None if mask is None else mask.to(DEV))
            assert_close(got, pixel_sums(x_hat, x, mask), exact_w, name='bf16 keys %s N=%d' % (model_class, n))
    # each key alone: the other half stays fp32
    for keys, dtypes in [({'hip_encode_dtype': 'bf16', 'hip_decode_dtype': 'f32'}, ('bf16', 'f32')),
                         ({'hip_encode_dtype': 'f32', 'hip_decode_dtype': 'bf16'}, ('f32', 'bf16'))]:
        model.hparams.update(keys)
        assert_close(pixel_stats_device(model, x, 0), pixel_sums(_x_hat(model, x, kwargs, dtypes), x, None), True,
                     name='%s %s' % (model_class, dtypes))


def test_unserved_model_under_the_keys_warns_once_and_runs_fp32():
    n = 12
    model, meta = _small(golden='ae_cfg1_bn', n=n)
    x = case_data(meta, device=DEV)['images'][0].contiguous()
    want, want5 = pixel_stats_device(model, x, 0).clone(), pixel_stats_device(model, x[:5], 0).clone()
    model.hparams.update(hip_encode_dtype='bf16', hip_decode_dtype='bf16')
    with pytest.warns(UserWarning, match='batch-norm') as rec:
        got = pixel_stats_device(model, x, 0)
        again = pixel_stats_device(model, x[:5], 0)
    assert len([w for w in rec if 'bf16 decoding' in str(w.message)]) == 1
    assert len([w for w in rec if 'bf16 encoding' in str(w.message)]) <= 1
    assert len(rec) <= 2
    assert torch.equal(got, want) and torch.equal(again, want5)


@pytest.mark.parametrize('n', TRIALS)
@pytest.mark.parametrize('model_class', CLASSES)
def test_sum_over_pixels_is_the_sum_over_frames_of_frame_errors(model_class, n):
    """fp32 lane, with masks.  bn_frame_sq_err sums a frame's D <= 61440 fp32 terms in a tree at most 28 roundings of
    2^-24 deep (16 in a thread, 6 in a wave, 2 across waves, up to 15 partials -- each on non-negative terms), the sum
    of the frames' scores here is float64: 28 * 2^-24 = 1.7e-6 < 2e-6 relative."""
    model, x, kwargs, labels, dim = _case(model_class, n)
    d = int(np.prod(dim))
    for mask, _ in _masks(dim, n, 8)[1:]:
        md = mask.to(DEV)
        sse = float(pixel_stats_device(model, x, 0, md, labels=labels)[0].sum())
        fe = float(frame_errors_device(model, x, 0, md, labels=labels).double().sum()) * d
        print('PIXEL-STATS-FIGURE %s N=%d: sum sse %.9g, sum frame errors * CHW %.9g, rel %.2e'
              % (model_class, n, sse, fe, abs(sse - fe) / fe))
        assert abs(sse - fe) <= 2e-6 * fe


@pytest.mark.parametrize('keys', [{}, {'hip_encode_dtype': 'bf16', 'hip_decode_dtype': 'bf16'}], ids=['f32', 'bf16'])
@pytest.mark.parametrize('model_class', ['ae', 'vae'])
def test_nothing_else_moves(model_class, keys):
    """loss(), forward(), the exported latents and frame_errors_device give the same bits after calls of
    pixel_stats_device as before."""
    n = 24
    model, meta = _small(model_class, DIM, n)
    model.hparams.update(keys)
    xu = _frames(n, DIM, 5).to(DEV)
    xf = (xu.float() / 255).contiguous()
    mask = _masks(DIM, n, 1)[1][0].to(DEV)
    kwargs = {'dataset': 0, 'use_mean': True} if model_class == 'vae' else {'dataset': 0}

    def snapshot():
        out = {}
        model.eval()
        torch.manual_seed(1)
        out['loss'] = {k: float(v) for k, v in dict(model.loss({'images': xf[None]}, dataset=0,
                                                               accumulate_grad=False)).items()}
        with torch.no_grad():
            out['forward'] = [t.clone() for t in model(xf, **kwargs) if torch.is_tensor(t)]
        out['latents'] = encode_trial_device(model, xu, 0, None, 1024).clone()
        out['frame_errors'] = frame_errors_device(model, xu, 0, mask).clone()
        return out
    before = snapshot()
    a = pixel_stats_device(model, xu, 0, mask)
    pixel_stats_device(model, xf, 0, out=a)
    pixel_stats_device(model, xu, 0, chunk_size=7)
    after = snapshot()
    assert before['loss'] == after['loss']
    assert len(before['forward']) == len(after['forward']) > 0
    for s, t in zip(before['forward'], after['forward']):
        assert torch.equal(s, t)
    assert torch.equal(before['latents'], after['latents'])
    assert torch.equal(before['frame_errors'], after['frame_errors'])
    # no request of the other exporters is left open
    assert hf.frame_err_request() is None and hf.frame_u8_request() is None


# ------------------------------------------------------------------------------------------ 3: end to end
def test_export_pixel_stats_end_to_end(tmp_path):
    dim = [1, 64, 48]
    root = str(tmp_path)
    arch = load_handcrafted_arch(list(dim), 6, None, check_memory=False)
    hp = base_hparams(arch, 'ae', {'expt_dir': root, 'device': 'cuda'})
    torch.manual_seed(0)
    hip = BUILDERS['ae'](hp).to(DEV)
    hip.version = 0
    os.makedirs(os.path.join(root, 'version_0'))
    rng = np.random.default_rng(3)
    lens = [12, 67, 12, 67, 12, 67, 12, 67, 12, 67]
    ids, paths, trials, masks = [], [], [], []
    for s in range(2):
        trials.append([rng.integers(0, 256, size=(t,) + tuple(dim), dtype=np.uint8) for t in lens])
        # (the generator serves the mask of a trial's first frame for the whole trial: fractional, non-zero)
        masks.append([(rng.random((t,) + tuple(dim)) * 0.75 + 0.25).astype(np.float32) for t in lens])
        sess_dir = os.path.join(root, 'lab', 'expt', 'animal', 'sess%d' % s)
        write_npz_session(os.path.join(sess_dir, 'data.npz'), {'images': trials[s], 'masks': masks[s]})
        ids.append({'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess%d' % s})
        paths.append([os.path.join(sess_dir, 'data.npz')] * 2)

    def generator():
        return ConcatSessionsGenerator(root, ids, signals_list=[['images', 'masks']] * 2,
                                       transforms_list=[[None, None]] * 2, paths_list=paths, device='cuda',
                                       placement='host_u8', keep_in_memory=False,
                                       trial_splits={'train_tr': 5, 'val_tr': 1, 'test_tr': 1, 'gap_tr': 1})
    gen = generator()
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        files = export_pixel_stats(gen, hip)
    assert files == [os.path.join(root, 'version_0', 'lab_expt_animal_sess%d_pixel_stats.pkl' % s) for s in range(2)]
    error_files = export_frame_errors(generator(), hip)
    for s, path in enumerate(files):
        with open(path, 'rb') as fh:
            got = pickle.load(fh)
        with open(error_files[s], 'rb') as fh:
            errors = pickle.load(fh)['mse']
        assert sorted(got) == ['n_frames', 'stats', 'summary', 'trials']
        idxs = gen.datasets[s].batch_idxs
        used = [int(t) for k in ('train', 'val', 'test') for t in idxs[k]]
        assert 0 < len(used) < len(lens)
        for k in ('train', 'val', 'test'):
            assert np.array_equal(np.asarray(got['trials'][k]), np.asarray(idxs[k]))
            want = np.zeros((4,) + tuple(dim))
            for t in idxs[k]:
                y = torch.from_numpy(trials[s][int(t)])
                x_hat = get_reconstruction(hip, y.to(DEV), dataset=s)
                want += pixel_sums(x_hat, y, masks[s][int(t)][0])
            assert got['n_frames'][k] == sum(lens[int(t)] for t in idxs[k]) > 0
            assert_close(got['stats'][k], want, exact_w=False, name='export sess%d %s' % (s, k))
            full = summarise_pixel_stats(got['stats'][k], got['n_frames'][k])
            assert got['summary'][k] == {'mse': full['mse'], 'r2': full['r2']}
            assert np.isfinite(full['r2']) and not np.isnan(full['r2_map']).any()
        val = np.concatenate([errors[int(t)] for t in idxs['val']]).astype(np.float64)
        assert val.size == got['n_frames']['val']
        print('PIXEL-STATS-FIGURE export sess%d: val mse %.9g, mean of frame errors %.9g'
              % (s, got['summary']['val']['mse'], val.mean()))
        assert abs(got['summary']['val']['mse'] - val.mean()) <= 2e-6 * val.mean()


def test_fit_writes_the_pixel_stats(tmp_path):
    from behavenet_amd.fitting.training import fit
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    hp = base_hparams(arch, 'ae', None)
    hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 1, 'min_n_epochs': 0, 'val_check_interval': 1,
               'enable_early_stop': False, 'early_stop_history': 10, 'rng_seed_train': 0, 'export_latents': False,
               'export_pixel_stats': True, 'progress_bar': False, 'device': 'cuda'})
    os.makedirs(os.path.join(str(tmp_path), 'version_0'))
    sess = SyntheticSession(10, 12, dim, seed=0, trial_splits='8;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    torch.manual_seed(0)
    model = BUILDERS['ae'](hp).to(DEV)
    model.version = 0

    class Exp(object):
        version = 0

        def log(self, row):
            pass

        def save(self):
            pass
    best = fit(hp, model, gen, Exp(), method='ae')
    path = os.path.join(str(tmp_path), 'version_0', 'lab_expt_animal_sess_pixel_stats.pkl')
    assert os.path.exists(path) and not os.path.exists(path.replace('pixel_stats', 'latents'))
    with open(path, 'rb') as f:
        got = pickle.load(f)
    assert got['n_frames'] == {'train': 96, 'val': 12, 'test': 12}
    gen.reset_iterators('test')
    data, s_ = gen.next_batch('test')
    want = pixel_stats(best, data['images'][0], s_)
    np.testing.assert_allclose(got['stats']['test'], want, rtol=RTOL, atol=0)
