"""Reconstruction movies, the host side (no GPU): the yardstick of tests/recon_movie_refs.py against itself, the
contraction probes, the strided layout of a movie of two rows, and every argument error of
``_hip.recon_panels_u8`` that is raised before anything reaches the device."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as bn_eval
from tests import recon_movie_refs as refs
from tests.recon_u8_refs import SPECIALS, quantise_u8

# the kernel's cases (tests/test_gpu_recon_movie.py) and the shapes of its placement, two-row and probe cases
SHAPES = refs.SHAPES + [(2, 1, 16, 16), (5, 1, 8, 16), (1, 1, 8, 16)]


@pytest.mark.parametrize('show_orig', [True, False], ids=['orig', 'blank'])
@pytest.mark.parametrize('mask_form', refs.MASK_FORMS)
@pytest.mark.parametrize('recon_u8', [False, True], ids=['recon-fp32', 'recon-u8'])
@pytest.mark.parametrize('orig_u8', [False, True], ids=['orig-fp32', 'orig-u8'])
def test_the_two_strips_agree(orig_u8, recon_u8, mask_form, show_orig):
    for shape in SHAPES:
        n, c, h, w = shape
        orig, recon, mask = refs.operands(shape, sum(shape), orig_u8, recon_u8, mask_form)
        a = refs.strip_blocks(orig, recon, mask, show_orig)
        b = refs.strip_index_rule(orig, recon, mask, show_orig)
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (n, h, 3 * c * w)
        assert np.array_equal(a, b), shape
        if not show_orig:
            assert not a[:, :, :c * w].any()
        elif orig_u8 and mask_form == 'none':          # the stored bytes themselves, channels side by side
            for k in range(c):
                assert np.array_equal(a[:, :, k * w:(k + 1) * w], orig[:, k])
        if recon_u8:
            for k in range(c):
                assert np.array_equal(a[:, :, (c + k) * w:(c + k + 1) * w], recon[:, k])


def test_special_values():
    """NaN is black in every panel it reaches, infinities saturate, the half-way values go to the even level; an
    original equal to its reconstruction gives the mid grey 128 (0.5 * 255 = 127.5 rounds to the even level)."""
    vals = np.array([v for v, _ in SPECIALS], dtype=np.float32)
    levels = np.array([g for _, g in SPECIALS], dtype=np.uint8)
    orig = vals.reshape(1, 1, 1, -1)
    zeros = np.zeros_like(orig)
    for fn in (refs.strip_blocks, refs.strip_index_rule):
        strip = fn(orig, zeros)
        k = vals.size
        assert np.array_equal(strip[0, 0, :k], levels) and not strip[0, 0, k:2 * k].any()
        with np.errstate(invalid='ignore', over='ignore'):
            assert np.array_equal(strip[0, 0, 2 * k:], quantise_u8(np.float32(0.5) + vals))
        assert strip[0, 0, 2 * k + int(np.flatnonzero(np.isnan(vals))[0])] == 0
        same = fn(np.full((1, 1, 1, 4), 77, np.uint8), np.full((1, 1, 1, 4), 77, np.uint8))
        assert np.array_equal(same[0, 0], [77] * 8 + [128] * 4)
        # the mask reaches the original and the residual, not the reconstruction
        masked = fn(np.full((1, 1, 1, 2), 255, np.uint8), np.full((1, 1, 1, 2), 51, np.uint8),
                    np.array([[[0.0, 1.0]]], dtype=np.float32))
        assert np.array_equal(masked[0, 0], [0, 255, 51, 51, quantise_u8(np.float32(0.5) - np.float32(51) / 255), 255])


def test_contraction_probes():
    o_u8, m, r = refs.contraction_probes(1)
    assert o_u8.dtype == np.uint8 and m.dtype == r.dtype == np.float32 and o_u8.shape == m.shape == r.shape == (64,)
    assert ((m > 0) & (m < 1)).all() and ((r >= 0) & (r <= 1)).all()
    o = o_u8.astype(np.float32) / np.float32(255)
    separate = quantise_u8(np.float32(0.5) + (o * m - r))
    once = quantise_u8(np.float32(0.5) + (o.astype(np.float64) * m - r.astype(np.float64)).astype(np.float32))
    assert (np.abs(separate.astype(int) - once.astype(int)) == 1).all()
    # seeded: the same probes every time, others under another seed
    again = refs.contraction_probes(1)
    assert all(np.array_equal(a, b) for a, b in zip((o_u8, m, r), again))
    assert not np.array_equal(refs.contraction_probes(2)[2], r)
    # both restatements take the separately rounded steps on them
    orig, recon, mask = probe_case(o_u8, m, r)
    for fn in (refs.strip_blocks, refs.strip_index_rule):
        assert np.array_equal(fn(orig, recon, mask)[0].reshape(8, 3, 16)[:, 2].reshape(-1)[:64], separate)


def probe_case(o_u8, m, r, shape=(1, 1, 8, 16)):
    """The probes in the first pixels of a seeded case of ``shape`` with a per-frame mask."""
    orig, recon, mask = refs.operands(shape, 11, True, False, 'per-frame', specials=False)
    for arr, vals in ((orig, o_u8), (recon, r), (mask, m)):
        arr.reshape(-1)[:vals.size] = vals
    return orig, recon, mask


def test_two_rows_are_two_strips_along_the_height():
    shape = (5, 1, 8, 16)
    orig, recon, mask = refs.operands(shape, 5, True, False, 'one')
    recon_lin = refs.operands(shape, 6, True, True, 'none')[1]
    top = refs.strip_index_rule(orig, recon, mask)
    bottom = refs.strip_index_rule(orig, recon_lin, mask, show_orig=False)
    want = np.concatenate([top, bottom], axis=1)
    assert want.shape == (5, 16, 48)
    # row k of R sits at byte offset k H 3 C W of every frame of R H 3 C W bytes
    n, c, h, w = shape
    strip = 3 * c * h * w
    flat = np.zeros(n * 2 * strip, dtype=np.uint8)
    for k, rows in enumerate((top, bottom)):
        for i in range(n):
            flat[i * 2 * strip + k * strip:i * 2 * strip + (k + 1) * strip] = rows[i].reshape(-1)
    assert np.array_equal(flat.reshape(n, 2 * h, 3 * c * w), want)
    assert np.array_equal(refs.into_row(bottom, 1, 2, 0xAB)[:, h:], bottom)
    assert (refs.into_row(bottom, 1, 2, 0xAB)[:, :h] == 0xAB).all()
    assert not want[:, h:, :c * w].any()


def test_argument_errors_are_raised_on_the_host():
    f = torch.zeros((3, 2, 8, 12))
    u = torch.zeros((3, 2, 8, 12), dtype=torch.uint8)
    bad = [
        (dict(orig=f[0]), 'expected orig'), (dict(recon=f[0]), 'expected recon'),
        (dict(orig=np.zeros((3, 2, 8, 12), np.float32)), 'expected orig'),
        (dict(orig=f.double()), 'orig must be uint8 or float32'), (dict(recon=f.half()), 'recon must be uint8 or float32'),
        (dict(recon=f[:2]), 'share a shape'), (dict(recon=u[:, :, :, :8]), 'share a shape'),
        (dict(orig=f[:, :, :0], recon=f[:, :, :0]), 'pixels'),
        (dict(mask=u[0]), 'mask must be a float32'), (dict(mask=np.ones((2, 8, 12), np.float32)), 'mask must be a float32'),
        (dict(mask=f[0, 0]), 'expected a mask'), (dict(mask=f[:2]), 'expected a mask'), (dict(mask=f[:1]), 'expected a mask'),
        (dict(n_rows=0), 'row 0 of a movie of 0'), (dict(row=2, n_rows=2), 'row 2 of a movie of 2'),
        (dict(row=-1), 'row -1'),
        (dict(out=torch.zeros((3, 8, 72))), 'expected out uint8'),
        (dict(out=torch.zeros((3, 8, 72), dtype=torch.uint8), n_rows=2), 'expected out uint8'),
        (dict(out=torch.zeros((3, 8, 71), dtype=torch.uint8)), 'expected out uint8'),
        (dict(out=np.zeros((3, 8, 72), np.uint8)), 'expected out uint8'),
        (dict(orig=f.transpose(2, 3).contiguous().transpose(2, 3)), 'orig must be contiguous'),
        (dict(recon=u.transpose(0, 1).contiguous().transpose(0, 1)), 'recon must be contiguous'),
        (dict(mask=torch.zeros((2, 8, 24))[:, :, ::2]), 'mask must be contiguous'),
        (dict(out=torch.zeros((3, 8, 144), dtype=torch.uint8)[:, :, ::2]), 'out must be contiguous'),
        (dict(), 'expected orig on the GPU'),
    ]
    for kw, what in bad:
        kw = dict(dict(orig=f, recon=u), **kw)
        with pytest.raises(ValueError, match=what):
            _hip.recon_panels_u8(kw.pop('orig'), kw.pop('recon'), **kw)
    # the public functions refuse before they touch a model's parameters

    class _Stub(object):
        hparams = {'model_class': 'ae'}

        def parameters(self):
            raise AssertionError('the device was reached')

        def eval(self):
            raise AssertionError('the device was reached')
    with pytest.raises(ValueError, match='expected frames'):
        bn_eval.reconstruction_movie(_Stub(), f[0])
    with pytest.raises(ValueError, match='uint8 or float32'):
        bn_eval.reconstruction_movie(_Stub(), f.double())
    with pytest.raises(ValueError, match='expected masks'):
        bn_eval.reconstruction_movie(_Stub(), f, masks=torch.ones((2, 8, 11)))
    with pytest.raises(ValueError, match='expected masks'):
        bn_eval.reconstruction_movie(_Stub(), f, masks=torch.ones((2, 2, 8, 12)))
    with pytest.raises(ValueError, match='chunk_size'):
        bn_eval.reconstruction_movie(_Stub(), f, chunk_size=0)
    stub = _Stub()
    stub.hparams = {'model_class': 'ae', 'hip_decode_dtype': 'fp8'}
    with pytest.raises(ValueError, match='hip_decode_dtype'):
        bn_eval.reconstruction_movie(stub, f)
    stub.hparams = {'model_class': 'neural-ae'}
    with pytest.raises(ValueError, match='Invalid model class'):
        bn_eval.reconstruction_movie(_Stub(), f, extra_models=(stub,))


def test_the_symbol_is_declared_everywhere():
    assert 'bn_recon_panels_u8' in _hip.SIGNATURES
    restype, argtypes = _hip.SIGNATURES['bn_recon_panels_u8']
    assert len(argtypes) == 14
    assert {'reconstruction_movie', 'reconstruction_movie_device'} <= set(bn_eval.__all__)
    code = ('import sys; import behavenet_amd.plotting.ae_utils as m; assert m.__all__ == '
            '["make_ae_reconstruction_movie"]; sys.exit(int("matplotlib" in sys.modules))')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, '-c', code], cwd=repo).returncode == 0
