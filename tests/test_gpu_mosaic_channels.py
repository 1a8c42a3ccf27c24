"""``bn_frame_mosaic_ch_u8``: a range of channels side by side in every panel of the mosaic (csrc/frame_mosaic.hip).

Direct C calls on operands between guard bands, the output pre-filled with a sentinel; every comparison is
``torch.equal`` against ``tests/point_path_refs.mosaic_channels_rule``, the header's rule one sub-panel at a time, for
fp32 frames (with the half-way values, NaN and infinities of ``with_specials``) and uint8 frames.  The shapes are the
smallest at which the routes differ: 20-column panels, whose 16-byte segments straddle sub-panels and whose rows are a
multiple of 16 bytes only for some ``n_ch`` (byte gathers under 16-byte stores, and byte stores), and 32-column
panels, where every segment lies in one sub-panel (16-byte loads).  With ``n_ch == 1`` the bytes are those of
``bn_frame_mosaic_u8`` on every case."""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from tests import point_path_refs as refs
from tests import traversal_refs
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_reconstructions import SENTINEL
from tests.test_gpu_traversals import _call, _frames, _out, _place, _place_src

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2

SRC_322 = [[[4, -1], [0, 4]], [[3, 3], [9, 1]], [[2, 0], [-1, -1]]]          # -1, repeats and an index >= p
SRC_111 = [[[1]]]


def _call_ch(fd, src_d, ch0, n_ch, crop, out, dims=None, src_shape=None):
    p, c, h, w = dims or fd.shape
    y_min, x_min, hc, wc = (0, 0, h, w) if crop is None else crop
    t, r, cc = src_shape or src_d.shape
    return _hip.load().bn_frame_mosaic_ch_u8(fd.data_ptr(), int(fd.dtype == torch.uint8), p, c, h, w, ch0, n_ch, y_min,
                                             x_min, hc, wc, src_d.data_ptr(), t, r, cc, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)


def _check(frames, src, ch0, n_ch, crop=None, in_off=0, out_off=0):
    src = np.asarray(src, dtype=np.int32)
    want = refs.mosaic_channels_rule(frames, src, ch0, n_ch, crop)
    fd, sd = _place(frames, in_off), _place_src(src)
    out, whole = _out(want.shape, out_off)
    assert _call_ch(fd, sd, ch0, n_ch, crop, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(want)), (frames.shape, ch0, n_ch, crop, in_off, out_off)
    n = want.size
    assert bool((whole[:out_off] == SENTINEL).all()) and bool((whole[out_off + n:] == SENTINEL).all())
    if n_ch == 1:          # the old entry point writes the same bytes
        old, whole_old = _out(want.shape, out_off)
        assert _call(fd, sd, ch0, crop, old) == 0
        torch.cuda.synchronize()
        assert torch.equal(old, out)
        assert bool((whole_old[:out_off] == SENTINEL).all()) and bool((whole_old[out_off + n:] == SENTINEL).all())
    return want


CASES = [  # name, (P, C, H, W), (ch0, n_ch), crop (y_min, x_min, Hc, Wc)
    ('20 columns 0+1', (5, 3, 12, 20), (0, 1), None),
    ('20 columns 0+2', (5, 3, 12, 20), (0, 2), None),
    ('20 columns 0+3', (5, 3, 12, 20), (0, 3), None),
    ('20 columns 1+1', (5, 3, 12, 20), (1, 1), None),
    ('20 columns 1+2', (5, 3, 12, 20), (1, 2), None),
    ('32 columns 0+1', (4, 2, 16, 32), (0, 1), None),
    ('32 columns 0+2', (4, 2, 16, 32), (0, 2), None),
    ('32x32 1+2', (6, 3, 32, 32), (1, 2), None),
    ('past the right and bottom edges', (6, 3, 32, 32), (1, 2), (20, 16, 16, 32)),
    ('past the edges, 20 columns', (5, 3, 12, 20), (0, 3), (5, 9, 10, 16)),
    ('x_min off a 16-byte boundary', (6, 3, 32, 32), (0, 3), (3, 5, 16, 16)),
    ('x_min on a 16-byte boundary', (6, 3, 32, 32), (0, 3), (3, 16, 16, 16)),
]


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_kernel_against_the_rule(case, u8):
    name, shape, (ch0, n_ch), crop = case
    frames = _frames(shape, len(name), u8)
    for src in (SRC_322, SRC_111):
        want = _check(frames, src, ch0, n_ch, crop)
        hc, wc = shape[2:] if crop is None else crop[2:]
        assert want.shape == (len(src), len(src[0]) * hc, len(src[0][0]) * n_ch * wc)
        if name.startswith('past the'):          # the last row and column lie outside the frame
            assert not want[:, -1].any() and not want[:, :, -1].any() and want.any()
    if n_ch > 1:          # the sub-panels of a panel are different channels of ONE frame
        one = refs.mosaic_channels_rule(frames, SRC_111, ch0, n_ch, crop)[0]
        wc = one.shape[1] // n_ch
        for q in range(n_ch):
            assert np.array_equal(one[:, q * wc:(q + 1) * wc],
                                  traversal_refs.mosaic_index_rule(frames, SRC_111, ch0 + q, crop)[0])


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
def test_offset_operands_give_the_same_bytes(u8):
    """Frames and output 4 bytes and 1 byte off their 16-byte boundary (fp32 frames cannot sit 1 byte off)."""
    four = 4 if u8 else 1          # (offsets of the frames are in elements)
    offsets = [(four, 0), (0, 4), (0, 1), (four, 4), (four, 1)] + ([(1, 0), (1, 1)] if u8 else [])
    for name, shape, (ch0, n_ch), crop in (CASES[1], CASES[6], CASES[7], CASES[8]):
        frames = _frames(shape, 7, u8)
        want = _check(frames, SRC_322, ch0, n_ch, crop)
        for in_off, out_off in offsets:
            got = _check(frames, SRC_322, ch0, n_ch, crop, in_off, out_off)
            assert np.array_equal(got, want), (name, in_off, out_off)


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'u8'])
def test_thousands_of_channels(u8):
    """(panel, channel) of a sub-panel far from the few channels of a camera: 255 and 256 panels of 4099 one-pixel
    channels (rows of 1,045,245 bytes, stored byte by byte, and of 1,049,344, stored 16 at a time) and 65536
    channels in one panel."""
    for c, cc in [(4099, 255), (4099, 256), (65536, 1)]:
        frames = _frames((3, c, 1, 1), c + cc, u8)
        src = np.random.default_rng(cc).integers(-1, 4, size=(1, 1, cc)).astype(np.int32)          # -1 .. 3: 3 is >= p
        grey = frames if u8 else refs.quantise_u8(frames)
        shown = (src[0, 0] >= 0) & (src[0, 0] < 3)
        want = np.where(shown[:, None], grey[np.where(shown, src[0, 0], 0), :, 0, 0], 0).astype(np.uint8)
        out, whole = _out((1, 1, cc * c))
        assert _call_ch(_place(frames), _place_src(src), 0, c, None, out) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(want.reshape(1, 1, cc * c))), (c, cc)
        assert bool((whole[cc * c:] == SENTINEL).all())


def test_empty_counts_and_refusals_write_nothing():
    frames = _place(_frames((3, 2, 8, 12), 1, False))
    frames_u8 = _place(_frames((3, 2, 8, 12), 1, True))
    src = _place_src(np.zeros((2, 2, 2)))
    out, whole = _out((2, 16, 48))
    for shape in [(0, 2, 2), (2, 0, 2), (2, 2, 0)]:          # an empty result: nothing is launched
        assert _call_ch(frames, src, 0, 2, None, out, src_shape=shape) == 0
    big = 1 << 30
    refused = [
        dict(n_ch=0), dict(n_ch=-1), dict(ch0=-1), dict(ch0=-1, n_ch=3),          # the channel range
        dict(ch0=0, n_ch=3), dict(ch0=1, n_ch=2), dict(ch0=2, n_ch=1), dict(ch0=1, n_ch=(1 << 31) - 1),
        dict(crop=(0, 0, 8, big // 2)),                                # cc n_ch wc = 2^31 columns, cc wc = 2^30
        dict(crop=(0, 0, 8, big), n_ch=1),                             # ... and the old limits
        dict(crop=(-1, 0, 4, 4)), dict(crop=(0, -1, 4, 4)), dict(crop=(0, 0, 0, 4)), dict(crop=(0, 0, 4, 0)),
        dict(dims=(3, 0, 8, 12)), dict(dims=(3, 2, 0, 12)), dict(dims=(3, 2, 8, 0)), dict(dims=(-1, 2, 8, 12)),
        dict(src_shape=(-1, 2, 2)), dict(src_shape=(2, -2, 2)), dict(src_shape=(2, 2, -2)),
        dict(src_shape=(big, 2, 2)), dict(crop=(0, 0, big, 12), src_shape=(1, 2, 2)),
        dict(crop=(0, 0, 1, 2048), src_shape=(big, 1, 1)),             # 2^30 rows of one thread row each
    ]
    for kw in refused:
        kw = dict(dict(ch0=0, n_ch=2, crop=None), **kw)
        for fd in (frames, frames_u8):
            assert _call_ch(fd, src, kw['ch0'], kw['n_ch'], kw['crop'], out, kw.get('dims'),
                            kw.get('src_shape')) == E_SHAPE, kw
    lib, st = _hip.load(), torch.cuda.current_stream().cuda_stream
    args = (3, 2, 8, 12, 0, 2, 0, 0, 8, 12)
    assert lib.bn_frame_mosaic_ch_u8(None, 0, *args, src.data_ptr(), 2, 2, 2, out.data_ptr(), st) == E_ARG
    assert lib.bn_frame_mosaic_ch_u8(frames.data_ptr(), 0, *args, None, 2, 2, 2, out.data_ptr(), st) == E_ARG
    assert lib.bn_frame_mosaic_ch_u8(frames.data_ptr(), 0, *args, src.data_ptr(), 2, 2, 2, None, st) == E_ARG
    assert lib.bn_frame_mosaic_ch_u8(frames.data_ptr() + 2, 0, *args, src.data_ptr(), 2, 2, 2, out.data_ptr(),
                                     st) == E_SHAPE
    assert lib.bn_frame_mosaic_ch_u8(frames.data_ptr(), 0, *args, src.data_ptr() + 2, 2, 2, 2, out.data_ptr(),
                                     st) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())
    # without frames every panel is blank and `frames` may be NULL
    assert lib.bn_frame_mosaic_ch_u8(None, 0, 0, 2, 8, 12, 0, 2, 0, 0, 8, 12, src.data_ptr(), 2, 2, 2, out.data_ptr(),
                                     st) == 0
    torch.cuda.synchronize()
    assert not bool(out.any()) and bool((whole[out.numel():] == SENTINEL).all())


def test_wrapper():
    for u8 in (False, True):
        frames = _frames((5, 3, 8, 16), 3, u8)
        src = [[[4, -1, 4], [0, 1, 2]], [[3, 3, 3], [-1, -1, -1]]]
        fd = _place(frames)
        crop = (2, 4, 6, 16)
        for ch, (ch0, n_ch) in [(None, (0, 3)), ((1, 2), (1, 2)), ((2, 1), (2, 1)), ([0, 2], (0, 2))]:
            got = _hip.frame_mosaic_u8(fd, src, ch=ch, crop=crop)
            assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (2, 12, 3 * n_ch * 16)
            assert np.array_equal(got.cpu().numpy(), refs.mosaic_channels_rule(frames, src, ch0, n_ch, crop))
        # an int is the old entry point, one channel wide
        one = _hip.frame_mosaic_u8(fd, src, ch=2, crop=crop)
        assert torch.equal(one, _hip.frame_mosaic_u8(fd, src, ch=(2, 1), crop=crop))
        assert np.array_equal(one.cpu().numpy(), traversal_refs.mosaic_index_rule(frames, src, 2, crop))
        grid = _hip.frame_mosaic_u8(fd, src[0], ch=None)          # (R, Cc): one image
        assert np.array_equal(grid.cpu().numpy(), refs.mosaic_channels_rule(frames, [src[0]], 0, 3))
        for ch, what in [((2, 2), 'channels'), ('all', 'ch must be'), (3, 'channel 3')]:
            with pytest.raises(ValueError, match=what):
                _hip.frame_mosaic_u8(fd, src, ch=ch)
