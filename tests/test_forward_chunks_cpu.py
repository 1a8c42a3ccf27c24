"""``fitting.eval._forward_chunks``, the one chunked forward pass behind ``frame_errors_device``,
``reconstruct_trial_device``, ``pixel_stats_device`` and ``reconstruction_movie_device``, and ``_trial_masks``, on a
recording model with CPU tensors.  No GPU."""

import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting import eval as ev

C, H, W = 2, 3, 4


class _Recorder(torch.nn.Module):
    """``forward`` notes what it was given and the state it ran in, and returns ``(x * 0.5, None)``."""

    def __init__(self, model_class='ae', model_type='conv'):
        super().__init__()
        self.hparams = {'model_class': model_class, 'model_type': model_type}
        self.calls = []
        self.train()

    def forward(self, x, **kwargs):
        self.calls.append({'shape': tuple(x.shape), 'dtype': x.dtype, 'first': float(x.flatten()[0]), 'kwargs': kwargs,
                           'training': self.training, 'grad': torch.is_grad_enabled(),
                           'requests': (hf.frame_err_request(), hf.frame_u8_request())})
        return x * 0.5, None


def _frames(t, dtype=torch.float32):
    """Frame n is filled with n, so a chunk's first value names its first frame."""
    y = torch.arange(t, dtype=torch.float32).view(t, 1, 1, 1).expand(t, C, H, W)
    return y.to(dtype).contiguous()


def _walk(model, y, chunk_size, labels=None, labels_2d=None, request=None, x=None, sess=0):
    seen = []
    ev._forward_chunks('who', model, y, sess, labels, labels_2d, chunk_size,
                       lambda beg, end, x_hat, req: seen.append((beg, end, x_hat, req)), request, x)
    return seen


@pytest.mark.parametrize('t,chunk_size,bounds', [(5, 2, [(0, 2), (2, 4), (4, 5)]), (4, 4, [(0, 4)]), (4, 9, [(0, 4)]),
                                                 (0, 3, [])])
def test_chunk_bounds(t, chunk_size, bounds):
    model, y = _Recorder(), _frames(t)
    seen = _walk(model, y, chunk_size, sess=3)
    assert [(beg, end) for beg, end, _, _ in seen] == bounds
    assert [(int(c['first']), c['shape']) for c in model.calls] == [(beg, (end - beg, C, H, W)) for beg, end in bounds]
    for (beg, end, x_hat, req), call in zip(seen, model.calls):
        assert torch.equal(x_hat, y[beg:end] * 0.5) and req is None
        assert call['kwargs'] == {'dataset': 3}


def test_conditional_labels_arrive_sliced_to_the_chunk():
    y = _frames(5)
    labels, labels_2d = torch.arange(10.0).view(5, 2), torch.arange(20.0).view(5, 4)
    model = _Recorder('cond-ae')
    _walk(model, y, 2, labels, labels_2d)
    for (beg, end), call in zip([(0, 2), (2, 4), (4, 5)], model.calls):
        assert torch.equal(call['kwargs']['labels'], labels[beg:end])
        assert torch.equal(call['kwargs']['labels_2d'], labels_2d[beg:end])
    model = _Recorder('cond-ae')
    _walk(model, y, 2, labels, None)
    assert [c['kwargs']['labels_2d'] for c in model.calls] == [None] * 3
    model = _Recorder('ae')
    _walk(model, y, 2, labels, labels_2d)
    assert all(set(c['kwargs']) == {'dataset'} for c in model.calls)


@pytest.mark.parametrize('model_class,mean', [('vae', True), ('beta-tcvae', True), ('ps-vae', True), ('msps-vae', True),
                                              ('cond-vae', True), ('ae', False), ('cond-ae', False),
                                              ('cond-ae-msp', False)])
def test_posterior_mean_for_the_variational_classes(model_class, mean):
    model = _Recorder(model_class)
    _walk(model, _frames(3), 2, labels=torch.zeros(3, 2))
    assert len(model.calls) == 2
    for call in model.calls:
        assert ('use_mean' in call['kwargs']) == mean and call['kwargs'].get('use_mean', True) is True


def test_stored_frames_are_converted_only_where_the_model_needs_floats(monkeypatch):
    converted = []

    def convert(u8):
        converted.append(tuple(u8.shape))
        return u8.float() / 255

    monkeypatch.setattr(_hip, 'u8_to_unit_float', convert)
    y = _frames(5, torch.uint8)
    # a conv model without label maps, or with label COORDINATES, takes the uint8 frames: no library call
    for labels_2d in (None, torch.zeros(5, 4)):
        model = _Recorder('cond-ae')
        _walk(model, y, 2, torch.zeros(5, 2), labels_2d)
        assert converted == [] and [c['dtype'] for c in model.calls] == [torch.uint8] * 3
    # dense label maps and the linear models want floats: ONE conversion of the whole trial
    for model, labels_2d in ((_Recorder('cond-ae'), torch.zeros(5, 2, H, W)), (_Recorder('ae', 'linear'), None)):
        del converted[:]
        _walk(model, y, 2, torch.zeros(5, 2), labels_2d)
        assert converted == [(5, C, H, W)] and [c['dtype'] for c in model.calls] == [torch.float32] * 3
    # ... unless the caller has the copy already
    del converted[:]
    model = _Recorder('ae', 'linear')
    _walk(model, y, 2, x=y.float() / 255)
    assert converted == [] and [c['dtype'] for c in model.calls] == [torch.float32] * 3
    # float frames go in as they are
    model = _Recorder('ae', 'linear')
    _walk(model, _frames(5), 2)
    assert converted == [] and [c['dtype'] for c in model.calls] == [torch.float32] * 3


def test_eval_mode_and_no_grad_inside_forward():
    model = _Recorder()
    assert model.training and torch.is_grad_enabled()
    _walk(model, _frames(3), 2)
    assert [(c['training'], c['grad']) for c in model.calls] == [(False, False)] * 2
    assert torch.is_grad_enabled()


def test_validation_names_the_caller():
    model = _Recorder()
    with pytest.raises(ValueError, match='who: expected frames'):
        _walk(model, _frames(3)[0], 2)
    with pytest.raises(ValueError, match='who: frames must be uint8 or float32'):
        _walk(model, _frames(3).double(), 2)
    with pytest.raises(ValueError, match='Invalid model class neural-ae'):
        _walk(_Recorder('neural-ae'), _frames(3), 2)
    assert model.calls == [] and model.training


def test_a_request_is_open_for_the_model_call_and_closed_in_per_chunk():
    y = _frames(5)
    model, opened = _Recorder(), []

    def request(beg, end):
        opened.append((beg, end))
        return hf.scoring_frames(y[beg:end], None, 0.25)

    def per_chunk(beg, end, x_hat, req):
        assert hf.frame_err_request() is None and hf.frame_u8_request() is None
        assert isinstance(req, hf.FrameErrRequest) and req.target.shape[0] == end - beg and req.scale == 0.25
        assert req is model.calls[-1]['requests'][0]

    ev._forward_chunks('who', model, y, 0, None, None, 2, per_chunk, request)
    assert opened == [(0, 2), (2, 4), (4, 5)] and len(model.calls) == 3
    assert all(c['requests'][0] is not None and c['requests'][1] is None for c in model.calls)

    model = _Recorder()
    seen = _walk(model, y, 5, request=lambda beg, end: hf.quantising_frames())
    assert isinstance(seen[0][3], hf.FrameU8Request) and seen[0][3] is model.calls[0]['requests'][1]
    assert hf.frame_u8_request() is None


@pytest.mark.parametrize('request_of', [lambda y: (lambda beg, end: hf.scoring_frames(y[beg:end], None, 1.0)),
                                        lambda y: (lambda beg, end: hf.quantising_frames()), lambda y: None])
def test_nothing_stays_open_after_an_exception_from_per_chunk(request_of):
    y = _frames(5)
    model = _Recorder()

    def per_chunk(beg, end, x_hat, req):
        if beg:
            raise RuntimeError('the second chunk')

    with pytest.raises(RuntimeError, match='the second chunk'):
        with hf.encode_precision('bf16'), hf.decode_precision('bf16'):
            ev._forward_chunks('who', model, y, 0, None, None, 2, per_chunk, request_of(y))
    assert len(model.calls) == 2
    assert hf.frame_err_request() is None and hf.frame_u8_request() is None
    assert hf.encode_dtype() == 'f32' and hf.decode_dtype() == 'f32'
    assert torch.is_grad_enabled()


def test_trial_masks():
    one = torch.rand(C, H, W)
    assert ev._trial_masks(None, _frames(3)) == (None, False)
    for t in (1, 3):
        for given in (one, one[None]):
            masks, per_frame = ev._trial_masks(given, _frames(t))
            assert not per_frame and masks.shape == (C, H, W) and torch.equal(masks, one)
    each = torch.rand(3, C, H, W)
    masks, per_frame = ev._trial_masks(each, _frames(3))
    assert per_frame and torch.equal(masks, each)
    # integer masks come back as float32, strided ones contiguous
    masks, per_frame = ev._trial_masks((each > 0.5).to(torch.int64), _frames(3))
    assert per_frame and masks.dtype == torch.float32 and torch.equal(masks, (each > 0.5).float())
    masks, per_frame = ev._trial_masks((one > 0.5).to(torch.uint8)[None], _frames(3))
    assert not per_frame and masks.dtype == torch.float32 and torch.equal(masks, (one > 0.5).float())
    masks, _ = ev._trial_masks(torch.rand(C, H, 2 * W)[:, :, ::2], _frames(3))
    assert masks.is_contiguous() and masks.shape == (C, H, W)
