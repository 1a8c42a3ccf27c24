"""Per-frame reconstruction errors of device-resident uint8 trials, four ways, alternated in ONE process.

  (a) host     ``get_reconstruction`` from images, then the per-frame MSE in numpy: what there was before
               ``frame_errors_device`` (every reconstructed frame crosses to the host)
  (b) fp32     ``frame_errors_device``, no key: the model's fp32 forward + ``bn_frame_sq_err``
  (c) unfused  both bf16 keys; the bf16 decoder writes x_hat, ``bn_frame_sq_err`` reads it back
  (d) fused    both bf16 keys as ``frame_errors_device`` runs them: the layer onto the frame scores in its epilogue
               (``bn_convT2d_last_bf16_sqerr``), x_hat is never written

Per shape every variant is warmed first, then windows of at least --window seconds alternate --reps times with a
device synchronise around each: ms per trial and frames/s (median, with the spread over the windows).  (b) to (d)
leave their (T,) result on the device, as ``export_frame_errors`` keeps it until its one transfer at the end.  Then the
two last-layer variants alone, hipEvents around --layer-iters back-to-back launches on operands of the layer's shapes
(random activations, the model's weights, the trial's frames), with the bytes each has to move.
    python tools/bench_frame_errors.py [--reps 5] [--window 1.0] [--layer-iters 50]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.fitting import eval as ev
from tools.bench_decode import SHAPES, build, event_ms, window

VARIANTS = ('host', 'fp32', 'unfused', 'fused')


def variants(model):
    def host(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        x_hat = ev.get_reconstruction(model, y, dataset=0)
        return ((x_hat - y.cpu().numpy().astype(np.float32) / 255) ** 2).reshape(y.shape[0], -1).mean(axis=1)

    def fp32(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        return ev.frame_errors_device(model, y, 0, chunk_size=1024)

    def unfused(y):
        with hf.encode_precision('bf16'), hf.decode_precision('bf16'):
            return ev._frame_errors_device(model, y, 0, None, None, None, 1024, fused=False)

    def fused(y):
        model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
        return ev.frame_errors_device(model, y, 0, chunk_size=1024)
    return {'host': host, 'fp32': fp32, 'unfused': unfused, 'fused': fused}


def last_layer(name, model, y, iters):
    dec = model.decoding
    layer = dec._plan[-1]
    n = y.shape[0]
    w, b = [p.detach().contiguous() for p in dec._stack_params(None)[-2:]]
    g = layer.geom(n)
    if not _hip.convT2d_bf16_ok(g, last=True):
        print('%-14s the last layer is not the vector-unit layer: nothing to compare' % name)
        return
    a16 = (torch.randn((n, layer.hin, layer.win, layer.cin), device='cuda') * 0.5).to(torch.bfloat16)
    d = y[0].numel()
    x_hat = torch.empty((n, layer.cout, layer.hout, layer.wout), device='cuda')
    out = torch.empty((n,), device='cuda')

    def two():
        _hip.convT2d_last_bf16(a16, w, b, g, layer.act, hf.LRELU_SLOPE, out=x_hat)
        _hip.frame_sq_err(x_hat, y, None, 1.0 / d, out=out)
    t_layer = event_ms(lambda: _hip.convT2d_last_bf16(a16, w, b, g, layer.act, hf.LRELU_SLOPE, out=x_hat), iters)
    t_err = event_ms(lambda: _hip.frame_sq_err(x_hat, y, None, 1.0 / d, out=out), iters)
    t_two = event_ms(two, iters)
    t_one = event_ms(lambda: _hip.convT2d_last_bf16_sqerr(a16, w, b, y, None, g, layer.act, hf.LRELU_SLOPE, 1.0 / d,
                                                          out=out), iters)
    common = a16.numel() * 2 + w.numel() * 4 + y.numel()
    mb_two, mb_one = (common + 2 * x_hat.numel() * 4) / 1e6, common / 1e6
    print('%-14s last layer alone: bn_convT2d_last_bf16 %.1f us + bn_frame_sq_err %.1f us, back to back %.1f us '
          '(%.1f MB, %.0f GB/s); bn_convT2d_last_bf16_sqerr %.1f us (%.1f MB, %.0f GB/s); unfused / fused = %.2f'
          % (name, t_layer * 1e3, t_err * 1e3, t_two * 1e3, mb_two, mb_two / t_two, t_one * 1e3, mb_one,
             mb_one / t_one, t_two / t_one))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--layer-iters', type=int, default=50)
    args = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for name, n, dim in SHAPES:
        model = build(dim)
        g = torch.Generator().manual_seed(1)
        trials = [torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8).to('cuda') for _ in range(8)]
        fns = variants(model)
        res = {}
        for k in VARIANTS:                                   # warm every variant on every trial
            for t in trials:
                res[k] = fns[k](t)
        torch.cuda.synchronize()
        ref = res['host']
        for k in VARIANTS[1:]:
            got = res[k].cpu().numpy()
            print('%-14s %-8s max |mse - host mse| / max mse = %.2e' % (name, k, abs(got - ref).max() / ref.max()))
        ms = {k: [] for k in VARIANTS}
        for _ in range(args.reps):
            for k in VARIANTS:
                ms[k].append(window(fns[k], trials, args.window))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in VARIANTS:
            print('%-14s %-8s %.4f ms per trial (min %.4f max %.4f over %d windows), %.0f frames/s'
                  % (name, k, med[k], min(ms[k]), max(ms[k]), args.reps, n / med[k] * 1e3))
        print('%-14s host / fp32 = %.2f, host / fused = %.2f, unfused / fused = %.3f (slowest fused window against '
              'fastest unfused window: %.3f)' % (name, med['host'] / med['fp32'], med['host'] / med['fused'],
                                                 med['unfused'] / med['fused'], min(ms['unfused']) / max(ms['fused'])))
        last_layer(name, model, trials[0], args.layer_iters)


if __name__ == '__main__':
    main()
