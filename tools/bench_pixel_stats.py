"""Per-pixel error and moment sums of device-resident uint8 trials, three ways, alternated in ONE process.

  (a) host   ``get_reconstruction`` from images, then the four per-pixel sums in numpy float64: what a user can do
             without ``pixel_stats_device`` (every reconstructed fp32 frame crosses to the host)
  (b) fp32   ``pixel_stats_device``, no key: the model's fp32 forward + ``bn_pixel_stats_accum``
  (c) bf16   ``pixel_stats_device`` with both bf16 keys; the bf16 decoder writes its fp32 x_hat, the kernel reads it

Per shape every variant is warmed first, then windows of at least --window seconds alternate --reps times with a
device synchronise around each: ms per trial and frames/s (median, with the spread over the windows).  (b) and (c)
add onto ONE (4, C, H, W) accumulator on the device, as ``export_pixel_stats`` does per session and split.  Then
  (d) the kernel alone, hipEvents around --kernel-iters back-to-back launches on a random x_hat and the trial's
      frames, with the bytes it has to move (x_hat, the uint8 frames, the workspace written and read back, the
      accumulator read and written) against the 8 TB/s peak.
    python tools/bench_pixel_stats.py [--reps 5] [--window 1.0] [--kernel-iters 50]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as ev
from tools.bench_decode import SHAPES, build, event_ms, window

VARIANTS = ('host', 'fp32', 'bf16')
PEAK_GBS = 8000.0


def host_sums(x_hat, y_u8):
    """The four sums in numpy, float64 throughout."""
    t = y_u8.astype(np.float64) / 255
    d = x_hat.astype(np.float64) - t
    return np.stack([(d * d).sum(axis=0), np.full(t.shape[1:], float(t.shape[0])), t.sum(axis=0), (t * t).sum(axis=0)])


def variants(model, acc):
    def host(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        return host_sums(ev.get_reconstruction(model, y, dataset=0), y.cpu().numpy())

    def fp32(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        return ev.pixel_stats_device(model, y, 0, chunk_size=1024, out=acc['fp32'])

    def bf16(y):
        model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
        return ev.pixel_stats_device(model, y, 0, chunk_size=1024, out=acc['bf16'])
    return {'host': host, 'fp32': fp32, 'bf16': bf16}


def kernel_alone(name, y, iters):
    n, d = y.shape[0], y[0].numel()
    x_hat = torch.rand(tuple(y.shape), device='cuda')
    acc = torch.zeros((4,) + tuple(y.shape[1:]), dtype=torch.float64, device='cuda')
    ws = _hip.load().bn_pixel_stats_ws_bytes(n, d)
    t = event_ms(lambda: _hip.pixel_stats_accum(x_hat, y, None, acc), iters)
    mb = (x_hat.numel() * 4 + y.numel() + 2 * ws + 2 * acc.numel() * 8) / 1e6
    print('%-14s bn_pixel_stats_accum alone: %.1f us, %.1f MB (%.1f MB of it the workspace, written and read), '
          '%.0f GB/s = %.0f %% of the %.0f GB/s peak'
          % (name, t * 1e3, mb, 2 * ws / 1e6, mb / t, 100 * mb / t / PEAK_GBS, PEAK_GBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--kernel-iters', type=int, default=50)
    args = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for name, n, dim in SHAPES:
        model = build(dim)
        g = torch.Generator().manual_seed(1)
        trials = [torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8).to('cuda') for _ in range(8)]
        acc = {k: torch.zeros((4,) + tuple(dim), dtype=torch.float64, device='cuda') for k in VARIANTS[1:]}
        fns = variants(model, acc)
        ref = fns['host'](trials[0])
        for k in VARIANTS[1:]:                               # one trial each: against the host's sums
            got = fns[k](trials[0]).cpu().numpy()
            print('%-14s %-8s max |sse - host sse| / max sse = %.2e, moments %.2e'
                  % (name, k, abs(got[0] - ref[0]).max() / ref[0].max(), abs(got[1:] - ref[1:]).max() / ref[1:].max()))
        for k in VARIANTS:                                   # warm every variant on every trial
            for t in trials:
                fns[k](t)
        torch.cuda.synchronize()
        ms = {k: [] for k in VARIANTS}
        for _ in range(args.reps):
            for k in VARIANTS:
                ms[k].append(window(fns[k], trials, args.window))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in VARIANTS:
            print('%-14s %-8s %.4f ms per trial (min %.4f max %.4f over %d windows), %.0f frames/s'
                  % (name, k, med[k], min(ms[k]), max(ms[k]), args.reps, n / med[k] * 1e3))
        print('%-14s host / fp32 = %.2f, host / bf16 = %.2f' % (name, med['host'] / med['fp32'],
                                                                med['host'] / med['bf16']))
        kernel_alone(name, trials[0], args.kernel_iters)


if __name__ == '__main__':
    main()
