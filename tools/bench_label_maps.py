"""The input of a conditional encoder for one trial, two ways, alternated in ONE process (hparams['hip_label_maps']).

  (a) host    the one-hot maps are ALREADY resident on the device as a dense fp32 (T, L, H, W) tensor -- the host
              route at its most favourable, after its transform and its copy -- then what the model does per trial:
              ``u8_to_unit_float`` of the stored frames and ``torch.cat`` of frames and maps
  (b) device  ``_hip.cond_encoder_input`` on the stored uint8 frames and the (T, 2 L) coordinates: one pass

Both give the same tensor (checked, bit for bit).  Per route hipEvents bracket --iters calls walking --trials
different trials, after a warm-up of every trial; --reps such windows alternate, median and spread are printed, with
the bytes each route has to move by its algorithm (not measured traffic) and (b)'s effective bandwidth against the
8 TB/s peak.  Then the one-off costs (a) leaves out, per trial: ``MakeOneHot2D`` and the float32 cast on the host
(host clock), the copy of the dense maps from pageable memory (host clock around a synchronised copy) and the device
bytes the generator keeps.
    python tools/bench_label_maps.py [--frames 256] [--dim 1 128 128] [--maps 4] [--reps 5] [--iters 2000] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.data.transforms import MakeOneHot2D

PEAK_GBS = 8000.0


def algorithm_bytes(t, c, h, w, n_maps):
    """Bytes each route reads and writes by its algorithm."""
    frame, out = t * c * h * w, t * (c + n_maps) * h * w * 4
    maps = t * n_maps * h * w * 4
    host = frame + 4 * frame          # u8_to_unit_float: uint8 read, fp32 written
    host += 4 * frame + maps + out    # torch.cat: both operands read, the input written
    return {'host': host, 'device': frame + t * 2 * n_maps * 4 + out}


def event_window(fn, trials, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(trials[i % len(trials)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--dim', type=int, nargs=3, default=[1, 128, 128])
    ap.add_argument('--maps', type=int, default=4)
    ap.add_argument('--trials', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_label_maps.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    t, (c, h, w), n_maps = args.frames, args.dim, args.maps
    say('device: %s' % torch.cuda.get_device_name(0))
    say('trial: %d frames of %dx%dx%d uint8, %d label maps (%d coordinate columns)' % (t, c, h, w, n_maps, 2 * n_maps))
    rng = np.random.default_rng(0)
    transform = MakeOneHot2D(h, w)
    trials, host_s, copy_s = [], [], []
    for _ in range(args.trials):
        u8 = rng.integers(0, 256, size=(t, c, h, w), dtype=np.uint8)
        coords = np.concatenate([rng.uniform(-2, w + 1, size=(t, n_maps)), rng.uniform(-2, h + 1, size=(t, n_maps))],
                                axis=1).astype(np.float32)
        t0 = time.perf_counter()
        dense = np.ascontiguousarray(transform(coords).astype(np.float32))          # the generator's host work
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dense_dev = torch.from_numpy(dense).float().to('cuda')                     # ... and its pageable copy
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        host_s.append(t1 - t0)
        copy_s.append(t3 - t2)
        trials.append((torch.from_numpy(u8).to('cuda'), torch.from_numpy(coords).to('cuda'), dense_dev))

    def host(trial):
        return torch.cat((_hip.u8_to_unit_float(trial[0]), trial[2]), 1)

    def device(trial):
        return _hip.cond_encoder_input(trial[0], trial[1])
    fns = {'host': host, 'device': device}
    for trial in trials:                                         # warm-up of every trial, and the identity
        a, b = host(trial), device(trial)
        if not torch.equal(a, b):
            raise SystemExit('the two routes differ')
    say('the two routes give the same (%d, %d, %d, %d) fp32 tensor on all %d trials, bit for bit'
        % (t, c + n_maps, h, w, len(trials)))
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k in fns:
            ms[k].append(event_window(fns[k], trials, args.iters))
    nbytes = algorithm_bytes(t, c, h, w, n_maps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    what = {'host': '(a) maps resident + u8_to_unit_float + torch.cat', 'device': '(b) bn_cond_encoder_input, one pass'}
    for k in fns:
        say('%-50s %.1f us per trial (min %.1f max %.1f over %d windows of %d calls), %.1f MB by the algorithm'
            % (what[k], med[k] * 1e3, min(ms[k]) * 1e3, max(ms[k]) * 1e3, args.reps, args.iters, nbytes[k] / 1e6))
    gbs = nbytes['device'] / 1e9 / (med['device'] * 1e-3)
    say('(b) effective bandwidth: %.0f GB/s = %.0f %% of the %.0f GB/s peak; (a) / (b) = %.2f'
        % (gbs, 100 * gbs / PEAK_GBS, PEAK_GBS, med['host'] / med['device']))
    say('one-off costs per trial that (a) leaves out (medians over %d trials):' % len(trials))
    say('  MakeOneHot2D + float32 cast on the host: %.1f ms (float64 scratch %.1f MB)'
        % (statistics.median(host_s) * 1e3, t * n_maps * h * w * 8 / 1e6))
    dense_mb = t * n_maps * h * w * 4 / 1e6
    say('  copy of the dense maps from pageable memory: %.1f ms for %.1f MB' % (statistics.median(copy_s) * 1e3, dense_mb))
    say('  device bytes kept per trial by the generator: %.1f MB of maps against %.1f KB of coordinates'
        % (dense_mb, t * 2 * n_maps * 4 / 1e3))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
