"""The latent traversal movie of a PS-VAE, tiled on the device (fitting.eval.traversal_movie, csrc/frame_mosaic.hip).

The workload: 16 latents x 30 steps x 5 base points at 2x128x128 on a default-architecture PS-VAE -- 2,400 decoded
points, a movie of 150 frames of 6 x 3 panels (two of them blank).

  (a) the mosaic launch alone, fp32 and uint8 frames: hipEvents around --iters launches, --reps windows alternated
      with the yardstick ``bn_unit_float_to_u8`` on the SAME byte count (4 read + 1 written per element) in the same
      run; microseconds, and the bytes the algorithm moves over the time against the 8 TB/s peak
  (b) end to end: ``traversal_movie`` (one batched decode, one mosaic launch, one copy of the movie) against the
      per-point loop -- one ``get_reconstruction`` call and one copy of an fp32 frame per point, quantised, cropped
      and tiled in numpy -- which was the only way before; host clock around work that ends in a synchronise
  (c) the bytes that cross to the host, both ways
    python tools/bench_traversals.py [--latents 16] [--steps 30] [--bases 5] [--reps 5] [--iters 200] [--out FILE]
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
from behavenet_amd.data.synthetic import base_hparams
from behavenet_amd.fitting.eval import get_reconstruction, movie_src, traversal_movie, traversal_points
from behavenet_amd.models import PSVAE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch

PEAK_GBS = 8000.0
DIM = [2, 128, 128]


def build(n_latents):
    arch = load_handcrafted_arch(list(DIM), n_latents, None, check_memory=False)
    hp = base_hparams(arch, 'ps-vae', {'ps_vae.alpha': 1000, 'ps_vae.beta': 5, 'ps_vae.anneal_epochs': 100,
                                       'max_n_epochs': 200})
    hp['n_labels'] = 4
    hp['device'] = 'cuda'
    np.random.seed(0)
    torch.manual_seed(0)
    return PSVAE(hp).to('cuda').eval()


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def host_movie(model, table, n_base, n_dims, n_frames, n_cols, ch):
    """The per-point loop: decode, copy, quantise and tile on the host."""
    src = movie_src(n_base, n_dims, n_frames, n_cols)
    h, w = DIM[1:]
    movie = np.zeros((src.shape[0], src.shape[1] * h, src.shape[2] * w), dtype=np.uint8)
    where = {int(s): (t, r, c) for (t, r, c), s in np.ndenumerate(src) if s >= 0}
    for p in range(table.shape[0]):
        im = get_reconstruction(model, table[p:p + 1])[0, ch]
        t, r, c = where[p]
        movie[t, r * h:(r + 1) * h, c * w:(c + 1) * w] = np.clip(np.rint(im * np.float32(255)), 0, 255).astype(np.uint8)
    return movie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--latents', type=int, default=16)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--bases', type=int, default=5)
    ap.add_argument('--cols', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_traversals.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    k, n_frames, n_base, n_cols, ch = args.latents, args.steps, args.bases, args.cols, 0
    model = build(k)
    rng = np.random.default_rng(0)
    bases = rng.normal(size=(n_base, k)).astype(np.float32)
    mins, maxes, idxs = np.full(k, -2.0), np.full(k, 2.0), list(range(k))
    table = np.concatenate([traversal_points(b, mins, maxes, idxs, n_frames)[0] for b in bases])
    p, (c, h, w) = table.shape[0], DIM
    src = movie_src(n_base, k, n_frames, n_cols)
    t_n, r_n, c_n = src.shape
    say('device: %s' % torch.cuda.get_device_name(0))
    say('movie: %d latents x %d steps x %d base points = %d points of %dx%dx%d; %d frames of %d x %d panels (%d blank)'
        % (k, n_frames, n_base, p, c, h, w, t_n, r_n, c_n, r_n * c_n - k))

    # (a) the mosaic launch alone
    frames32 = torch.rand((p, c, h, w), device='cuda')
    frames8 = _hip.unit_float_to_u8(frames32)
    src_d = torch.from_numpy(src).to('cuda')
    written = t_n * r_n * c_n * h * w
    fns, nbytes = {}, {}
    for name, frames, width in (('fp32', frames32, 4), ('uint8', frames8, 1)):
        nbytes['mosaic ' + name] = p * h * w * width + written + src.size * 4
        n_yard = nbytes['mosaic ' + name] // 5
        yard_in = torch.rand((n_yard,), device='cuda')
        yard_out = torch.empty((n_yard,), dtype=torch.uint8, device='cuda')
        fns['mosaic ' + name] = (lambda f=frames: _hip.frame_mosaic_u8(f, src_d, ch))
        fns['yardstick ' + name] = (lambda a=yard_in, b=yard_out: _hip.unit_float_to_u8(a, out=b))
        nbytes['yardstick ' + name] = 5 * n_yard
    want = _hip.frame_mosaic_u8(frames8, src_d, ch)
    if not torch.equal(_hip.frame_mosaic_u8(frames32, src_d, ch), want):
        raise SystemExit('the mosaic of fp32 frames is not the mosaic of their grey levels')
    for fn in fns.values():
        event_window(fn, 10)
    us = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            us[name].append(event_window(fn, args.iters))
    say('(a) one launch, hipEvents around %d calls, %d alternated windows; bytes by the algorithm (frames shown read '
        'once, the movie and the source table), not measured traffic' % (args.iters, args.reps))
    for name in fns:
        med = statistics.median(us[name])
        gbs = nbytes[name] / 1e9 / (med * 1e-6)
        say('  %-16s %8.1f us (min %.1f max %.1f), %.1f MB, %.0f GB/s = %.0f %% of the %.0f GB/s peak'
            % (name, med, min(us[name]), max(us[name]), nbytes[name] / 1e6, gbs, 100 * gbs / PEAK_GBS, PEAK_GBS))
    for name in ('fp32', 'uint8'):
        say('  mosaic / yardstick at the same bytes, %s frames: %.2f'
            % (name, statistics.median(us['mosaic ' + name]) / statistics.median(us['yardstick ' + name])))
    del frames32, frames8

    # (b) end to end
    def device_route():
        return traversal_movie(model, bases, mins, maxes, idxs, n_frames, n_cols, ch=ch)
    movie = device_route()
    for q in range(8):          # (warm-up of the single-frame route)
        get_reconstruction(model, table[q:q + 1])
    torch.cuda.synchronize()
    dev_s = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        device_route()
        torch.cuda.synchronize()
        dev_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    loop = host_movie(model, table, n_base, k, n_frames, n_cols, ch)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    diff = np.abs(movie.astype(np.int16) - loop.astype(np.int16))
    say('(b) end to end, host clock: traversal_movie %.1f ms (min %.1f max %.1f over %d runs); the per-point loop '
        '(%d get_reconstruction calls + numpy quantise, tile) %.0f ms, once: %.0f x'
        % (statistics.median(dev_s) * 1e3, min(dev_s) * 1e3, max(dev_s) * 1e3, args.reps, p, host_s * 1e3,
           host_s / statistics.median(dev_s)))
    say('    the two movies differ in %.3f %% of the bytes, by %d grey levels at most (a batch of one may take another '
        'kernel route)' % (100.0 * float((diff > 0).mean()), int(diff.max())))
    # (c) bytes to the host
    say('(c) bytes to the host: %.1f MB (the uint8 movie) against %.1f MB (%d fp32 frames of %d channels)'
        % (movie.nbytes / 1e6, p * c * h * w * 4 / 1e6, p, c))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
