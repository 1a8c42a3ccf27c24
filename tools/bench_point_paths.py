"""The point-path traversal movie of a PS-VAE, both views in every panel, tiled on the device
(fitting.eval.point_path_movie, bn_frame_mosaic_ch_u8 in csrc/frame_mosaic.hip).

The workload: 16 latents, each walked min -> max -> min in two legs of 10 + 1 steps from 5 base points at 2x128x128 on
a default-architecture PS-VAE -- 1,760 decoded points, a movie of 5 x (22 + 5 buffer) = 135 frames of 6 x 3 panels (two
of them blank), every panel its frame's two channels side by side.

  (a) the mosaic launch alone, fp32 and uint8 frames: hipEvents around --iters launches, --reps windows alternated, in
      the same run, with the route the channel range replaces -- ``bn_frame_mosaic_u8`` on the frames viewed as
      (P C, 1, H, W) with C source indices per panel, which writes the same bytes -- and with the yardstick
      ``bn_unit_float_to_u8`` on the same byte count; microseconds, and the bytes the algorithm moves over the time
  (b) end to end: ``point_path_movie`` (one batched decode, one mosaic launch per 200 movie frames, one copy of the
      movie) against the per-point loop -- one ``get_reconstruction`` call and one copy of an fp32 frame per point,
      quantised and tiled in numpy -- which was the only way before; host clock around work that ends in a synchronise
  (c) the bytes that cross to the host, both ways
    python tools/bench_point_paths.py [--latents 16] [--frames 10] [--bases 5] [--reps 5] [--iters 200] [--out FILE]
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
from behavenet_amd.fitting.eval import get_reconstruction, path_movie_src, path_points, point_path_movie
from tools.bench_traversals import DIM, PEAK_GBS, build, event_window


def movie_table(bases, panels, n_frames):
    legs = []
    for row in bases:
        for d, lo, hi in panels:
            points = np.array([row] * 3)
            points[0, d], points[1, d], points[2, d] = lo, hi, lo
            legs.append(path_points(points, n_frames))
    return np.concatenate(legs).astype(np.float32)


def host_movie(model, table, src):
    """The per-point loop: decode, copy, quantise and tile on the host, the channels of a frame side by side."""
    c, h, w = DIM
    movie = np.zeros((src.shape[0], src.shape[1] * h, src.shape[2] * c * w), dtype=np.uint8)
    where = {int(s): (t, r, k) for (t, r, k), s in np.ndenumerate(src) if s >= 0}
    for p in range(table.shape[0]):
        im = np.concatenate(list(get_reconstruction(model, table[p:p + 1])[0]), axis=1)
        t, r, k = where[p]
        movie[t, r * h:(r + 1) * h, k * c * w:(k + 1) * c * w] = \
            np.clip(np.rint(im * np.float32(255)), 0, 255).astype(np.uint8)
    return movie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--latents', type=int, default=16)
    ap.add_argument('--frames', type=int, default=10, help='n_frames: a leg has n_frames + 1 steps')
    ap.add_argument('--bases', type=int, default=5)
    ap.add_argument('--buffer', type=int, default=5)
    ap.add_argument('--cols', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_point_paths.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    k, n_frames, n_base, n_buf, n_cols = args.latents, args.frames, args.bases, args.buffer, args.cols
    n_steps = 2 * (n_frames + 1)
    model = build(k)
    rng = np.random.default_rng(0)
    bases = rng.normal(size=(n_base, k)).astype(np.float32)
    panels = [(d, -2.0, 2.0) for d in range(k)]
    table = movie_table(bases, panels, n_frames)
    p, (c, h, w) = table.shape[0], DIM
    src = path_movie_src(n_base, k, n_steps, n_buf, n_cols)
    t_n, r_n, c_n = src.shape
    say('device: %s' % torch.cuda.get_device_name(0))
    say('movie: %d latents x 2 legs of %d + 1 steps x %d base points = %d points of %dx%dx%d; %d frames (%d of them '
        'buffer frames) of %d x %d panels (%d blank), %d channels side by side in a panel'
        % (k, n_frames, n_base, p, c, h, w, t_n, n_base * n_buf if n_base > 1 else 0, r_n, c_n, r_n * c_n - k, c))

    # (a) the mosaic launch alone
    frames32 = torch.rand((p, c, h, w), device='cuda')
    frames8 = _hip.unit_float_to_u8(frames32)
    src_d = torch.from_numpy(src).to('cuda')
    # the view route: one source index per channel, blank panels stay blank
    src_view = np.where(src[..., None] >= 0, src[..., None] * c + np.arange(c), -1).reshape(t_n, r_n, c_n * c)
    src_view_d = torch.from_numpy(np.ascontiguousarray(src_view, dtype=np.int32)).to('cuda')
    written = t_n * r_n * c_n * c * h * w
    fns, nbytes = {}, {}
    for name, frames, width in (('fp32', frames32, 4), ('uint8', frames8, 1)):
        moved = p * c * h * w * width + written
        view = frames.view(p * c, 1, h, w)
        fns['channels ' + name] = (lambda f=frames: _hip.frame_mosaic_u8(f, src_d, None))
        nbytes['channels ' + name] = moved + src.size * 4
        fns['view ' + name] = (lambda f=view: _hip.frame_mosaic_u8(f, src_view_d, 0))
        nbytes['view ' + name] = moved + src_view.size * 4
        n_yard = moved // 5
        yard_in = torch.rand((n_yard,), device='cuda')
        yard_out = torch.empty((n_yard,), dtype=torch.uint8, device='cuda')
        fns['yardstick ' + name] = (lambda a=yard_in, b=yard_out: _hip.unit_float_to_u8(a, out=b))
        nbytes['yardstick ' + name] = 5 * n_yard
        if not torch.equal(fns['channels ' + name](), fns['view ' + name]()):
            raise SystemExit('the channel range and the view route write different movies')
    if not torch.equal(fns['channels fp32'](), fns['channels uint8']()):
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
        ch_us = statistics.median(us['channels ' + name])
        say('  %s frames: channels / view %.2f, channels / yardstick at the same bytes %.2f'
            % (name, ch_us / statistics.median(us['view ' + name]), ch_us / statistics.median(us['yardstick ' + name])))
    del frames32, frames8, fns

    # (b) end to end
    def device_route():
        return point_path_movie(model, bases, panels, n_frames, n_buf, n_cols, ch=None)
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
    loop = host_movie(model, table, src)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    diff = np.abs(movie.astype(np.int16) - loop.astype(np.int16))
    say('(b) end to end, host clock: point_path_movie %.1f ms (min %.1f max %.1f over %d runs); the per-point loop '
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
