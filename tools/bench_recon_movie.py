"""The reconstruction movie of an autoencoder -- original | reconstruction | residual -- written on the device
(fitting.eval.reconstruction_movie, csrc/recon_panels.hip).

The workload: one trial of 400 stored uint8 frames of 2x128x128 through a default-architecture conv AE.

  (a) the panel launch alone, on uint8 frames with an fp32 reconstruction (the fp32 lane), with a uint8 one (a served
      bf16 decoder's grey levels) and with per-frame masks: hipEvents around --iters launches, --reps windows
      alternated, in the same run, with ``bn_frame_mosaic_u8`` (fp32 frames, whole single-channel panels) and
      ``bn_unit_float_to_u8`` on the SAME byte count; microseconds, and the bytes the algorithm moves (every operand
      read once, the strips written) over the time against the 8 TB/s peak
  (b) end to end: ``reconstruction_movie`` (forward pass, one panel launch per chunk, one copy of the movie) against
      the host route -- ``get_reconstruction`` copies the fp32 reconstruction, numpy builds the three fp32 arrays,
      clips, quantises and puts the panels together; host clock around work that ends in a synchronise
  (c) the bytes that cross to the host, both ways
    python tools/bench_recon_movie.py [--frames 400] [--reps 5] [--iters 200] [--out FILE]
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
from behavenet_amd.fitting.eval import get_reconstruction, reconstruction_movie
from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch

PEAK_GBS = 8000.0
DIM = [2, 128, 128]


def build(n_latents=12):
    arch = load_handcrafted_arch(list(DIM), n_latents, None, check_memory=False)
    hp = base_hparams(arch, 'ae')
    hp['device'] = 'cuda'
    np.random.seed(0)
    torch.manual_seed(0)
    return AE(hp).to('cuda').eval()


def smooth_frames(n, seed=0):
    """uint8 frames with structure (a noise trial would make every residual a noise image too)."""
    c, h, w = DIM
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing='ij')
    ph = torch.rand((n, c, 1, 1), generator=g) * 6.28
    img = 0.5 + 0.45 * torch.sin(6.0 * yy + ph) * torch.cos(4.0 * xx - ph)
    return (img * 255).round().clamp(0, 255).to(torch.uint8)


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def host_movie(model, xf):
    """The reference's way: the fp32 reconstruction to the host, three fp32 arrays, clip and quantise in numpy."""
    recon = get_reconstruction(model, xf, dataset=0)
    orig = xf.cpu().numpy()
    ims = [orig, recon, np.float32(0.5) + (orig - recon)]
    panels = [np.concatenate([im[:, k] for k in range(im.shape[1])], axis=2) for im in ims]
    return np.clip(np.rint(np.concatenate(panels, axis=2) * np.float32(255)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_recon_movie.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    n, (c, h, w) = args.frames, DIM
    px = n * c * h * w
    say('device: %s' % torch.cuda.get_device_name(0))
    say('trial: %d frames of %dx%dx%d, movie (%d, %d, %d) uint8' % (n, c, h, w, n, h, 3 * c * w))

    # (a) the panel launch alone
    xu = smooth_frames(n).to('cuda')
    recon32 = torch.rand((n, c, h, w), device='cuda')
    recon8 = _hip.unit_float_to_u8(recon32)
    masks = (torch.rand((n, c, h, w), device='cuda') > 0.3).float()
    out = torch.empty((n, h, 3 * c * w), dtype=torch.uint8, device='cuda')
    fns, nbytes = {}, {}
    for lane, recon, mask, per_px in (('u8|fp32', recon32, None, 1 + 4 + 3), ('u8|u8', recon8, None, 1 + 1 + 3),
                                      ('u8|fp32|mask', recon32, masks, 1 + 4 + 4 + 3)):
        name = 'panels ' + lane
        nbytes[name] = px * per_px
        fns[name] = (lambda r=recon, m=mask: _hip.recon_panels_u8(xu, r, m, out=out))
        # the neighbours at the same byte count: 4 bytes read and 1 written per element
        n_el = nbytes[name] // 5
        p = max(1, n_el // (h * w))
        planes = torch.rand((p, 1, h, w), device='cuda')
        src_d = torch.arange(p, dtype=torch.int32, device='cuda').view(p, 1, 1)
        fns['  mosaic at the bytes of ' + lane] = (lambda f=planes, s=src_d: _hip.frame_mosaic_u8(f, s, 0))
        nbytes['  mosaic at the bytes of ' + lane] = p * h * w * 5 + 4 * p
        yard_in = torch.rand((n_el,), device='cuda')
        yard_out = torch.empty((n_el,), dtype=torch.uint8, device='cuda')
        fns['  float_to_u8 at the bytes of ' + lane] = (lambda a=yard_in, b=yard_out: _hip.unit_float_to_u8(a, out=b))
        nbytes['  float_to_u8 at the bytes of ' + lane] = 5 * n_el
    for fn in fns.values():
        event_window(fn, 10)
    us = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            us[name].append(event_window(fn, args.iters))
    say('(a) one launch, hipEvents around %d calls, %d alternated windows; bytes by the algorithm (every operand read '
        'once, the output written), not measured traffic' % (args.iters, args.reps))
    for name in fns:
        med = statistics.median(us[name])
        gbs = nbytes[name] / 1e9 / (med * 1e-6)
        say('  %-42s %8.1f us (min %.1f max %.1f), %.1f MB, %.0f GB/s = %.0f %% of the %.0f GB/s peak'
            % (name, med, min(us[name]), max(us[name]), nbytes[name] / 1e6, gbs, 100 * gbs / PEAK_GBS, PEAK_GBS))
    del recon32, recon8, masks, fns

    # (b) end to end
    model = build()
    xf = _hip.u8_to_unit_float(xu)
    movie = reconstruction_movie(model, xu, 0)
    loop = host_movie(model, xf)
    torch.cuda.synchronize()
    dev_s, host_s = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        reconstruction_movie(model, xu, 0)
        torch.cuda.synchronize()
        dev_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_movie(model, xf)
        torch.cuda.synchronize()
        host_s.append(time.perf_counter() - t0)
    diff = np.abs(movie.astype(np.int16) - loop.astype(np.int16))
    say('(b) end to end, host clock, %d alternated runs: reconstruction_movie %.1f ms (min %.1f max %.1f); the host '
        'route (get_reconstruction + three fp32 arrays + numpy clip, quantise, concatenate) %.1f ms (min %.1f max %.1f): '
        '%.1f x' % (args.reps, statistics.median(dev_s) * 1e3, min(dev_s) * 1e3, max(dev_s) * 1e3,
                    statistics.median(host_s) * 1e3, min(host_s) * 1e3, max(host_s) * 1e3,
                    statistics.median(host_s) / statistics.median(dev_s)))
    say('    the two movies differ in %.4f %% of the bytes, by %d grey levels at most (the host route decodes all %d '
        'frames in one batch, the movie in chunks of 200)' % (100.0 * float((diff > 0).mean()), int(diff.max()), n))
    # (c) bytes to the host
    say('(c) bytes to the host: %.1f MB (the uint8 movie) against %.1f MB (the fp32 reconstruction)'
        % (movie.nbytes / 1e6, px * 4 / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
