"""The correlation matrices of a model's latents (fitting.eval.latent_correlations, csrc/segment_gram.hip), measured in
ONE process:

  (a) end to end  a default-architecture PS-VAE at 2x128x128 over a synthetic session (device-resident uint8 trials):
                  ``latent_correlations`` in batches of 200 rows -- every train trial encoded, one device table, one
                  launch, (S, D + 1, D + 1) doubles to the host -- against the reference's route written with this
                  package's pieces: per trial ``encode_trial`` to numpy, ``np.vstack``, then ``np.corrcoef`` per batch.
                  Host clock around work that ends with the numbers on the host; the two alternated.  Checked against
                  each other before anything is timed.
  (b) the launch  ``bn_segment_gram`` alone, by hipEvents around --iters calls of the wrapper, warm-up first: 10^6 x 16
                  as one segment, as 4,000 trials of 250 rows and as batches of 200 rows, and 10^6 x 64 as one segment;
                  microseconds, GB/s by the algorithm's bytes (the table read once; not measured traffic) and float64
                  GFLOP/s by the algorithm's D (D + 1) / 2 FMAs a row.  Next to each, alternated in the same run:
                  ``bn_segment_label_sums`` without masks on two tables of half the columns (the same bytes: the
                  streaming neighbour) and torch's route on the device, ``t = z.double(); t.T @ t`` -- per segment for
                  the segmented cases --, checked against the launch first.
    python tools/bench_latent_corr.py [--trials 64] [--frames 250] [--reps 5] [--iters 50] [--out FILE]
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
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.data.synthetic import base_hparams
from behavenet_amd.fitting.eval import encode_trial, latent_correlations
from behavenet_amd.models import PSVAE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch

PEAK_GBS = 8000.0
PEAK_FP64_GFLOPS = 78600.0          # the data sheet's vector float64 rate; its matrix float64 rate is the same
DIM = [2, 128, 128]
N_LABELS, N_LATENTS = 4, 12
BATCH = 200


def build():
    arch = load_handcrafted_arch(list(DIM), N_LATENTS, None, check_memory=False)
    hp = base_hparams(arch, 'ps-vae', {'ps_vae.alpha': 1000, 'ps_vae.beta': 5, 'ps_vae.anneal_epochs': 100,
                                       'max_n_epochs': 10, 'n_labels': N_LABELS, 'device': 'cuda'})
    np.random.seed(0)
    torch.manual_seed(0)
    return PSVAE(hp).to('cuda').eval()


def reference_route(gen, model, batch_size=BATCH):
    """The hyperparameter search's lines (plotting/cond_ae_utils.py:1679-1698 of the reference) on this package's
    pieces: the train trials' latents on the host, stacked, ``np.corrcoef`` of the first two unsupervised columns per
    batch."""
    ds = gen.datasets[0]
    latents = np.vstack([encode_trial(model, torch.from_numpy(ds.images_u8[int(t)]).cuda(), 0)
                         for t in ds.batch_idxs['train']])
    out = []
    for i in range(int(np.ceil(latents.shape[0] / batch_size))):
        corr = np.corrcoef(latents[i * batch_size:(i + 1) * batch_size, N_LABELS + np.array([0, 1])].T)
        out.append(np.abs(corr[0, 1]))
    return np.asarray(out)


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def torch_gram(z, bounds):
    """The second moments alone, (S, D, D) float64, by torch on the device: a float64 copy, one matmul a segment."""
    t = z.double()
    return torch.stack([t[a:b].T @ t[a:b] for a, b in zip(bounds[:-1], bounds[1:])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trials', type=int, default=64, help='train trials of the synthetic session')
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_latent_corr.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))

    # (a) end to end
    model = build()
    sess = SyntheticSession(args.trials + 2, args.frames, DIM, seed=1, n_labels=N_LABELS,
                            trial_splits='%d;1;1;0' % args.trials)
    gen = SyntheticSessionsGenerator([sess], device='cuda', placement='device_u8')
    n_train = len(sess.batch_idxs['train'])
    say('(a) PS-VAE %dx%dx%d, %d latents, %d labels; %d train trials of %d frames, batches of %d rows'
        % (DIM[0], DIM[1], DIM[2], N_LATENTS, N_LABELS, n_train, args.frames, BATCH))
    got = latent_correlations(gen, model, segments=BATCH)
    want = reference_route(gen, model)
    worst = float(np.abs(got['abs_corr_01'] - want).max())
    say('    latent_correlations against the host route: largest difference of |corr[0, 1]| %.2e over %d batches'
        % (worst, len(want)))
    assert len(want) == len(got['abs_corr_01']) and worst < 1e-6
    ours, theirs = [], []
    for _ in range(args.reps):
        ours.append(host_clock(lambda: latent_correlations(gen, model, segments=BATCH)))
        theirs.append(host_clock(lambda: reference_route(gen, model)))
    say('    latent_correlations (walk, encode, one launch, %d doubles back)  %9.2f ms (min %.2f max %.2f over %d)'
        % (got['gram'].size, statistics.median(ours), min(ours), max(ours), args.reps))
    say('    host route (encode, copy, vstack, %d np.corrcoef calls)         %9.2f ms (min %.2f max %.2f over %d)'
        % (len(want), statistics.median(theirs), min(theirs), max(theirs), args.reps))
    del model, gen

    # (b) the launch alone
    n = 10 ** 6
    g = torch.Generator(device='cuda').manual_seed(3)
    for D, cases in ((16, (('one segment of 10^6 rows', [0, n]),
                           ('4,000 trials of 250 rows', list(range(0, n + 1, 250))),
                           ('5,000 batches of 200 rows', list(range(0, n + 1, 200))))),
                     (64, (('one segment of 10^6 rows', [0, n]),))):
        z = 300 + torch.randn((n, D), device='cuda', generator=g)
        shift = z[0].contiguous()
        half_a = torch.randn((n, D // 2), device='cuda', generator=g)          # the neighbour: the same bytes
        half_b = torch.randn((n, D // 2), device='cuda', generator=g)
        nbytes = n * D * 4
        flops = 2.0 * n * D * (D + 1) / 2
        fns = {}
        for name, bounds in cases:
            off_d = torch.tensor(bounds, dtype=torch.int64, device='cuda')
            ours_d = _hip.segment_gram(z, off_d, shift)
            torch_d = torch_gram(z - shift, bounds)
            assert torch.equal(ours_d[:, 0, 0], (off_d[1:] - off_d[:-1]).double())
            rel = ((ours_d[:, 1:, 1:] - torch_d).abs().amax(dim=(1, 2))
                   / torch_d.abs().amax(dim=(1, 2))).max().item()
            say('(b) 10^6 x %d, %s: bn_segment_gram against torch float64 (on z - shift), largest difference '
                'relative to the matrix\'s largest entry %.1e' % (D, name, rel))
            assert rel < 1e-9
            fns['bn_segment_gram, ' + name] = (lambda o=off_d: _hip.segment_gram(z, o, shift))
            fns['  bn_segment_label_sums at the same bytes, ' + name] = \
                (lambda o=off_d: _hip.segment_label_sums(half_a, half_b, None, o))
            fns['  torch z.double(); t.T @ t a segment, ' + name] = (lambda b=bounds: torch_gram(z, b))
        for fn in fns.values():
            event_window(fn, 2)
        us = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                iters = args.iters
                if 'torch' in name:
                    iters = max(args.iters // 10, 2) if 'one segment' in name else 1
                us[name].append(event_window(fn, iters))
        say('    10^6 x %d fp32; hipEvents around the calls, %d alternated windows; %.0f MB by the algorithm (the table '
            'read once), %.2f GFLOP float64 by the algorithm (D (D + 1) / 2 FMAs a row); not measured traffic'
            % (D, args.reps, nbytes / 1e6, flops / 1e9))
        for name in fns:
            med = statistics.median(us[name])
            gbs = nbytes / 1e9 / (med * 1e-6)
            line = '    %-66s %10.1f us (min %.1f max %.1f), %.0f GB/s = %.0f %% of the %.0f GB/s peak' \
                % (name, med, min(us[name]), max(us[name]), gbs, 100 * gbs / PEAK_GBS, PEAK_GBS)
            if name.startswith('bn_segment_gram'):
                gf = flops / 1e9 / (med * 1e-6)
                line += ', %.0f GFLOP/s = %.0f %% of the %.0f float64 peak' % (gf, 100 * gf / PEAK_FP64_GFLOPS,
                                                                             PEAK_FP64_GFLOPS)
            say(line)
        blocks, rows = _hip._segment_gram_plan(n, D)
        say('    partition: %d row blocks of %d rows; the %.0f MB table fits the 256 MiB Infinity Cache and is re-read in '
            'every window: rates on a set that can stay cache-resident, not HBM rates' % (blocks, rows, nbytes / 1e6))
        del z, half_a, half_b, fns
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
