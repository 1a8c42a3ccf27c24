"""The per-trial label R^2 and MSE of a PS-VAE (fitting.eval.label_r2, csrc/segment_sums.hip), measured in ONE process:

  (a) end to end  a default-architecture PS-VAE at 2x128x128 over a synthetic session (device-resident uint8 trials,
                  labels and label masks): ``label_r2`` -- every trial encoded, three device tables, one launch, (S, L,
                  4) doubles to the host -- against the reference's route written with this package's pieces: per
                  trial ``get_transformed_latents(images)`` to numpy, then the masked per-label loop with
                  ``_r2_variance_weighted`` and ``np.mean(np.square(...))``.  Host clock around work that ends with
                  the numbers on the host; the two alternated.  Checked against each other before anything is timed.
  (b) the launch  ``bn_segment_label_sums`` alone at 10^6 x 16 with masks, by hipEvents around --iters calls: as 4,000
                  segments of 250 rows and as one segment of 10^6; microseconds and GB/s by the algorithm's bytes (the
                  three tables read once: 12 bytes an element; not measured traffic).  In the same run, alternated:
                  ``bn_column_count`` on a table of the same bytes (the streaming neighbour), and the same sums from
                  torch ops on the device (``torch.where`` on float64 copies + ``torch.segment_reduce``), the composite
                  the launch replaces, checked against it first.
  (c) from HBM    (b)'s 192 MB fit the 256 MiB Infinity Cache and are re-read in every window; the same launches and the
                  same neighbour at 6 x 10^6 x 16 (1.15 GB), which cannot stay there.
    python tools/bench_label_r2.py [--trials 64] [--frames 250] [--reps 5] [--iters 50] [--out FILE]
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
from behavenet_amd.fitting.eval import label_r2
from behavenet_amd.models import PSVAE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from behavenet_amd.models.vaes import _r2_variance_weighted

PEAK_GBS = 8000.0
DIM = [2, 128, 128]
N_LABELS, N_LATENTS = 4, 12


class MaskedGenerator(SyntheticSessionsGenerator):
    """The synthetic generator, serving the sessions' ``labels_masks`` next to their labels."""

    def _extra_signals(self, sample, sess, trial):
        sample['labels_masks'] = self._masks[sess][trial][None]


def build():
    arch = load_handcrafted_arch(list(DIM), N_LATENTS, None, check_memory=False)
    hp = base_hparams(arch, 'ps-vae', {'ps_vae.alpha': 1000, 'ps_vae.beta': 5, 'ps_vae.anneal_epochs': 100,
                                       'max_n_epochs': 10, 'n_labels': N_LABELS, 'device': 'cuda'})
    np.random.seed(0)
    torch.manual_seed(0)
    return PSVAE(hp).to('cuda').eval()


def reference_route(gen, model, dtype='val'):
    """get_label_r2's loop (plotting/cond_ae_utils.py:1246-1265 of the reference) on this package's pieces."""
    rows = []
    gen.reset_iterators(dtype)
    for _ in range(gen.n_tot_batches[dtype]):
        data, sess = gen.next_batch(dtype)
        y = data['labels'][0].cpu().numpy()
        n = data['labels_masks'][0].cpu().numpy()
        with torch.no_grad():
            z = model.get_transformed_latents(data['images'][0], dataset=sess)
        for i in range(N_LABELS):
            y_true, y_pred = y[:, i][n[:, i] == 1], z[:, i][n[:, i] == 1]
            if len(y_true) > 10:
                rows.append((int(data['batch_idx'].item()), i, _r2_variance_weighted(y_true, y_pred),
                             float(np.mean(np.square(y_true - y_pred)))))
            else:
                rows.append((int(data['batch_idx'].item()), i, np.nan, np.nan))
    return rows


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


def torch_sums(pred, truth, mask, lengths):
    """The same (S, L, 4) float64 sums from torch ops on the device."""
    ok = mask == 1
    y, p = truth.double(), pred.double()
    zero = torch.zeros((), dtype=torch.float64, device=pred.device)
    d = y - p
    terms = torch.stack([ok.double(), torch.where(ok, y, zero), torch.where(ok, y * y, zero),
                         torch.where(ok, d * d, zero)], dim=2)
    return torch.segment_reduce(terms, 'sum', lengths=lengths, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trials', type=int, default=64, help='val trials of the synthetic session')
    ap.add_argument('--frames', type=int, default=250)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_label_r2.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))

    # (a) end to end
    model = build()
    sess = SyntheticSession(args.trials + 2, args.frames, DIM, seed=1, n_labels=N_LABELS,
                            trial_splits='1;%d;1;0' % args.trials)
    rng = np.random.default_rng(2)
    gen = MaskedGenerator([sess], device='cuda', placement='device_u8')
    gen._masks = [[torch.from_numpy((rng.random(l.shape) < 0.8).astype(np.float32)).cuda() for l in sess.labels]]
    n_val = len(sess.batch_idxs['val'])
    say('(a) PS-VAE %dx%dx%d, %d latents, %d labels; %d val trials of %d frames, 80 %% label masks'
        % (DIM[0], DIM[1], DIM[2], N_LATENTS, N_LABELS, n_val, args.frames))
    got = label_r2(gen, model, 'val')
    want = {(t, i): (r2, mse) for t, i, r2, mse in reference_route(gen, model)}
    worst = 0.0
    for k, t in enumerate(got['trial']):
        for i in range(N_LABELS):
            r2, mse = want[(int(t), i)]
            worst = max(worst, abs(got['r2'][k, i] - r2) / max(1.0, abs(1 - r2)), abs(got['mse'][k, i] - mse) / mse)
    say('    label_r2 against the per-trial host route: largest difference %.2e (R^2 relative to max(1, |1 - R^2|), '
        'MSE relative; the host route squares in float32)' % worst)
    assert worst < 1e-5
    ours, theirs = [], []
    for _ in range(args.reps):
        ours.append(host_clock(lambda: label_r2(gen, model, 'val')))
        theirs.append(host_clock(lambda: reference_route(gen, model)))
    say('    label_r2 (walk, encode, one launch, %d doubles back)  %9.2f ms (min %.2f max %.2f over %d)'
        % (got['sums'].size, statistics.median(ours), min(ours), max(ours), args.reps))
    say('    per-trial route (encode, copy, %d host scores)        %9.2f ms (min %.2f max %.2f over %d)'
        % (n_val * N_LABELS, statistics.median(theirs), min(theirs), max(theirs), args.reps))
    del model, gen

    # (b) the launch alone
    n, L = 10 ** 6, 16
    g = torch.Generator(device='cuda').manual_seed(3)
    truth = 300 + 50 * torch.randn((n, L), device='cuda', generator=g)
    pred = truth + 20 * torch.randn((n, L), device='cuda', generator=g)
    mask = (torch.rand((n, L), device='cuda', generator=g) < 0.8).float()
    shapes = {'4,000 segments of 250 rows': torch.full((4000,), 250, dtype=torch.int64, device='cuda'),
              'one segment of 10^6 rows': torch.full((1,), n, dtype=torch.int64, device='cuda')}
    offsets = {k: torch.cat([v.new_zeros(1), v.cumsum(0)]) for k, v in shapes.items()}
    nbytes = 3 * n * L * 4
    neighbour = torch.randn((n, 3 * L), device='cuda', generator=g)          # the same bytes in one table
    fns = {}
    for name in shapes:
        ours_d, torch_d = _hip.segment_label_sums(pred, truth, mask, offsets[name]), torch_sums(pred, truth, mask, shapes[name])
        assert torch.equal(ours_d[..., 0], torch_d[..., 0])
        rel = ((ours_d - torch_d).abs() / torch_d.abs().clamp_min(1e-300)).max().item()
        say('(b) %s: bn_segment_label_sums against the torch composite, largest relative difference %.1e'
            % (name, rel))
        assert rel < 1e-9
        fns['bn_segment_label_sums, ' + name] = (lambda o=offsets[name]: _hip.segment_label_sums(pred, truth, mask, o))
        fns['  torch.where + segment_reduce, ' + name] = (lambda v=shapes[name]: torch_sums(pred, truth, mask, v))
    fns['bn_column_count at the same bytes (10^6 x 48)'] = lambda: _hip.column_count(neighbour)
    for fn in fns.values():
        event_window(fn, 3)
    us = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            us[name].append(event_window(fn, args.iters if 'torch' not in name else max(args.iters // 10, 2)))
    say('    10^6 x 16 fp32 predictions, labels and masks; hipEvents around the calls, %d alternated windows; %.0f MB by '
        'the algorithm (three tables read once), not measured traffic' % (args.reps, nbytes / 1e6))
    for name in fns:
        med = statistics.median(us[name])
        gbs = nbytes / 1e9 / (med * 1e-6)
        say('    %-62s %9.1f us (min %.1f max %.1f), %.0f GB/s = %.0f %% of the %.0f GB/s peak'
            % (name, med, min(us[name]), max(us[name]), gbs, 100 * gbs / PEAK_GBS, PEAK_GBS))
    blocks, rows = _hip._segment_sums_plan(n, L)
    say('    partition: %d row blocks of %d rows' % (blocks, rows))
    say('    (the 192 MB of (b) fit the 256 MiB Infinity Cache and are re-read in every window: these are rates on a set '
        'that can stay cache-resident, not HBM rates)')
    del pred, truth, mask, neighbour, fns

    # (c) the same launches on a set that does not fit the cache
    n = 6 * 10 ** 6
    truth = 300 + 50 * torch.randn((n, L), device='cuda', generator=g)
    pred = truth + 20 * torch.randn((n, L), device='cuda', generator=g)
    mask = (torch.rand((n, L), device='cuda', generator=g) < 0.8).float()
    neighbour = torch.randn((n, 3 * L), device='cuda', generator=g)
    nbytes = 3 * n * L * 4
    many = torch.arange(0, n + 1, 250, dtype=torch.int64, device='cuda')
    one = torch.tensor([0, n], dtype=torch.int64, device='cuda')
    fns = {'bn_segment_label_sums, 24,000 segments of 250 rows': lambda: _hip.segment_label_sums(pred, truth, mask, many),
           'bn_segment_label_sums, one segment of 6 x 10^6 rows': lambda: _hip.segment_label_sums(pred, truth, mask, one),
           'bn_column_count at the same bytes (6 x 10^6 x 48)': lambda: _hip.column_count(neighbour)}
    a_many, a_one = fns['bn_segment_label_sums, 24,000 segments of 250 rows'](), \
        fns['bn_segment_label_sums, one segment of 6 x 10^6 rows']()
    rel = ((a_many.sum(dim=0) - a_one[0]).abs() / a_one[0].abs()).max().item()
    say('(c) 6 x 10^6 x 16, %.0f MB by the algorithm: more than four times the Infinity Cache, so every window streams '
        'from HBM; the 24,000 segments added up against the single one: largest relative difference %.1e'
        % (nbytes / 1e6, rel))
    assert rel < 1e-9
    for fn in fns.values():
        event_window(fn, 3)
    us = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            us[name].append(event_window(fn, max(args.iters // 2, 2)))
    for name in fns:
        med = statistics.median(us[name])
        gbs = nbytes / 1e9 / (med * 1e-6)
        say('    %-62s %9.1f us (min %.1f max %.1f), %.0f GB/s = %.0f %% of the %.0f GB/s peak'
            % (name, med, min(us[name]), max(us[name]), gbs, 100 * gbs / PEAK_GBS, PEAK_GBS))
    blocks, rows = _hip._segment_sums_plan(n, L)
    say('    partition: %d row blocks of %d rows' % (blocks, rows))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
