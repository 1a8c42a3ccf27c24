"""One EM iteration of a GRID of ARHMMs on one table of latents (models.arhmm.ARHMMGroup, csrc/arhmm.hip), measured in
ONE process on --rows x 16 latents (default 10^6) cut into trials of 250 rows, one lag, the grid K in {2, 4, 8, 16, 32}
x 4 values of kappa x 3 seeds: 60 models, 744 states, cut into groups by fitting.eval.arhmm_grid_groups (two groups).

  (a) the grid     ``ARHMMGroup.em_step`` per group: fold, three launches, one transfer, every model's M-step on the
                   host.  Host clock around work that ends with the parameters on the host.
  (b) one by one   the same 60 iterations through ``ARHMM.em_step``, one model after the other.
                   (a) and (b) alternate, --reps times after a warm-up of each, from the same initialised models.
  (c) the launches ``bn_arhmm_grid_loglik``, ``bn_hmm_grid_forward_backward`` (posteriors, and likelihood only) and
                   ``bn_arhmm_grid_moments`` per group, by hipEvents around --iters calls of the wrappers.
    python tools/bench_arhmm_grid.py [--rows 1000000] [--reps 3] [--iters 3] [--out FILE]
"""
import argparse
import os
import pickle
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.signal import lfilter

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import arhmm_grid, arhmm_grid_groups
from behavenet_amd.models.arhmm import ARHMM, ARHMMGroup

D, LAGS, TRIAL = 16, 1, 250
STATES, KAPPAS, SEEDS = (2, 4, 8, 16, 32), (1.0, 10.0, 100.0, 1000.0), (0, 1, 2)


def table(n, seed):
    """fp32 (n, D): a random walk pulled to one of 16 centres that changes every 40 rows or so."""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((16, D))
    z = np.repeat(rng.integers(0, 16, size=n // 40 + 1), 40)[:n]
    drive = 0.2 * centres[z] + 0.3 * rng.standard_normal((n, D))
    drive[0] = 0.0
    return lfilter([1.0], [1.0, -0.8], drive, axis=0).astype(np.float32)


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm_grid.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    n = args.rows
    z_d = torch.from_numpy(table(n, 1)).cuda()
    offsets = np.minimum(np.arange(n // TRIAL + 1, dtype=np.int64) * TRIAL, n)
    offsets[-1] = n
    off_d = torch.from_numpy(offsets).cuda()
    grid = arhmm_grid(STATES, n_lags=LAGS, transitions='sticky', kappa=KAPPAS, rng_seed_model=SEEDS)
    groups = arhmm_grid_groups(grid, n)
    say('--- %d x %d, lags = %d, %d trials of %d rows; %d models, %d states, %d groups of %s models and %s states'
        % (n, D, LAGS, len(offsets) - 1, TRIAL, len(grid), sum(c['n_states'] for c in grid), len(groups),
           [len(g) for g in groups], [sum(grid[i]['n_states'] for i in g) for g in groups]))
    models = [ARHMM(c['n_states'], D, lags=LAGS, transitions='sticky', kappa=c['kappa']) for c in grid]
    ms, _ = host_clock(lambda: [m.initialize(z_d, offsets, seed=c['rng_seed_model']) for m, c in zip(models, grid)])
    say('initialised one by one (ARHMM.initialize): %.1f ms' % ms)
    start = pickle.dumps(models)

    def grid_step(ms_):
        return [ARHMMGroup([ms_[i] for i in g]).em_step(z_d, off_d).sum(axis=1) for g in groups]

    def single_step(ms_):
        return [m.em_step(z_d, off_d).sum() for m in ms_]

    grid_step(pickle.loads(start))                          # warm-up of both routes
    single_step(pickle.loads(start))
    t_grid, t_single = [], []
    for _ in range(args.reps):
        a, b = pickle.loads(start), pickle.loads(start)
        ms, lg = host_clock(lambda: grid_step(a))
        t_grid.append(ms)
        ms, ls = host_clock(lambda: single_step(b))
        t_single.append(ms)
    lg = np.concatenate(lg)[np.argsort(np.concatenate(groups))]
    ls = np.asarray(ls)
    worst = max(np.abs(getattr(x, name) - getattr(y, name)).max() for x, y in zip(a, b)
                for name in ('As', 'bs', 'Sigmas', 'log_Ps', 'log_pi0'))
    say('(a) ARHMMGroup.em_step, %d groups:      %9.1f ms (min %.1f max %.1f over %d)'
        % (len(groups), statistics.median(t_grid), min(t_grid), max(t_grid), len(t_grid)))
    say('(b) ARHMM.em_step, %d models in turn:  %9.1f ms (min %.1f max %.1f over %d); (b) / (a) = %.2f'
        % (len(models), statistics.median(t_single), min(t_single), max(t_single), len(t_single),
           statistics.median(t_single) / statistics.median(t_grid)))
    say('    largest relative difference of a model\'s log-likelihood between the routes %.2e, of a parameter after '
        'the iteration %.2e' % (float(np.max(np.abs(lg - ls) / np.abs(ls))), worst))

    models = pickle.loads(start)
    for gi, g in enumerate(groups):
        group = ARHMMGroup([models[i] for i in g])
        KT, M, P = group.KT, group.M, group.P
        G, cst = group.fold()
        G_d, cst_d = torch.from_numpy(G).cuda(), torch.from_numpy(cst).cuda()
        shift_d = torch.from_numpy(models[0].shift).cuda()
        log_Ps, log_pi0 = (torch.from_numpy(v).cuda() for v in group._transitions())
        say('--- group %d: %d models, %d states (classes 4 / 8 / 16 / 32: %s models)'
            % (gi, M, KT, _hip._hmm_grid_order(group.Ks)[1]))
        ll = _hip.arhmm_grid_loglik(z_d, off_d, G_d, cst_d, LAGS, shift=shift_d)
        gamma, xi, _ = _hip.hmm_grid_forward_backward(ll, off_d, group.Ks, log_Ps, log_pi0)
        us = event_window(lambda: _hip.arhmm_grid_loglik(z_d, off_d, G_d, cst_d, LAGS, shift=shift_d, out=ll),
                          args.iters)
        say('(c) bn_arhmm_grid_loglik:                   %9.1f us  (%.1f float64 TFLOP/s by 2 n KT D P flops)'
            % (us, 2.0 * n * KT * D * P / us * 1e-6))
        us = event_window(lambda: _hip.hmm_grid_forward_backward(ll, off_d, group.Ks, log_Ps, log_pi0, gamma=gamma,
                                                                 xi=xi), args.iters)
        say('(c) bn_hmm_grid_forward_backward:           %9.1f us  (%.2f us a model, both sweeps)' % (us, us / M))
        us = event_window(lambda: _hip.hmm_grid_forward_backward(ll, off_d, group.Ks, log_Ps, log_pi0,
                                                                 want_posteriors=False), args.iters)
        say('(c) bn_hmm_grid_forward_backward, lik only: %9.1f us  (%.2f us a model)' % (us, us / M))
        us = event_window(lambda: _hip.arhmm_grid_moments(z_d, off_d, gamma, LAGS, shift=shift_d), args.iters)
        say('(c) bn_arhmm_grid_moments:                  %9.1f us  (%.1f float64 TFLOP/s by n KT P (P + 1) flops)'
            % (us, 1.0 * n * KT * P * (P + 1) / us * 1e-6))
        del ll, gamma, xi
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
