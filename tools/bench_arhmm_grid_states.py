"""The states, runs and statistics of a GRID of ARHMMs on one table of latents (ARHMMGroup.table_runs,
bn_hmm_grid_viterbi), measured in ONE process on tools/bench_arhmm_grid.py's own problem: --rows x 16 latents (default
10^6) cut into trials of 250 rows, one lag, K in {2, 4, 8, 16, 32} x 4 values of kappa x 3 seeds -- 60 models, 744
states, cut into groups by fitting.eval.arhmm_grid_groups.  The models are initialised and advanced one EM iteration,
so the paths are those of models that have seen the table.

  (a) one by one   ``ARHMM.table_runs`` for the 60 models in turn: a log-likelihood launch, a Viterbi launch, the run
                   search and a synchronisation each (the route before the group had a decoding half).
  (b) the group    ``ARHMMGroup.table_runs`` per group: one log-likelihood launch, one Viterbi launch a class, the
                   run searches without a synchronisation between them, two transfers.
                   (a) and (b) alternate, --reps times after a warm-up of each; host clock around work that ends with
                   the results on the host; median, minimum and maximum of the windows are reported.
  (c) Viterbi alone  ``bn_hmm_viterbi`` for the models of a group in turn against ``bn_hmm_grid_viterbi`` for the
                   group, on the same ll, by hipEvents around --iters calls, the two alternating --reps times.
    python tools/bench_arhmm_grid_states.py [--rows 1000000] [--reps 10] [--iters 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import arhmm_grid, arhmm_grid_groups
from behavenet_amd.models.arhmm import ARHMM, ARHMMGroup
from tools.bench_arhmm_grid import D, KAPPAS, LAGS, SEEDS, STATES, TRIAL, event_window, host_clock, table


def spread(ts):
    return '%9.1f (min %.1f max %.1f over %d)' % (statistics.median(ts), min(ts), max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm_grid_states.py measures on a GPU; none is visible')
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
    for m, c in zip(models, grid):
        m.initialize(z_d, offsets, seed=c['rng_seed_model'])
    for g in groups:
        ARHMMGroup([models[i] for i in g]).em_step(z_d, off_d)

    def one_by_one():
        return [m.table_runs(z_d, off_d) for m in models]

    def grouped():
        out = [None] * len(models)
        for g in groups:
            for i, triple in zip(g, ARHMMGroup([models[i] for i in g]).table_runs(z_d, off_d)):
                out[i] = triple
        return out

    one_by_one()                                            # warm-up of both routes
    grouped()
    t_single, t_group = [], []
    for _ in range(args.reps):
        ms, a = host_clock(one_by_one)
        t_single.append(ms)
        ms, b = host_clock(grouped)
        t_group.append(ms)
    same = all(np.array_equal(u, v) for x, y in zip(a, b) for u, v in zip(x, y))
    say('(a) ARHMM.table_runs, %d models in turn: %s ms' % (len(models), spread(t_single)))
    say('(b) ARHMMGroup.table_runs, %d groups:    %s ms; (a) / (b) = %.2f'
        % (len(groups), spread(t_group), statistics.median(t_single) / statistics.median(t_group)))
    say('    runs, frames and transition counts of the two routes are %s; %d runs in all'
        % ('identical' if same else 'DIFFERENT', sum(len(x[0]) for x in b)))

    for gi, g in enumerate(groups):
        members = [models[i] for i in g]
        group = ARHMMGroup(members)
        say('--- group %d: %d models, %d states (classes 4 / 8 / 16 / 32: %s models)'
            % (gi, group.M, group.KT, _hip._hmm_grid_order(group.Ks)[1]))
        ll = group._loglik_table(z_d, off_d)
        log_Ps, log_pi0 = (torch.from_numpy(v).cuda() for v in group._transitions())
        own = [(ll[:, group.koff[i]:group.koff[i + 1]].contiguous(), torch.from_numpy(m.log_Ps).cuda(),
                torch.from_numpy(m.log_pi0).cuda()) for i, m in enumerate(members)]
        out = torch.zeros((group.M, n), dtype=torch.int32, device=ll.device)

        def single():
            for l, p, p0 in own:
                _hip.hmm_viterbi(l, off_d, p, p0)

        def packed():
            _hip.hmm_grid_viterbi(ll, off_d, group.Ks, log_Ps, log_pi0, out=out)
        u_single, u_packed = [], []
        for _ in range(args.reps):
            u_single.append(event_window(single, args.iters))
            u_packed.append(event_window(packed, args.iters))
        say('(c) bn_hmm_viterbi, %3d models in turn: %s us' % (group.M, spread(u_single)))
        say('(c) bn_hmm_grid_viterbi, one call:      %s us  (%.2f us a model); in turn / one call = %.2f'
            % (spread(u_packed), statistics.median(u_packed) / group.M,
               statistics.median(u_single) / statistics.median(u_packed)))
        del ll, own, out
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
