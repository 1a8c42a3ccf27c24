"""The session classifier on latents (fitting.eval.session_classifier, csrc/softmax_cv.hip), measured in ONE process on
a table of --rows latents of 4 sessions (default 10^6 x 16: 4,000 trials of 250 frames, 16 unsupervised latents; and
10^6 x 64, the widest table served):

  (a) sklearn     ``LogisticRegressionCV(Cs=<8 values>, cv=5, penalty='l2', multi_class='multinomial')`` as the
                  reference's ``fit_classifier`` calls it, on the host copy of the table, then ``accuracy_score`` on a
                  held-out table of a tenth of the rows.  Host clock.
  (b) the device  what ``session_classifier`` does with the table once the trials are encoded:
                  ``fitting.eval.classify_table`` (folds, 40 models in lockstep, held-out scores, refit; defaults
                  tol = 1e-4, max_iter = 100) and ``score_table`` on the held-out table.  Host clock around work that
                  ends with the numbers on the host; alternated with (a), --reps times.
  (c) the launch  ``bn_softmax_cv_lossgrad`` alone at M = 40 and M = 1 (S = 4), by hipEvents around --iters calls of
                  the wrapper, warm-up first, the cases alternated in --reps windows: microseconds, GB/s by the
                  algorithm's bytes (table, classes and folds read once; not measured traffic) and float64 GFLOP/s by
                  the algorithm's 4 M S (D + 1) flops a row.
    python tools/bench_session_classifier.py [--rows 1000000] [--reps 2] [--iters 20] [--skip-sklearn] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.classifier import DEFAULT_CS
from behavenet_amd.fitting.eval import classify_table, score_table

PEAK_GBS = 8000.0
PEAK_FP64_GFLOPS = 78600.0
S = 4


def table(n, D, seed):
    """fp32 (n, D) rows of four overlapping Gaussian classes of unequal size, in session order, and their classes."""
    rng = np.random.default_rng([seed, D])
    sizes = (np.array([0.4, 0.3, 0.2, 0.1]) * n).astype(int)
    sizes[0] += n - sizes.sum()
    centres = 0.5 * np.random.default_rng([7, D]).standard_normal((S, D))
    z = np.concatenate([centres[k] + rng.standard_normal((m, D)) for k, m in enumerate(sizes)]).astype(np.float32)
    return z, np.concatenate([np.full(m, k, dtype=np.int32) for k, m in enumerate(sizes)])


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def sklearn_route(z, y, z_held, y_held):
    from sklearn.linear_model import LogisticRegressionCV
    from sklearn.metrics import accuracy_score
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            lr = LogisticRegressionCV(Cs=list(DEFAULT_CS), cv=5, penalty='l2', multi_class='multinomial')
        except TypeError:
            lr = LogisticRegressionCV(Cs=list(DEFAULT_CS), cv=5, penalty='l2')
        lr.fit(z, y)
    return accuracy_score(y_held, lr.predict(z_held)), lr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-sklearn', action='store_true')
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_session_classifier.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    n = args.rows
    for D in (16, 64):
        z, y = table(n, D, 1)
        z_held, y_held = table(n // 10, D, 2)
        z_d, held_d = torch.from_numpy(z).cuda(), torch.from_numpy(z_held).cuda()

        def device_route():
            lr = classify_table(z_d, y, S)
            hits, rows = score_table(held_d, y_held, lr.weights_)
            return hits / rows, lr
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            device_route()                                  # warm-up
            ours, theirs, fc, lr, fc_sk, sk = [], [], None, None, None, None
            for _ in range(args.reps):
                ms, (fc, lr) = host_clock(device_route)
                ours.append(ms)
                if not args.skip_sklearn:
                    ms, (fc_sk, sk) = host_clock(lambda: sklearn_route(z, y, z_held, y_held))
                    theirs.append(ms)
        say('(a, b) %d x %d, 4 sessions, 5 folds x 8 values of C, tol 1e-4, max_iter 100, held-out table of %d rows'
            % (n, D, len(y_held)))
        say('    classify_table + score_table on the device table    %10.1f ms (min %.1f max %.1f over %d); fc %.6f, C_ %g, '
            'iterations of the 40 models %d to %d, of the refit %d, all converged: %s'
            % (statistics.median(ours), min(ours), max(ours), args.reps, fc, lr.C_, lr.n_iter_.min(), lr.n_iter_.max(),
               lr.refit_n_iter_, lr.converged_))
        if theirs:
            say('    sklearn LogisticRegressionCV + accuracy_score, host  %10.1f ms (min %.1f max %.1f over %d); fc %.6f, C_ %g'
                % (statistics.median(theirs), min(theirs), max(theirs), args.reps, fc_sk, sk.C_[0]))
            say('    largest difference of the fold scores %.2e; (a) / (b) = %.1f'
                % (np.abs(lr.scores_ - sk.scores_[sk.classes_[-1]]).max(), statistics.median(theirs) / statistics.median(ours)))
        else:
            say('    sklearn: not measured (--skip-sklearn)')

        # (c) one launch
        g = torch.Generator(device='cuda').manual_seed(3)
        y_d = torch.from_numpy(y).cuda()
        fold_d = torch.randint(0, 5, (n,), device='cuda', generator=g, dtype=torch.int32)
        fns = {}
        for M in (40, 1):
            W = torch.randn((M, S, D + 1), device='cuda', generator=g, dtype=torch.float64) / D ** 0.5
            leave = torch.tensor([(m % 6) - 1 for m in range(M)], dtype=torch.int32, device='cuda')
            fns[M] = (lambda W=W, leave=leave: _hip.softmax_cv_lossgrad(z_d, y_d, fold_d, W, leave))
        for fn in fns.values():
            event_window(fn, 2)
        us = {M: [] for M in fns}
        for _ in range(max(args.reps, 5)):
            for M, fn in fns.items():
                us[M].append(event_window(fn, args.iters))
        nbytes = n * (D * 4 + 8)
        for M in fns:
            med = statistics.median(us[M])
            flops = 4.0 * n * M * S * (D + 1)
            gbs, gf = nbytes / 1e9 / (med * 1e-6), flops / 1e9 / (med * 1e-6)
            blocks, rows, mg = _hip._softmax_cv_plan(n, D, S, M)
            say('(c) bn_softmax_cv_lossgrad %d x %d, S = 4, M = %2d: %9.1f us (min %.1f max %.1f over %d alternated windows of %d '
                'calls); %.0f MB by the algorithm = %.0f GB/s = %.1f %% of the %.0f GB/s peak; %.1f GFLOP float64 = %.0f '
                'GFLOP/s = %.1f %% of the %.0f peak; %d row blocks of %d rows x %d model groups'
                % (n, D, M, med, min(us[M]), max(us[M]), len(us[M]), args.iters, nbytes / 1e6, gbs, 100 * gbs / PEAK_GBS,
                   PEAK_GBS, flops / 1e9, gf, 100 * gf / PEAK_FP64_GFLOPS, PEAK_FP64_GFLOPS, blocks, rows, -(-M // mg)))
        del z_d, held_d, fns
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
