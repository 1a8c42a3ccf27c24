"""One EM iteration of an ARHMM on a table of latents (models.arhmm.ARHMM, csrc/arhmm.hip), measured in ONE process
on --rows x 16 latents (default 10^6), K = 16 states, one lag, cut into trials two ways: 4,000 trials of 250 rows and
100 trials of 10^4 rows.

  (a) the host    the same iteration from the numpy restatement (tests/arhmm_refs.py: folded density, scaled
                  forward-backward trial by trial, einsum moments, the model's M-step) on the host copy of the table.
                  Host clock, once.
  (b) the device  ``ARHMM.em_step``: fold, three launches, one transfer of K (P^2 + K + 1) doubles, the M-step on the
                  host.  Host clock around work that ends with the parameters on the host, --reps times after a
                  warm-up.
  (c) the launches ``bn_arhmm_loglik``, ``bn_hmm_forward_backward`` (posteriors, and likelihood only),
                  ``bn_arhmm_moments`` and ``bn_hmm_viterbi`` alone, by hipEvents around --iters calls of the wrappers.
                  Forward-backward and Viterbi are chains in time: their cost is (longest trial) x (step latency), so
                  the line gives the time per row of the longest trial and no rate.
    python tools/bench_arhmm.py [--rows 1000000] [--reps 3] [--iters 5] [--skip-host] [--out FILE]
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

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM

K, D, LAGS = 16, 16, 1


def table(n, seed):
    """fp32 (n, D): a random walk pulled to one of K centres that changes every 40 rows or so."""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((K, D))
    z = np.repeat(rng.integers(0, K, size=n // 40 + 1), 40)[:n]
    x = np.zeros((n, D), dtype=np.float64)
    noise = 0.3 * rng.standard_normal((n, D))
    for t in range(1, n):
        x[t] = 0.8 * x[t - 1] + 0.2 * centres[z[t]] + noise[t]
    return x.astype(np.float32)


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
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    n = args.rows
    host = table(n, 1)
    z_d = torch.from_numpy(host).cuda()
    for n_trials in (n // 250, n // 10 ** 4):
        T = n // n_trials
        offsets = np.minimum(np.arange(n_trials + 1, dtype=np.int64) * T, n)
        offsets[-1] = n
        off_d = torch.from_numpy(offsets).cuda()
        say('--- %d x %d, K = %d, lags = %d: %d trials of %d rows' % (n, D, K, LAGS, n_trials, T))
        model = ARHMM(K, D, lags=LAGS)
        model.initialize(z_d, offsets, seed=0)
        start = pickle.dumps(model)
        model.em_step(z_d, offsets)                         # warm-up
        ours = []
        for _ in range(args.reps):
            model = pickle.loads(start)
            ms, lls = host_clock(lambda: model.em_step(z_d, offsets))
            ours.append(ms)
        say('(b) ARHMM.em_step on the device: %9.1f ms (min %.1f max %.1f over %d), log-likelihood %.6e'
            % (statistics.median(ours), min(ours), max(ours), len(ours), float(np.sum(lls))))
        if not args.skip_host:
            from tests import arhmm_refs as refs
            ref = pickle.loads(start)
            t0 = time.perf_counter()
            lls_h = refs.em_iteration(ref, host, offsets, second_form=True)
            ms_h = (time.perf_counter() - t0) * 1e3
            worst = max(np.abs(getattr(ref, a) - getattr(model, a)).max() for a in ('As', 'bs', 'Sigmas', 'log_Ps'))
            say('(a) the numpy restatement on the host:  %9.1f ms, log-likelihood %.6e; (a) / (b) = %.1f; largest '
                'parameter difference after the iteration %.2e' % (ms_h, float(np.sum(lls_h)), ms_h / statistics.median(ours), worst))
        model = pickle.loads(start)
        G, cst = model.fold()
        G_d, cst_d = torch.from_numpy(G).cuda(), torch.from_numpy(cst).cuda()
        shift_d = torch.from_numpy(model.shift).cuda()
        lp, l0 = torch.from_numpy(model.log_Ps).cuda(), torch.from_numpy(model.log_pi0).cuda()
        ll = _hip.arhmm_loglik(z_d, off_d, G_d, cst_d, LAGS, shift=shift_d)
        gamma, xi, _ = _hip.hmm_forward_backward(ll, off_d, lp, l0)
        us = event_window(lambda: _hip.arhmm_loglik(z_d, off_d, G_d, cst_d, LAGS, shift=shift_d, out=ll), args.iters)
        P = 1 + (LAGS + 1) * D
        say('(c) bn_arhmm_loglik:                   %9.1f us  (%.1f float64 GFLOP/s by 2 n K D P flops)'
            % (us, 2.0 * n * K * D * P / us * 1e-3))
        us = event_window(lambda: _hip.hmm_forward_backward(ll, off_d, lp, l0, gamma=gamma, xi=xi), args.iters)
        say('(c) bn_hmm_forward_backward:           %9.1f us  (%.1f ns a row of the longest trial, both sweeps)'
            % (us, us * 1e3 / T))
        us = event_window(lambda: _hip.hmm_forward_backward(ll, off_d, lp, l0, want_posteriors=False), args.iters)
        say('(c) bn_hmm_forward_backward, lik only: %9.1f us  (%.1f ns a row of the longest trial)' % (us, us * 1e3 / T))
        us = event_window(lambda: _hip.arhmm_moments(z_d, off_d, gamma, LAGS, shift=shift_d), args.iters)
        say('(c) bn_arhmm_moments:                  %9.1f us  (%.1f float64 GFLOP/s by n K P (P + 1) flops)'
            % (us, 1.0 * n * K * P * (P + 1) / us * 1e-3))
        us = event_window(lambda: _hip.hmm_viterbi(ll, off_d, lp, l0), args.iters)
        say('(c) bn_hmm_viterbi:                    %9.1f us  (%.1f ns a row of the longest trial, walk back included)'
            % (us, us * 1e3 / T))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
