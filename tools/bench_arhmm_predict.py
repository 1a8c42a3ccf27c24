"""One-step-ahead predictions of an ARHMM and their sums (bn_hmm_predictive, bn_arhmm_predict in csrc/arhmm.hip,
``ARHMM.prediction_sums``), measured in ONE process on --rows x 16 latents (default 10^6), K = 16 states, one lag, cut
into trials two ways: 4,000 trials of 250 rows and 100 trials of 10^4 rows.

  (a) the host     the numpy restatement (tests/arhmm_predict_refs.py: scaled weights trial by trial, one einsum a
                   trial) on the host copy of the table, from the device's log-likelihoods.  Host clock, once.
  (b) the device   ``ARHMM.prediction_sums``: fold, log-likelihoods, weights, the product, two segment reductions and
                   ONE transfer of (2, S, D, 4) doubles.  Host clock around work that ends on the host, --reps times
                   after a warm-up.
  (c) torch        the same predictions by a float64 ``torch.einsum`` over (state, history entry) on the device, from
                   the same weights: what a user without the kernel would write.  hipEvents.
  (d) the launches ``bn_hmm_predictive`` against ``bn_hmm_forward_backward``'s forward sweep on the same table (it is
                   that sweep plus one store a step: a chain in time, so the line gives the time per row of the
                   longest trial), and ``bn_arhmm_predict`` with its float64 rate by 2 n K Q D flops and its traffic by
                   the bytes it must move (the table once, the weights once, the predictions once).
    python tools/bench_arhmm_predict.py [--rows 1000000] [--reps 3] [--iters 5] [--skip-host] [--out FILE]
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
from behavenet_amd.models.arhmm import ARHMM
from tools.bench_arhmm import D, K, LAGS, event_window, host_clock, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm_predict.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    n = args.rows
    host = table(n, 1)
    z_d = torch.from_numpy(host).cuda()
    Q = 1 + LAGS * D
    for n_trials in (n // 250, n // 10 ** 4):
        T = n // n_trials
        offsets = np.minimum(np.arange(n_trials + 1, dtype=np.int64) * T, n)
        offsets[-1] = n
        off_d = torch.from_numpy(offsets).cuda()
        say('--- %d x %d, K = %d, lags = %d: %d trials of %d rows' % (n, D, K, LAGS, n_trials, T))
        model = ARHMM(K, D, lags=LAGS)
        model.initialize(z_d, offsets, seed=0)
        model.em_step(z_d, offsets)
        model.em_step(z_d, offsets)
        model.prediction_sums(z_d, off_d)                   # warm-up
        ours = []
        for _ in range(args.reps):
            ms, sums = host_clock(lambda: model.prediction_sums(z_d, off_d))
            ours.append(ms)
        tot = sums.sum(axis=1)
        ss = tot[:, :, 2] - tot[:, :, 1] ** 2 / tot[:, :, 0]
        say('(b) ARHMM.prediction_sums on the device: %9.1f ms (min %.1f max %.1f over %d); pooled R2 %.6f, of '
            'persistence %.6f' % (statistics.median(ours), min(ours), max(ours), len(ours),
                                  1.0 - tot[0, :, 3].sum() / ss[0].sum(), 1.0 - tot[1, :, 3].sum() / ss[1].sum()))
        G, cst = model.fold()
        lp, l0 = torch.from_numpy(model.log_Ps).cuda(), torch.from_numpy(model.log_pi0).cuda()
        W_d = torch.from_numpy(model.generative()[0]).cuda()
        ll = _hip.arhmm_loglik(z_d, off_d, G, cst, LAGS, shift=model.shift)
        w = _hip.hmm_predictive(ll, off_d, lp, l0)
        xhat = _hip.arhmm_predict(z_d, off_d, W_d, w, LAGS)
        if not args.skip_host:
            from tests import arhmm_predict_refs as prefs
            ll_h, W_h = ll.cpu().numpy(), model.generative()[0]
            t0 = time.perf_counter()
            w_h = prefs.weights_table(ll_h, offsets, model.log_Ps, model.log_pi0, prefs.weights_scaled)
            x_h = prefs.predict_einsum(host, offsets, W_h, w_h, LAGS)
            ms_h = (time.perf_counter() - t0) * 1e3
            say('(a) the numpy restatement on the host:   %9.1f ms (weights and predictions, no sums); largest '
                'difference of the weights %.2e, of the predictions %.2e'
                % (ms_h, np.abs(w_h - w.cpu().numpy()).max(), np.abs(x_h - xhat.cpu().numpy()).max()))

        def by_einsum():
            # phi (n, Q) in float64 from the shifted table; rows that are not AR rows are not masked (the timing's
            # favour goes to torch)
            prev = torch.zeros((n, D), dtype=torch.float64, device=z_d.device)
            prev[1:] = z_d[:-1]
            phi = torch.cat([torch.ones((n, 1), dtype=torch.float64, device=z_d.device), prev], dim=1)
            return torch.einsum('tk,tq,kdq->td', w, phi, W_d)
        x_t = by_einsum()
        us = event_window(by_einsum, args.iters)
        ar = torch.ones(n, dtype=torch.bool, device=z_d.device)
        ar[off_d[:-1]] = False
        say('(c) float64 torch.einsum on the device:  %9.1f us  (largest difference from bn_arhmm_predict on the AR '
            'rows %.2e)' % (us, float((x_t - xhat)[ar].abs().max())))
        us_p = event_window(lambda: _hip.hmm_predictive(ll, off_d, lp, l0, out=w), args.iters)
        us_f = event_window(lambda: _hip.hmm_forward_backward(ll, off_d, lp, l0, want_posteriors=False), args.iters)
        say('(d) bn_hmm_predictive:                   %9.1f us  (%.1f ns a row of the longest trial)'
            % (us_p, us_p * 1e3 / T))
        say('(d) bn_hmm_forward_backward, lik only:   %9.1f us  (%.1f ns a row of the longest trial); predictive / '
            'forward = %.2f' % (us_f, us_f * 1e3 / T, us_p / us_f))
        us = event_window(lambda: _hip.arhmm_predict(z_d, off_d, W_d, w, LAGS, out=xhat), args.iters)
        moved = n * (4.0 * D + 8.0 * K + 8.0 * D)
        say('(d) bn_arhmm_predict:                    %9.1f us  (%.1f float64 GFLOP/s by 2 n K Q D flops; %.1f GB/s by '
            'the table, the weights and the predictions once)' % (us, 2.0 * n * K * Q * D / us * 1e-3, moved / us * 1e-3))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
