"""Exact multi-step forecasts of an ARHMM and their sums (bn_arhmm_forecast_sums in csrc/arhmm.hip,
``ARHMM.forecast_sums``), measured in ONE process on --rows x 16 latents (default 10^6), K = 16 states, one lag, cut
into 4,000 trials of 250 rows, for H = 1, 4, 10 and 32 horizons.

  (a) end to end   ``ARHMM.forecast_sums``: the maps on the host, fold, log-likelihoods, causal weights, the fused
                   launch and ONE transfer of (H, S, D, 5) doubles.  Host clock around work that ends on the host,
                   --reps times after a warm-up.
  (b) the launch   ``bn_arhmm_forecast_sums`` alone (plan, fold of the maps, product with scoring, combine) from device
                   operands, with its float64 rate by 2 n K Q H D flops.  hipEvents around --iters calls.
  (c) the loop     the unfused route on the same table and weights, from kernels that were there before the fused one:
                   H rounds of ``bn_arhmm_predict`` with the map of the round's horizon, the shift of its (n, D) float64
                   forecasts to their target rows with the rounding to fp32 and two ``bn_segment_label_sums``
                   launches (model and persistence).  The valid-row masks of the H rounds are made before the clock
                   starts.  hipEvents around --loop-iters passes.
(b) and (c) alternate --reps times in the same process; the lines give the median with the smallest and the largest.
    python tools/bench_arhmm_forecast.py [--rows 1000000] [--reps 3] [--iters 20] [--loop-iters 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.models.arhmm import ARHMM
from tools.bench_arhmm import D, K, LAGS, event_window, host_clock, table

HORIZONS = (1, 4, 10, 32)


def spread(v):
    return '%9.1f us (min %.1f max %.1f over %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--loop-iters', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm_forecast.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    n = args.rows
    z_d = torch.from_numpy(table(n, 1)).cuda()
    Q = 1 + LAGS * D
    n_trials = max(n // 250, 1)
    T = n // n_trials
    offsets = np.minimum(np.arange(n_trials + 1, dtype=np.int64) * T, n)
    offsets[-1] = n
    off_d = torch.from_numpy(offsets).cuda()
    say('--- %d x %d, K = %d, lags = %d: %d trials of %d rows' % (n, D, K, LAGS, n_trials, T))
    model = ARHMM(K, D, lags=LAGS)
    model.initialize(z_d, offsets, seed=0)
    model.em_step(z_d, offsets)
    model.em_step(z_d, offsets)
    w = model.table_weights(z_d, off_d)
    first = max(LAGS, 1)
    e = off_d.clamp(0, n)
    for H in HORIZONS:
        model.forecast_sums(z_d, off_d, H)                  # warm-up
        ours = [host_clock(lambda: model.forecast_sums(z_d, off_d, H)) for _ in range(args.reps)]
        sums = ours[-1][1]
        ms = [o[0] for o in ours]
        tot = sums.sum(axis=2)                              # (2, H, D, 4) over the trials
        ss = tot[..., 2] - tot[..., 1] ** 2 / tot[..., 0]
        r2 = 1.0 - tot[..., 3].sum(axis=2) / ss.sum(axis=2)
        say('H = %2d (a) ARHMM.forecast_sums end to end:      %9.1f ms (min %.1f max %.1f over %d); pooled R2 at '
            'h = %d: %.4f, of persistence %.4f'
            % (H, statistics.median(ms), min(ms), max(ms), len(ms), H, r2[0, -1], r2[1, -1]))
        N_d = torch.from_numpy(model.forecast_maps(H)).cuda()
        out = torch.zeros((H, n_trials, D, 5), dtype=torch.float64, device='cuda')
        masks, ones = [], torch.ones_like(e[:-1], dtype=torch.int32)
        for h in range(1, H + 1):
            beg = torch.minimum(e[:-1] + first + h - 1, e[1:])
            steps = torch.zeros((n + 1,), dtype=torch.int32, device='cuda')
            steps.index_add_(0, beg, ones)
            steps.index_add_(0, torch.maximum(e[1:], beg), -ones)
            masks.append((steps.cumsum(0)[:n] > 0).to(torch.float32)[:, None].expand(-1, D).contiguous())
        xhat = torch.zeros((n, D), dtype=torch.float64, device='cuda')
        moved = torch.zeros((n, D), dtype=torch.float32, device='cuda')
        back = torch.zeros((n, D), dtype=torch.float32, device='cuda')
        loop_sums = [None] * H

        def fused():
            return _hip.arhmm_forecast_sums(z_d, off_d, N_d, w, LAGS, out=out)

        def loop():
            for h in range(1, H + 1):
                _hip.arhmm_predict(z_d, off_d, N_d[h - 1], w, LAGS, out=xhat)
                moved[h - 1:] = xhat[:n - h + 1]            # to the target rows, rounded to the table's format
                back[h:] = z_d[:n - h]                      # x_{t-1} of the origin, seen from the target row
                loop_sums[h - 1] = (_hip.segment_label_sums(moved, z_d, masks[h - 1], off_d),
                                    _hip.segment_label_sums(back, z_d, masks[h - 1], off_d))
        fused()
        loop()
        us_f, us_l = [], []
        for _ in range(args.reps):
            us_f.append(event_window(fused, args.iters))
            us_l.append(event_window(loop, args.loop_iters))
        five = out.cpu().numpy()
        unf = np.stack([np.stack([a.cpu().numpy() for a, _ in loop_sums]),
                        np.stack([b.cpu().numpy() for _, b in loop_sums])])
        ours5 = np.stack([five[..., :4], five[..., [0, 1, 2, 4]]])
        assert np.array_equal(ours5[..., 0], unf[..., 0])
        diff = np.abs(ours5 - unf).sum(axis=2) / np.maximum(np.abs(unf).sum(axis=2), 1e-300)
        fl = 2.0 * n * K * Q * H * D
        say('H = %2d (b) bn_arhmm_forecast_sums:              %s  (%.1f float64 GFLOP/s by 2 n K Q H D flops)'
            % (H, spread(us_f), fl / statistics.median(us_f) * 1e-3))
        say('H = %2d (c) the unfused loop of %2d rounds:        %s  loop / fused = %.2f; largest relative difference '
            'of the pooled sums %.1e (the loop rounds xhat to fp32)'
            % (H, H, spread(us_l), statistics.median(us_l) / statistics.median(us_f), float(diff.max())))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
