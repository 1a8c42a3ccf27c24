"""Sampling from an ARHMM (models.arhmm.ARHMM.sample_table, bn_arhmm_sample in csrc/arhmm.hip), measured in ONE
process on trials of 1,200 rows (the reference's 1,000-frame trial plus 200 burn-in rows), D = 16 latents, K = 16
states, one lag: 50 trials (the reference's 50 samples) and 4,000 trials.

  (a) the host     restatement A of tests/arhmm_sample_refs.py (the plain loop over trials and rows, states by the
                   counting rule) on the host copies of the same noise.  Host clock, once.
  (b) the device   ``ARHMM.sample_table``: the Cholesky factors and cumulative sums on the host, their upload, the
                   noise from torch's device generator, one launch.  Host clock around work that ends with a
                   synchronize, --reps times after a warm-up.
  (c) the launch   ``_hip.arhmm_sample`` alone on resident operands, by hipEvents around at least --iters calls and
                   --window-ms of them: states sampled and states given, with sticky transition rows (0.95 on the
                   diagonal: the recursion reloads its matrix on a change of state only) and with uniform rows (a
                   change at 15 rows in 16).  The launch is a chain in time: its cost is (longest trial) x (step
                   latency), so the line gives the time per row of the longest trial.
    python tools/bench_arhmm_sample.py [--reps 5] [--iters 20] [--window-ms 300] [--skip-host] [--out FILE]
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

K, D, LAGS, T = 16, 16, 1, 1200


def model(stay, seed=0):
    rng = np.random.RandomState(seed)
    m = ARHMM(K, D, lags=LAGS)
    for k in range(K):
        m.As[k] = 0.5 * np.eye(D) + 0.2 / np.sqrt(D) * rng.randn(D, D)
        B = rng.randn(D, D)
        m.Sigmas[k] = B @ B.T / D + 0.2 * np.eye(D)
    m.bs = rng.randn(K, D)
    Ps = np.full((K, K), (1.0 - stay) / (K - 1)) + (stay - (1.0 - stay) / (K - 1)) * np.eye(K)
    m.log_Ps = np.log(Ps / Ps.sum(axis=1, keepdims=True))
    return m


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_window(fn, iters, window_ms):
    """Microseconds per call: hipEvents around at least ``iters`` calls and at least ``window_ms`` of them (a window of
    a few milliseconds measures the clock ramp as much as the kernels)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    while True:
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_ms:
            return ms / iters * 1e3
        iters = int(iters * max(2.0, 1.2 * window_ms / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--window-ms', type=float, default=300.0)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_arhmm_sample.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    sticky, uniform = model(0.95), model(1.0 / K)
    for n_trials in (50, 4000):
        n = n_trials * T
        offsets = np.arange(n_trials + 1, dtype=np.int64) * T
        say('--- %d trials of %d rows, D = %d, K = %d, lags = %d' % (n_trials, T, D, K, LAGS))
        sticky.sample_table(offsets, seed=0)                # warm-up
        ours = []
        for _ in range(args.reps):
            ms, (x, z) = host_clock(lambda: sticky.sample_table(offsets, seed=0))
            ours.append(ms)
        med = statistics.median(ours)
        say('(b) ARHMM.sample_table on the device:   %9.2f ms (min %.2f max %.2f over %d)'
            % (med, min(ours), max(ours), len(ours)))
        gen = torch.Generator(device='cuda')
        gen.manual_seed(0)
        eps = torch.randn((n, D), dtype=torch.float64, device='cuda', generator=gen)
        u = torch.rand((n,), dtype=torch.float64, device='cuda', generator=gen)
        if not args.skip_host:
            from tests import arhmm_sample_refs as sr
            eps_h, u_h = eps.cpu().numpy(), u.cpu().numpy()
            t0 = time.perf_counter()
            xa, za = sr.sample_a(*sticky.generative(), offsets, eps_h, u=u_h)
            ms_h = (time.perf_counter() - t0) * 1e3
            same = bool(np.array_equal(za, z.cpu().numpy()))
            say('(a) restatement A on the host:          %9.2f ms; (a) / (b) = %.1f; state paths equal: %s; largest '
                'difference of x %.2e' % (ms_h, ms_h / med, same, float(np.abs(xa - x.cpu().numpy()).max())))
        off_d = torch.from_numpy(offsets).cuda()
        x_out = torch.zeros((n, D), dtype=torch.float64, device='cuda')
        z_out = torch.zeros((n,), dtype=torch.int32, device='cuda')
        for name, m in (('sticky rows (0.95)', sticky), ('uniform rows', uniform)):
            ops = [torch.from_numpy(a).cuda() for a in m.generative()]
            us = event_window(lambda: _hip.arhmm_sample(*ops, off_d, eps, u=u, x=x_out, states_out=z_out), args.iters,
                              args.window_ms)
            changes = float((z_out.view(n_trials, T)[:, 1:] != z_out.view(n_trials, T)[:, :-1]).double().mean())
            say('(c) bn_arhmm_sample, states sampled, %-18s %9.1f us  (%.1f ns a row of the longest trial; the '
                'state changes at %.3f of the rows)' % (name + ':', us, us * 1e3 / T, changes))
            given = z_out.clone()
            # (the wrapper's range check of given states is one reduction and one host read: part of the call)
            us = event_window(lambda: _hip.arhmm_sample(*ops, off_d, eps, states=given, x=x_out, states_out=z_out),
                              args.iters, args.window_ms)
            say('(c) bn_arhmm_sample, states given,   %-18s %9.1f us  (%.1f ns a row of the longest trial)'
                % (name + ':', us, us * 1e3 / T))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
