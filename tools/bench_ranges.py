"""The ranges of a latent table (``compute_range``: the 5th, 95th and 50th percentile of every column), four ways, in
ONE process:

  (a) compute_range    this package's, end to end from a device table (host clock around the call, which ends with the
                       selected values on the host): one count, one select with six ranks a column, numpy's lerp
  (b) the two launches ``bn_column_count`` and ``bn_column_select`` alone, by hipEvents, with the bytes they have to
                       read by the algorithm (one count pass plus four histogram passes of n * d * 4; not measured
                       traffic) over the time, in GB/s
  (c) reference route  the same table copied to the host, then ``compute_range`` as the reference writes it: three
                       ``np.nanpercentile(values, p, axis=0)`` calls (host clock; the copy timed apart)
  (d) torch.sort       along dimension 0 on the device, by hipEvents: what a user could have reached for (it gives
                       the order statistics of NaN-free columns, and no interpolation yet)

(a) is checked against (c), exactly, before anything is timed.
    python tools/bench_ranges.py [--reps 7] [--out FILE]
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
from behavenet_amd.fitting.eval import percentile_plan
from behavenet_amd.plotting.cond_ae_utils import compute_range

SHAPES = [(10 ** 6, 16), (2 * 10 ** 5, 64)]


def reference_compute_range(values, min_p=5, max_p=95):
    return {'min': np.nanpercentile(values, min_p, axis=0), 'max': np.nanpercentile(values, max_p, axis=0),
            'med': np.nanpercentile(values, 50, axis=0)}


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def host_clock(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ms):
    return '%9.3f ms (min %.3f max %.3f over %d)' % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    for n, d in SHAPES:
        rng = np.random.default_rng(n + d)
        # latents as an encoder gives them: a scale and an offset per column
        host = (rng.standard_normal((n, d)) * rng.uniform(0.5, 20, size=d) + rng.uniform(-5, 5, size=d)).astype(np.float32)
        table = torch.from_numpy(host).cuda()
        want = reference_compute_range(host)
        got = compute_range([table])
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        say('table %d x %d float32 (%.1f MB): compute_range equals three np.nanpercentile calls, exactly'
            % (n, d, n * d * 4 / 1e6))
        cols, col_groups, slabs, rows = _hip.column_select_plan(n, d, 6)
        say('  partition: %d column groups of %d columns x %d row blocks of %d rows' % (col_groups, cols, slabs, rows))
        compute_range([table])          # (warm: the arena is sized)
        say('  (a) compute_range, device table -> dict on the host   %s' % fmt(host_clock(lambda: compute_range([table]),
                                                                                         args.reps)))
        n_valid = _hip.column_count(table).cpu().numpy()
        ranks = torch.from_numpy(percentile_plan(n_valid, (5, 95, 50))[0]).cuda()
        count_ms = events(lambda: _hip.column_count(table), args.reps)
        select_ms = events(lambda: _hip.column_select(table, ranks), args.reps)
        by_algorithm = 5 * n * d * 4
        both = statistics.median(count_ms) + statistics.median(select_ms)
        say('  (b) bn_column_count                                   %s' % fmt(count_ms))
        say('      bn_column_select, r = 6                           %s' % fmt(select_ms))
        say('      %.1f MB by the algorithm (five passes) in %.3f ms: %.0f GB/s'
            % (by_algorithm / 1e6, both, by_algorithm / both / 1e6))
        copy_ms = host_clock(lambda: table.cpu(), args.reps)
        ref_ms = host_clock(lambda: reference_compute_range(host), max(args.reps // 2, 3))
        say('  (c) copy of the table to the host                     %s' % fmt(copy_ms))
        say('      the reference\'s compute_range (3 x np.nanpercentile) %s' % fmt(ref_ms))
        sort_ms = events(lambda: torch.sort(table, dim=0), args.reps)
        say('  (d) torch.sort(table, dim=0) on the device            %s' % fmt(sort_ms))
        say('  (c) / (a) = %.0f; (d) / (b) = %.2f'
            % ((statistics.median(copy_ms) + statistics.median(ref_ms)) / statistics.median(
                host_clock(lambda: compute_range([table]), args.reps)), statistics.median(sort_ms) / both))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
