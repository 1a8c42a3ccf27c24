"""State runs and the syllable movie (bn_state_runs in csrc/state_runs.hip, bn_stamp_boxes_u8 and the mosaic in
csrc/frame_mosaic.hip, fitting.eval.syllable_movie_device), measured in ONE process.

  (a) the runs     an int32 state table of STATE_RUNS_TILE * STATE_RUNS_SCAN + STATE_RUNS_TILE + 5 rows (about a
                   million) in 1,000-row trials, K = 16, runs of 20 rows on average and of 2:
                   ``_hip.state_runs`` by a host clock around the call (its synchronisation is part of it) and the
                   launches alone by hipEvents (``bn_state_runs`` with resident operands); next to it the numpy
                   ``diff`` route on the host -- the table's transfer included -- which gives the same rows.
                   Bytes of the launches: the states are read twice (8 n), 16 bytes a run are written.
  (b) the movie    K = 16 states, max_frames = 400, 1 x 128 x 128 uint8 frames (the benchmark's frame size) of 40
                   trials of 1,000 frames resident on the device: ``syllable_movie_device`` by a host clock, its
                   mosaic launches and its stamp launch by hipEvents.  Bytes of a mosaic launch: one byte read and
                   one written per pixel shown, one written per blank pixel.

    python tools/bench_syllables.py [--reps 5] [--iters 20] [--window-ms 300] [--out FILE]
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
from behavenet_amd.fitting import eval as ev

K = 16
HBM_TBS = 6.3           # what a copy achieves on the device (8 TB/s on paper)


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_window(fn, iters, window_ms):
    """Microseconds per call: hipEvents around at least ``iters`` calls and at least ``window_ms`` of them."""
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


def sticky(rng, n, mean):
    lengths = rng.geometric(1.0 / mean, size=int(2 * n / mean) + 16)
    states = rng.randint(0, K, size=len(lengths))
    same = np.nonzero(states[1:] == states[:-1])[0] + 1
    states[same] = (states[same - 1] + 1) % K                   # (a chain of repeats may still repeat: harmless)
    return np.repeat(states, lengths)[:n].astype(np.int32)


def numpy_runs(states_d, offsets):
    """The host route: the table crosses, then one diff over it with the trial starts forced."""
    s = states_d.cpu().numpy()
    start = np.ones(len(s), dtype=bool)
    start[1:] = s[1:] != s[:-1]
    start[offsets[:-1][offsets[:-1] < len(s)]] = True
    beg = np.nonzero(start)[0]
    end = np.append(beg[1:], len(s))
    trial = np.searchsorted(offsets, beg, side='right') - 1
    return np.stack([trial, beg - offsets[trial], end - offsets[trial], s[beg]], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--window-ms', type=float, default=300.0)
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_syllables.py measures on a GPU; none is visible')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('device: %s' % torch.cuda.get_device_name(0))
    rng = np.random.RandomState(0)
    lib = _hip.load()
    n = _hip.STATE_RUNS_TILE * _hip.STATE_RUNS_SCAN + _hip.STATE_RUNS_TILE + 5
    offsets = np.append(np.arange(0, n, 1000), n).astype(np.int64)
    S = len(offsets) - 1
    off_d = torch.from_numpy(offsets).cuda()
    for mean in (20, 2):
        states = torch.from_numpy(sticky(rng, n, mean)).cuda()
        say('--- (a) %d rows in %d trials, K = %d, runs of %d rows on average' % (n, S, K, mean))
        _hip.state_runs(states, off_d, K)
        ours = [host_clock(lambda: _hip.state_runs(states, off_d, K)) for _ in range(args.reps)]
        runs = ours[-1][1][0]
        R = int(runs.shape[0])
        ours = [ms for ms, _ in ours]
        host = [host_clock(lambda: numpy_runs(states, offsets)) for _ in range(args.reps)]
        same = bool(np.array_equal(host[-1][1], runs.cpu().numpy()))
        host = [ms for ms, _ in host]
        say('_hip.state_runs (launches, one synchronisation, trim):  %8.3f ms (min %.3f max %.3f over %d); %d runs'
            % (statistics.median(ours), min(ours), max(ours), len(ours), R))
        say('numpy diff on the host, the transfer included:          %8.3f ms (min %.3f max %.3f over %d); same rows: %s'
            % (statistics.median(host), min(host), max(host), len(host), same))
        out = torch.empty((n, 4), dtype=torch.int32, device='cuda')
        stats = torch.zeros((K + K * K + 2,), dtype=torch.int64, device='cuda')
        nbytes = lib.bn_state_runs_ws_bytes(n, S, K)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
        at, st = stats.data_ptr(), torch.cuda.current_stream().cuda_stream

        def launch():
            rc = lib.bn_state_runs(states.data_ptr(), off_d.data_ptr(), S, K, n, out.data_ptr(), n, at, at + 8 * K,
                                   at + 8 * (K + K * K), at + 8 * (K + K * K + 1), ws.data_ptr(), nbytes, st)
            assert rc == 0
        us = event_window(launch, args.iters, args.window_ms)
        moved = 8 * n + 16 * R
        say('bn_state_runs, the five launches alone:                 %8.1f us; %.2f MB moved (states twice, 16 B a run): '
            '%.3f TB/s, %.1f %% of %.1f TB/s' % (us, moved / 1e6, moved / us / 1e6, 100 * moved / us / 1e6 / HBM_TBS,
                                               HBM_TBS))
    # ---------------------------------------------------------------------------------------------- (b)
    C, H, W, n_trials, T = 1, 128, 128, 40, 1000
    say('--- (b) the movie: K = %d, max_frames = 400, %d x %d x %d uint8 frames, %d trials of %d frames on the device'
        % (K, C, H, W, n_trials, T))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    trials = [torch.randint(0, 256, (T, C, H, W), dtype=torch.uint8, device='cuda', generator=gen)
              for _ in range(n_trials)]
    lengths = np.full(n_trials, T, dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lengths)))
    runs, _, _ = _hip.state_runs(torch.from_numpy(sticky(rng, int(off[-1]), 20)).cuda(), off, K)
    ms, chunks = host_clock(lambda: ev.discrete_chunks(runs, K, lengths))
    instances = ev.syllable_instances(chunks, min_threshold=5, seed=0)
    say('discrete_chunks of %d runs on the host: %.2f ms' % (int(runs.shape[0]), ms))
    ms, plan = host_clock(lambda: ev.syllable_movie_plan(instances, max_frames=400))
    src, mark, n_rows, n_cols = plan
    say('syllable_movie_plan: %.2f ms; %d movie frames of %d x %d panels, %d panels shown, %d marked'
        % (ms, len(src), n_rows, n_cols, int((src[..., 0] >= 0).sum()), int(mark.sum())))
    ev.syllable_movie_device(trials, instances, max_frames=400)
    ours = [host_clock(lambda: ev.syllable_movie_device(trials, instances, max_frames=400)) for _ in range(args.reps)]
    movie = ours[-1][1][0]
    ours = [m for m, _ in ours]
    say('syllable_movie_device (plan, gather of the clips\' rows, mosaic, stamp): %8.2f ms (min %.2f max %.2f over %d); '
        'movie %s, %.1f MB' % (statistics.median(ours), min(ours), max(ours), len(ours), tuple(movie.shape),
                               movie.numel() / 1e6))
    # the launches alone: planes of the frames shown once each, the plan's sources, chunks of 200 movie frames
    shown = int((src[..., 0] >= 0).sum())
    planes = torch.randint(0, 256, (shown, 1, H, W), dtype=torch.uint8, device='cuda', generator=gen)
    flat = np.full(src.shape[:3], -1, dtype=np.int32)
    flat[src[..., 0] >= 0] = np.arange(shown, dtype=np.int32)
    parts = [torch.from_numpy(np.ascontiguousarray(flat[b:b + 200])).cuda() for b in range(0, len(flat), 200)]
    us = event_window(lambda: [_hip.frame_mosaic_u8(planes, p, 0, None) for p in parts], args.iters, args.window_ms)
    moved = shown * H * W + movie.numel()
    say('the %d mosaic launches alone:   %8.1f us; %.1f MB moved (a byte read per pixel shown, a byte written per pixel): '
        '%.3f TB/s, %.1f %% of %.1f TB/s' % (len(parts), us, moved / 1e6, moved / us / 1e6,
                                           100 * moved / us / 1e6 / HBM_TBS, HBM_TBS))
    mark_d = torch.from_numpy(mark).cuda()
    us = event_window(lambda: _hip.stamp_boxes_u8(movie, mark_d, (C * H, W)), args.iters, args.window_ms)
    say('bn_stamp_boxes_u8 alone:        %8.1f us; %d panels read their mark, %d write 100 bytes each (latency, not '
        'bandwidth)' % (us, mark.size, int(mark.sum())))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
