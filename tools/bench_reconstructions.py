"""uint8 reconstructions of device-resident uint8 trials, four ways, alternated in ONE process.

  (a) host     ``get_reconstruction`` from images (fp32 frames cross to the host), then the rounding rule in numpy
               (``tests/recon_u8_refs.quantise_u8``): what there was before ``reconstruct_trial``
  (b) fp32     ``reconstruct_trial``, no key: the model's fp32 forward + ``bn_unit_float_to_u8``, uint8 to the host
  (c) fused    both bf16 keys as ``reconstruct_trial`` runs them: the layer onto the frame writes the grey levels
               (``bn_convT2d_last_bf16_u8``), the fp32 x_hat is never written
  (d) unfused  both bf16 keys; the bf16 decoder writes x_hat, ``bn_unit_float_to_u8`` reads it back

Every variant ends with the uint8 frames of the trial on the HOST.  Per shape every variant is warmed first, then windows
of at least --window seconds alternate --reps times with a device synchronise around each: ms per trial and frames/s
(median, with the spread over the windows).  Then the two last-layer variants alone, hipEvents around --layer-iters
back-to-back launches on operands of the layer's shapes, with the bytes each has to move; then
``export_reconstructions`` end to end, from a trial store on local disk to one, with --export-trials trials.
    python tools/bench_reconstructions.py [--reps 5] [--window 1.0] [--layer-iters 50] [--export-trials 40]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.data.data_generator import ConcatSessionsGenerator
from behavenet_amd.data.trial_store import write_npz_session
from behavenet_amd.fitting import eval as ev
from tests.recon_u8_refs import quantise_u8
from tools.bench_decode import SHAPES, build, event_ms, window

VARIANTS = ('host', 'fp32', 'fused', 'unfused')


def variants(model):
    def host(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        return quantise_u8(ev.get_reconstruction(model, y, dataset=0))

    def fp32(y):
        model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
        return ev.reconstruct_trial(model, y, 0, chunk_size=1024)

    def fused(y):
        model.hparams.update(hip_decode_dtype='bf16', hip_encode_dtype='bf16')
        return ev.reconstruct_trial(model, y, 0, chunk_size=1024)

    def unfused(y):
        with hf.encode_precision('bf16'), hf.decode_precision('bf16'):
            return ev._reconstruct_trial_device(model, y, 0, None, None, 1024, fused=False).cpu().numpy()
    return {'host': host, 'fp32': fp32, 'fused': fused, 'unfused': unfused}


def last_layer(name, model, y, iters):
    dec = model.decoding
    layer = dec._plan[-1]
    n = y.shape[0]
    w, b = [p.detach().contiguous() for p in dec._stack_params(None)[-2:]]
    g = layer.geom(n)
    if not _hip.convT2d_bf16_ok(g, last=True):
        print('%-14s the last layer is not the vector-unit layer: nothing to compare' % name)
        return
    a16 = (torch.randn((n, layer.hin, layer.win, layer.cin), device='cuda') * 0.5).to(torch.bfloat16)
    x_hat = torch.empty((n, layer.cout, layer.hout, layer.wout), device='cuda')
    out = torch.empty(x_hat.shape, dtype=torch.uint8, device='cuda')

    def two():
        _hip.convT2d_last_bf16(a16, w, b, g, layer.act, hf.LRELU_SLOPE, out=x_hat)
        _hip.unit_float_to_u8(x_hat, out=out)
    t_layer = event_ms(lambda: _hip.convT2d_last_bf16(a16, w, b, g, layer.act, hf.LRELU_SLOPE, out=x_hat), iters)
    t_u8 = event_ms(lambda: _hip.unit_float_to_u8(x_hat, out=out), iters)
    t_two = event_ms(two, iters)
    t_one = event_ms(lambda: _hip.convT2d_last_bf16_u8(a16, w, b, g, layer.act, hf.LRELU_SLOPE, out=out), iters)
    common = a16.numel() * 2 + w.numel() * 4 + out.numel()
    mb_two, mb_one = (common + 2 * x_hat.numel() * 4) / 1e6, common / 1e6
    print('%-14s last layer alone: bn_convT2d_last_bf16 %.1f us + bn_unit_float_to_u8 %.1f us (%.0f GB/s), back to '
          'back %.1f us (%.1f MB, %.0f GB/s); bn_convT2d_last_bf16_u8 %.1f us (%.1f MB, %.0f GB/s); unfused / fused = '
          '%.2f' % (name, t_layer * 1e3, t_u8 * 1e3, x_hat.numel() * 5 / 1e6 / t_u8, t_two * 1e3, mb_two,
                    mb_two / t_two, t_one * 1e3, mb_one, mb_one / t_one, t_two / t_one))
    # the copy to the host that every route ends with: fp32 frames against grey levels
    pin32, pin8 = torch.empty(x_hat.shape).pin_memory(), torch.empty(out.shape, dtype=torch.uint8).pin_memory()
    t32 = event_ms(lambda: pin32.copy_(x_hat, non_blocking=True), iters)
    t8 = event_ms(lambda: pin8.copy_(out, non_blocking=True), iters)
    print('%-14s copy to pinned host memory: fp32 frames %.1f MB in %.1f us, uint8 frames %.1f MB in %.1f us'
          % (name, x_hat.numel() * 4 / 1e6, t32 * 1e3, out.numel() / 1e6, t8 * 1e3))


def export(name, model, n, dim, n_trials):
    root = tempfile.mkdtemp(prefix='bn_recon_')
    try:
        rng = np.random.default_rng(2)
        trials = [rng.integers(0, 256, size=(n,) + tuple(dim), dtype=np.uint8) for _ in range(n_trials)]
        sess_dir = os.path.join(root, 'lab', 'expt', 'animal', 'sess')
        path = write_npz_session(os.path.join(sess_dir, 'data.npz'), {'images': trials})
        ids = [{'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess'}]
        os.makedirs(os.path.join(root, 'version_0'))
        model.hparams['expt_dir'], model.version = root, 0
        for label, keys in (('fp32', {}), ('both keys', {'hip_decode_dtype': 'bf16', 'hip_encode_dtype': 'bf16'})):
            model.hparams.pop('hip_decode_dtype', None), model.hparams.pop('hip_encode_dtype', None)
            model.hparams.update(keys)
            ms = []
            for _ in range(3):
                gen = ConcatSessionsGenerator(root, ids, signals_list=[['images']], transforms_list=[[None]],
                                              paths_list=[[path]], device='cuda', placement='host_u8',
                                              keep_in_memory=False,
                                              trial_splits={'train_tr': 8, 'val_tr': 1, 'test_tr': 1, 'gap_tr': 0})
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                files = ev.export_reconstructions(gen, model)
                ms.append((time.perf_counter() - t0) * 1e3 / n_trials)
            mb = os.path.getsize(files[0]) / 1e6
            print('%-14s export_reconstructions %-9s %d trials, disk to disk: %.3f ms per trial (min %.3f max %.3f over '
                  '3 runs), %.0f frames/s, %.0f MB written' % (name, label, n_trials, statistics.median(ms), min(ms),
                                                               max(ms), n / statistics.median(ms) * 1e3, mb))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--layer-iters', type=int, default=50)
    ap.add_argument('--export-trials', type=int, default=40)
    args = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for name, n, dim in SHAPES:
        model = build(dim)
        g = torch.Generator().manual_seed(1)
        trials = [torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8).to('cuda') for _ in range(8)]
        fns = variants(model)
        res = {}
        for k in VARIANTS:                                   # warm every variant on every trial
            for t in trials:
                res[k] = fns[k](t)
        torch.cuda.synchronize()
        for a, b in (('fp32', 'host'), ('fused', 'unfused'), ('fused', 'fp32')):
            diff = np.abs(res[a].astype(np.int32) - res[b].astype(np.int32))
            print('%-14s %-8s against %-8s %.2f%% of the bytes differ, by %d grey levels at most'
                  % (name, a, b, 100.0 * (diff > 0).mean(), diff.max()))
        ms = {k: [] for k in VARIANTS}
        for _ in range(args.reps):
            for k in VARIANTS:
                ms[k].append(window(fns[k], trials, args.window))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in VARIANTS:
            print('%-14s %-8s %.4f ms per trial (min %.4f max %.4f over %d windows), %.0f frames/s'
                  % (name, k, med[k], min(ms[k]), max(ms[k]), args.reps, n / med[k] * 1e3))
        for k in ('fused', 'unfused'):                       # (the windows the fused-against-unfused rule reads)
            print('%-14s %-8s windows, ms per trial: %s' % (name, k, ' '.join('%.4f' % v for v in ms[k])))
        print('%-14s host / fp32 = %.2f, host / fused = %.2f, unfused / fused = %.3f (fastest unfused window against '
              'slowest fused window: %.3f)' % (name, med['host'] / med['fp32'], med['host'] / med['fused'],
                                               med['unfused'] / med['fused'], min(ms['unfused']) / max(ms['fused'])))
        last_layer(name, model, trials[0], args.layer_iters)
        if args.export_trials:
            export(name, model, n, dim, args.export_trials)


if __name__ == '__main__':
    main()
