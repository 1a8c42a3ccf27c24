"""fp32 against bf16 encoding (hparams['hip_encode_dtype']) of device-resident trials, alternated in ONE process.

Per shape: every (shape, dtype) is warmed first, then fp32 and bf16 windows of at least --window seconds alternate
--reps times with a device synchronise around each window.  Prints ms per trial and frames/s for both dtypes
(median, with the spread over the windows), the ratio, and max |z_bf16 - z_f32| / max |z_f32|.  Then
``export_latents`` end to end from a file-backed data.npz session (as tools/probe_export.py), both dtypes, and
the feed alone.   python tools/bench_encode.py [--reps 5] [--window 1.0] [--export-trials 512] [--no-export]

Per-kernel times for the roofline shares come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_encode.py --no-export --reps 1 --window 0.2
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

from behavenet_amd.fitting.eval import encode_trial_device, export_latents
from behavenet_amd.models import AE
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from behavenet_amd.data.synthetic import base_hparams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH2 = os.path.join(REPO, 'behavenet_amd', 'configs', 'ae_jsons', 'ae_arch_2.json')
SHAPES = [('256x1x128x128 u8 (config 5)', 256, [1, 128, 128], None),
          ('189x2x128x128 u8 (Musall)', 189, [2, 128, 128], None),
          ('256x1x64x48 u8', 256, [1, 64, 48], None),
          ('256x1x128x128 u8 ae_arch_2', 256, [1, 128, 128], ARCH2)]


def build(dim, arch_json, extra=None):
    arch = load_handcrafted_arch(list(dim), 12, arch_json, check_memory=False)
    hp = base_hparams(arch, 'ae', dict({'device': 'cuda'}, **(extra or {})))
    torch.manual_seed(0)
    return AE(hp).to('cuda').eval()


def window(model, trials, dtype, seconds):
    model.hparams['hip_encode_dtype'] = dtype
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        for t in trials:
            encode_trial_device(model, t, 0, None, 1024)
        n += len(trials)
        if n % (4 * len(trials)) == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--export-trials', type=int, default=512)
    ap.add_argument('--no-export', action='store_true')
    args = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for name, n, dim, arch_json in SHAPES:
        model = build(dim, arch_json)
        g = torch.Generator().manual_seed(1)
        trials = [torch.randint(0, 256, (n,) + tuple(dim), generator=g, dtype=torch.uint8).to('cuda') for _ in range(8)]
        z = {}
        for dtype in ('f32', 'bf16'):                       # warm every shape in both arithmetics
            model.hparams['hip_encode_dtype'] = dtype
            for t in trials:
                z[dtype] = encode_trial_device(model, t, 0, None, 1024)
        torch.cuda.synchronize()
        err = float((z['bf16'] - z['f32']).abs().max() / z['f32'].abs().max())
        ms = {'f32': [], 'bf16': []}
        for _ in range(args.reps):
            for dtype in ('f32', 'bf16'):
                ms[dtype].append(window(model, trials, dtype, args.window))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in ('f32', 'bf16'):
            print('%-30s %-4s %.4f ms per trial (min %.4f max %.4f over %d windows), %.0f frames/s'
                  % (name, k, med[k], min(ms[k]), max(ms[k]), args.reps, n / med[k] * 1e3))
        print('%-30s f32 / bf16 = %.2f (slowest bf16 window against fastest f32 window: %.2f); '
              'max|z_bf16 - z_f32| / max|z_f32| = %.2e'
              % (name, med['f32'] / med['bf16'], min(ms['f32']) / max(ms['bf16']), err))
    if args.no_export:
        return
    from behavenet_amd.data.data_generator import ConcatSessionsGenerator
    from behavenet_amd.data.trial_store import write_npz_session
    tmp = tempfile.mkdtemp(prefix='bn_encode_')
    try:
        ids = {'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess'}
        sess_dir = os.path.join(tmp, 'lab', 'expt', 'animal', 'sess')
        rng = np.random.default_rng(0)
        block = [rng.integers(0, 256, size=(256, 1, 128, 128), dtype=np.uint8) for _ in range(16)]
        write_npz_session(os.path.join(sess_dir, 'data.npz'),
                          {'images': [block[i % 16] for i in range(args.export_trials)]})

        def gen():
            return ConcatSessionsGenerator(tmp, [ids], signals_list=[['images']], transforms_list=[[None]],
                                           paths_list=[[os.path.join(sess_dir, 'data.npz')]], device='cuda',
                                           placement='host_u8', keep_in_memory=False)
        model = build([1, 128, 128], None, {'expt_dir': tmp})
        model.version = 0
        out = os.path.join(tmp, 'l.pkl')
        for rep in range(2):
            g = gen()
            g.serve_uint8 = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            for split in ('train', 'val', 'test'):
                g.reset_iterators(split)
                for _ in range(g.n_tot_batches[split]):
                    g.next_batch(split)
                    k += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print('feed alone (pass %d): %.3f ms per trial, %.0f frames/s' % (rep, dt / k * 1e3, k * 256 / dt))
        for rep in range(3):
            for dtype in ('f32', 'bf16'):
                model.hparams['hip_encode_dtype'] = dtype
                g = gen()
                n_enc = sum(len(g.datasets[0].batch_idxs[s]) for s in ('train', 'val', 'test'))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                export_latents(g, model, filename=out)
                dt = time.perf_counter() - t0
                print('export_latents from data.npz, %s (pass %d): %.3f ms per trial, %.0f frames/s'
                      % (dtype, rep, dt / n_enc * 1e3, n_enc * 256 / dt))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
