"""What writing the training state of a resumable fit costs fit() on configs[1]: the fit of bench.py's
fit() secondary (epoch 0 + N epochs over 16 train / 2 val / 2 test resident trials of 256 frames),
timed with hparams['resume_training'] off and on (the state written after every epoch).

    python tools/bench_resume.py [epochs]

Prints one JSON line: seconds per fit (the faster of two timed runs after a warm-up), per epoch, and
the size of the state file."""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator  # noqa: E402
from behavenet_amd.fitting import training  # noqa: E402
from behavenet_amd.fitting.experiment import Experiment  # noqa: E402
from behavenet_amd.models import AE  # noqa: E402


def run(hp, keep_state_size):
    root = tempfile.mkdtemp()
    try:
        hp = dict(hp, expt_dir=os.path.join(root, 'expt'))
        torch.manual_seed(0)
        model = AE(dict(hp)).to('cuda')
        model.version = 0
        sess = SyntheticSession(20, bench.BATCH, bench.DIM, seed=100, trial_splits='8;1;1;0')
        gen = SyntheticSessionsGenerator([sess], device='cuda', placement='device')
        exp = Experiment(name='expt', save_dir=root, version=0)
        size = []
        if keep_state_size:
            # the state file is removed when the fit completes: note its size on the way
            real = training._atomic_save

            def spy(obj, path, durable=False):
                real(obj, path, durable=durable)
                if path.endswith(training.TRAINING_STATE_FILE):
                    size.append(os.path.getsize(path))
            training._atomic_save = spy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            training.fit(hp, model, gen, exp, method='ae')
        finally:
            if keep_state_size:
                training._atomic_save = real
        torch.cuda.synchronize()
        return time.perf_counter() - t0, size
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    n_epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    hp = bench.build_hparams()
    hp.update({'max_n_epochs': n_epochs, 'min_n_epochs': n_epochs, 'enable_early_stop': False,
               'val_check_interval': 1, 'version': 0, 'device': 'cuda', 'rng_seed_train': 0,
               'export_latents': False, 'early_stop_history': 10, 'progress_bar': False})
    out = {'epochs': n_epochs + 1}
    stdout = sys.stdout
    sys.stdout = sys.stderr
    try:
        for name, extra in (('off', {}), ('every_epoch', {'resume_training': True,
                                                          'training_state_interval': 1})):
            h = dict(hp, **extra)
            run(h, False)                   # (allocator pools, pinned buffers, kernel attributes)
            times, sizes = [], []
            for _ in range(2):
                dt, size = run(h, bool(extra))
                times.append(dt)
                sizes += size
            out[name] = {'seconds': min(times), 'ms_per_epoch': 1e3 * min(times) / (n_epochs + 1)}
            if sizes:
                out[name]['state_mb'] = max(sizes) / 1e6
    finally:
        sys.stdout = stdout
    out['cost_ms_per_epoch'] = out['every_epoch']['ms_per_epoch'] - out['off']['ms_per_epoch']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
