"""One process of tests/test_gpu_resume.py: fits on the MI355X that run unbroken, die mid-epoch, or
resume from the training state a killed run left.

    python tests/gpu_resume_child.py first|resume CASES ROOT

'first': every case unbroken into ROOT/u/<case> and killed (epoch 3, batch 2) into ROOT/k/<case>;
'resume': every case resumed in ROOT/k/<case>.  Each finished fit leaves final.pt (the model's and
the returned best model's state dicts) next to its version directory.  Case 'shardopt' runs on two
gloo ranks (RANK / WORLD_SIZE set by the launcher) with the sharded optimizer step."""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator  # noqa: E402
from behavenet_amd.fitting import distributed as bdist  # noqa: E402
from behavenet_amd.fitting.experiment import Experiment  # noqa: E402
from behavenet_amd.fitting.training import fit  # noqa: E402
from behavenet_amd.models import AE, PSVAE  # noqa: E402
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch  # noqa: E402
from tests.golden_utils import base_hparams  # noqa: E402
from tests.resume_utils import CrashAt, InjectedCrash  # noqa: E402

DEV = 'cuda'
DIM = [1, 32, 32]
CRASH = (3, 2)


def _case(case, root, seed):
    arch = load_handcrafted_arch(list(DIM), 6, None, check_memory=False)
    common = {'expt_dir': os.path.join(root, 'expt'), 'max_n_epochs': 4, 'min_n_epochs': 0,
              'val_check_interval': 1, 'enable_early_stop': True, 'early_stop_history': 10,
              'rng_seed_train': None, 'export_latents': False, 'progress_bar': False,
              'device': DEV, 'learning_rate': 1e-3, 'l2_reg': 1e-4, 'resume_training': True,
              'hip_graph': True}
    n_labels = 2 if case == 'psvae' else 0
    np.random.seed(seed)                # PS-VAE's orthogonal projection comes from numpy's RNG
    torch.manual_seed(seed)             # a resumed run must not depend on the fresh weights
    if case == 'psvae':
        hp = base_hparams(arch, 'ps-vae', dict(common, **{
            'ps_vae.alpha': 10.0, 'ps_vae.beta': 3.0, 'ps_vae.anneal_epochs': 3}))
        hp['n_labels'] = n_labels
        model = PSVAE(hp)
    elif case in ('ae_graph', 'ae_bn', 'shardopt'):
        hp = base_hparams(arch, 'ae', dict(common, ae_batch_norm=case == 'ae_bn'))
        if case == 'shardopt':
            hp.update({'dp_shard': 'frames', 'shard_optimizer': True})
        model = AE(hp)
    else:
        raise ValueError(case)
    model = model.to(DEV)
    model.version = 0
    sess = SyntheticSession(10, 40, DIM, seed=3, n_labels=n_labels, trial_splits='8;1;1;0')
    gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')
    return hp, model, gen


def run(case, root, crash, seed):
    hp, model, gen = _case(case, root, seed)
    exp = Experiment(name='expt', save_dir=root, version=0, debug=bdist.rank() != 0)
    try:
        best = fit(hp, model, CrashAt(gen, *(crash or (None, 0))), exp, method='ae')
    except InjectedCrash:
        print('case %s: crashed as planned' % case, flush=True)
        return
    torch.cuda.synchronize()
    if bdist.rank() == 0:
        torch.save({'model': {k: v.detach().cpu() for k, v in model.state_dict().items()},
                    'best': {k: v.detach().cpu() for k, v in best.state_dict().items()}},
                   os.path.join(root, 'final.pt'))
    else:
        torch.save({'model': {k: v.detach().cpu() for k, v in model.state_dict().items()}},
                   os.path.join(root, 'final_rank%d.pt' % bdist.rank()))
    print('case %s: done' % case, flush=True)


def main():
    phase, cases, root = sys.argv[1], sys.argv[2].split(','), sys.argv[3]
    torch.cuda.set_device(0)
    if os.environ.get('WORLD_SIZE'):
        bdist.init_from_env(backend='gloo')
    for case in cases:
        if phase == 'first':
            run(case, os.path.join(root, 'u', case), None, seed=0)
            run(case, os.path.join(root, 'k', case), CRASH, seed=0)
        else:
            run(case, os.path.join(root, 'k', case), None, seed=1)
    if bdist.is_active():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
