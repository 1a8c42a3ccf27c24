"""One rank of a 2-process frame-sharded PS-VAE step at 48 latents on ONE GPU (gloo rendezvous):
launched twice by tests/test_gpu_wide_latents.py with RANK=0/1.  Every rank evaluates the
decomposed KL of the all-gathered chunk with 46 unsupervised latents, i.e. on the wide kernel
generation.  Also imported by that test for the single-process step and the oracle of the case."""

import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from behavenet_amd.fitting import distributed as bdist  # noqa: E402
from behavenet_amd.fitting.optim import FlatAdamAMSGrad  # noqa: E402
from behavenet_amd.models import PSVAE  # noqa: E402
from behavenet_amd.models import vaes as hip_vaes  # noqa: E402
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch  # noqa: E402
from tests.dist_gpu_two_ranks import _Eps, flat_grad  # noqa: E402
from tests.golden_utils import base_hparams, make_frames, make_labels  # noqa: E402

DEV = 'cuda'
DIM = [1, 32, 32]
N_LAT, N_LABELS, BATCH, CHUNK = 48, 2, 44, 30


def _hparams():
    arch = load_handcrafted_arch(list(DIM), N_LAT, None, check_memory=False)
    hp = base_hparams(arch, 'ps-vae', {'ps_vae.alpha': 10.0, 'ps_vae.beta': 3.0,
                                       'ps_vae.anneal_epochs': 0, 'max_n_epochs': 10})
    hp['n_labels'] = N_LABELS
    return hp


def build_case():
    """-> (PS-VAE on the GPU, data dict, loss kwargs): batch 44 in chunks of 30 + 14."""
    data = {'images': torch.from_numpy(make_frames(BATCH, DIM, seed=8)).to(DEV)[None],
            'labels': torch.from_numpy(make_labels(BATCH, N_LABELS, seed=2)).to(DEV)[None]}
    torch.manual_seed(0)
    np.random.seed(0)
    model = PSVAE(_hparams()).to(DEV)
    model.train()
    hip_vaes.set_eps_provider(_Eps())
    return model, data, {'chunk_size': CHUNK}


def build_oracle(dtype=torch.float64):
    """The CPU oracle of the same case (same seeds => same parameters, same eps per chunk)."""
    from oracle import ref_cpu
    data = {'images': torch.from_numpy(make_frames(BATCH, DIM, seed=8)).to(dtype)[None],
            'labels': torch.from_numpy(make_labels(BATCH, N_LABELS, seed=2)).to(dtype)[None]}
    torch.manual_seed(0)
    np.random.seed(0)
    model = ref_cpu.PSVAE(_hparams()).to(dtype)
    model.eps_fn = _Eps()
    model.train()
    return model, data, {'chunk_size': CHUNK}


def main():
    """argv: output directory."""
    from tests.branches import record_branches
    tmp = sys.argv[1]
    torch.cuda.set_device(0)
    rank, world = bdist.init_from_env(backend='gloo')
    assert world == 2 and bdist.shard_mode() == 'frames' and bdist.frames_sharded()
    model, data, kw = build_case()
    opt = FlatAdamAMSGrad(model.get_parameters(), lr=1e-4)
    opt.zero_grad()
    try:
        with record_branches(model) as rec:
            loss = model.loss(data, dataset=0, accumulate_grad=True, **kw)
    finally:
        hip_vaes.set_eps_provider(None)
    bdist.reduce_gradients(opt)
    g = flat_grad(model).cpu().double().numpy()
    torch.save(rec, os.path.join(tmp, 'branches_rank%d.pt' % rank))
    if rank == 0:
        np.save(os.path.join(tmp, 'grad.npy'), g)
        with open(os.path.join(tmp, 'loss_rank0.json'), 'w') as f:
            json.dump(loss, f)
    torch.distributed.barrier()
    if rank == 0:
        open(os.path.join(tmp, 'done'), 'w').close()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
