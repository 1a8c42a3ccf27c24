"""Resumable fits on the MI355X: a fit killed in the middle of an epoch and resumed in a FRESH
process from its training state ends bit for bit where the unbroken fit ends -- final parameters,
best_val_model.pt, the returned best model and the metric rows (tests/gpu_resume_child.py runs the
fits).  Cases: the conv AE with the graphed step, the AE with batch norm (running statistics), the
PS-VAE (eps draws, annealing, numpy's orthogonal projection) and the AE on two gloo ranks with the
sharded optimizer step.  Also: FlatAdamAMSGrad's state through torch.optim.Adam and back, and a grid
point that is killed and rerun."""

import json
import os
import pickle
import subprocess
import sys

import pytest
import torch

from behavenet_amd.fitting.optim import FlatAdamAMSGrad
from behavenet_amd.fitting.training import TRAINING_STATE_FILE
from tests.resume_utils import CrashAt, InjectedCrash, read_rows
from tests.test_gpu_sharding import _child_env, _free_port, _wait_all

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, 'tests', 'gpu_resume_child.py')
ONE_RANK_CASES = ['ae_graph', 'ae_bn', 'psvae']


def _launch(root, phase, cases, ranks=1, limit_s=240):
    """The child script on ``ranks`` processes (two at most, and this one: within six GPU processes),
    under a time limit; a failure or stall fails the test with the logs' tails."""
    port = _free_port()
    procs, logs = [], []
    for r in range(ranks):
        extra = dict(RANK=str(r), WORLD_SIZE=str(ranks), LOCAL_RANK='0', MASTER_PORT=str(port)) \
            if ranks > 1 else {}
        logs.append(os.path.join(root, '%s_%s_rank%d.log' % (phase, cases[0], r)))
        with open(logs[-1], 'wb') as log:
            procs.append(subprocess.Popen(
                [sys.executable, CHILD, phase, ','.join(cases), root], env=_child_env(**extra),
                stdout=log, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                start_new_session=True))
    _wait_all(procs, logs, limit_s, '%s of %s' % (phase, ','.join(cases)))


@pytest.fixture(scope='module')
def fits(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('resume'))
    _launch(root, 'first', ONE_RANK_CASES)
    _launch(root, 'first', ['shardopt'], ranks=2)
    for case in ONE_RANK_CASES + ['shardopt']:
        vdir = os.path.join(root, 'k', case, 'expt', 'version_0')
        assert os.path.exists(os.path.join(vdir, TRAINING_STATE_FILE)), case
        assert not os.path.exists(os.path.join(root, 'k', case, 'final.pt')), case
    _launch(root, 'resume', ONE_RANK_CASES)
    _launch(root, 'resume', ['shardopt'], ranks=2)
    return root


def _assert_equal_dicts(a, b, what):
    assert list(a.keys()) == list(b.keys()), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize('case', ONE_RANK_CASES + ['shardopt'])
def test_resumed_fit_in_a_fresh_process_equals_the_unbroken_fit(fits, case):
    u, k = os.path.join(fits, 'u', case), os.path.join(fits, 'k', case)
    got_u = torch.load(os.path.join(u, 'final.pt'))
    got_k = torch.load(os.path.join(k, 'final.pt'))
    _assert_equal_dicts(got_u['model'], got_k['model'], 'final parameters')
    _assert_equal_dicts(got_u['best'], got_k['best'], 'returned best model')
    vu, vk = os.path.join(u, 'expt', 'version_0'), os.path.join(k, 'expt', 'version_0')
    _assert_equal_dicts(torch.load(os.path.join(vu, 'best_val_model.pt')),
                        torch.load(os.path.join(vk, 'best_val_model.pt')), 'best_val_model.pt')
    rows = read_rows(vu)
    assert len(rows) == 5 * 2 + 1 and rows == read_rows(vk)
    assert not os.path.exists(os.path.join(vk, TRAINING_STATE_FILE))
    if case == 'ae_bn':
        assert any('running_mean' in name for name in got_k['model'])
    if case == 'shardopt':
        # the other rank ends with the same parameters
        _assert_equal_dicts(got_k['model'], torch.load(os.path.join(k, 'final_rank1.pt'))['model'],
                            'rank 1')
        _assert_equal_dicts(got_u['model'], torch.load(os.path.join(u, 'final_rank1.pt'))['model'],
                            'rank 1, unbroken')


def test_flat_adam_state_through_torch_adam_and_back():
    """Steps on the device, the state to torch.optim.Adam on the CPU and back into a fresh arena: the
    moments and the step count survive, and the next step of both arenas is the same."""
    torch.manual_seed(0)
    shapes = [(16, 1, 5, 5), (16,), (33, 7), (1,)]
    params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    opt = FlatAdamAMSGrad(params, lr=1e-3, weight_decay=1e-4)
    grads = [[torch.randn(s, device=DEV) for s in shapes] for _ in range(4)]

    def step(o, g):
        o.zero_grad()               # (the arena padding keeps zero gradients, as in training)
        for p, gp in zip(o.params, g):
            p.grad.copy_(gp)
        o.step()
    for g in grads[:3]:
        step(opt, g)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    adam = torch.optim.Adam(cpu, lr=0.5, amsgrad=True)
    adam.load_state_dict(opt.state_dict())
    assert adam.param_groups[0]['lr'] == 1e-3
    for i in range(len(shapes)):
        for name, x in zip(('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'), opt.state_tensors(i)):
            assert torch.equal(adam.state[cpu[i]][name], x.cpu()), (i, name)
        assert float(adam.state[cpu[i]]['step']) == 3

    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    back = FlatAdamAMSGrad(twins, lr=0.5)
    back.load_state_dict(adam.state_dict())
    assert back.step_count == 3 and back.lr == 1e-3 and back.weight_decay == 1e-4
    for arena in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
        assert torch.equal(getattr(opt, arena), getattr(back, arena)), arena
    for o in (opt, back):
        step(o, grads[3])
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_p, back.flat_p)


def test_killed_grid_point_is_resumed_in_its_version(tmp_path, monkeypatch):
    from behavenet_amd.data import utils as data_utils
    from behavenet_amd.fitting import hyperparam_utils
    from behavenet_amd.fitting.ae_grid_search import run_grid
    from tests.test_fit_host import _write_sessions
    from tests.test_gpu_grid_search import _configs

    data_dir = os.path.join(str(tmp_path), 'data')
    _write_sessions(data_dir, n_sessions=1, n_trials=10, dim=(1, 32, 32), n_labels=0)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    real = data_utils.build_data_generator
    try:
        versions = {}
        for tag in ('unbroken', 'killed'):
            save_dir = os.path.join(str(tmp_path), tag)
            args = _configs(tmp_path, data_dir, save_dir, n_ae_latents=4)
            with open(args[args.index('--training_config') + 1]) as f:
                training = json.load(f)
            training.update({'max_n_epochs': 4, 'export_latents': False, 'resume_training': True})
            with open(args[args.index('--training_config') + 1], 'w') as f:
                json.dump(training, f)
            if tag == 'killed':
                monkeypatch.setattr(data_utils, 'build_data_generator',
                                    lambda *a, **kw: CrashAt(real(*a, **kw), 3, 4))
                with pytest.raises(InjectedCrash):
                    run_grid(hyperparam_utils.get_all_params('grid_search', args=args))
                monkeypatch.setattr(data_utils, 'build_data_generator', real)
                expt_dir = os.path.join(save_dir, 'lab', 'expt', 'animal', 'sess-0', 'ae', 'conv',
                                        '04_latents', 'grid-test')
                vdir = os.path.join(expt_dir, 'version_0')
                with open(os.path.join(vdir, 'meta_tags.pkl'), 'rb') as f:
                    assert pickle.load(f)['training_completed'] is False
                assert os.path.exists(os.path.join(vdir, TRAINING_STATE_FILE))
            (hp, model), = run_grid(hyperparam_utils.get_all_params('grid_search', args=args))
            assert model is not None and hp['version'] == 0 and hp['training_completed'] is True
            versions[tag] = os.path.join(hp['expt_dir'], 'version_0')
            assert sorted(os.listdir(hp['expt_dir'])) == ['version_0']
            assert not os.path.exists(os.path.join(versions[tag], TRAINING_STATE_FILE))
            with open(os.path.join(versions[tag], 'meta_tags.pkl'), 'rb') as f:
                assert pickle.load(f)['training_completed'] is True
            # a completed point is skipped
            again = run_grid(hyperparam_utils.get_all_params('grid_search', args=args))
            assert [m for _, m in again] == [None]
        rows = read_rows(versions['unbroken'])
        assert len(rows) == 5 * 2 + 1 and rows == read_rows(versions['killed'])
        _assert_equal_dicts(torch.load(os.path.join(versions['unbroken'], 'best_val_model.pt')),
                            torch.load(os.path.join(versions['killed'], 'best_val_model.pt')),
                            'best_val_model.pt')
    finally:
        os.environ.pop('BEHAVENET_DATA_DIR', None)
        os.environ.pop('BEHAVENET_SAVE_DIR', None)
