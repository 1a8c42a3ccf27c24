"""Up to 64 latents (the grid search's max_latents): the wide generation of the decomposed-KL
kernels (32 < D <= 64, csrc/decomposed_kl.hip) against the float64 oracle, and the three model
classes that use it -- BetaTCVAE, PSVAE, MSPSVAE -- at 48 and 64 latents, single-process,
frame-sharded and through fit_model."""

import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.models import vaes as hip_vaes
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from oracle import ref_cpu
from tests.branches import record_branches, BranchReplay
from tests.cases import case_hparams, case_data, seeded_build, EpsReplay
from tests.golden_utils import base_hparams
from tests.test_gpu_guard_bands import guarded, finite, _bands_stay_untouched  # noqa: F401
from tests.test_gpu_kernels import close
from tests.test_gpu_model import _pair, grads_close_on_same_branches

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(N, D):
    g = torch.Generator().manual_seed(N * 100 + D)
    z = torch.randn((N, D), generator=g)
    mu = torch.randn((N, D), generator=g) * 0.7
    lv = torch.randn((N, D), generator=g) * 0.5 - 0.3
    return z, mu, lv


@pytest.mark.parametrize('N,D', [(200, 33), (200, 48), (200, 64), (56, 64), (1, 64), (7, 40),
                                 (1024, 58), (2048, 64)])
def test_wide_decomposed_kl_vs_float64(N, D):
    """The three terms and dz / dmu / dlogvar under arbitrary upstream weights, against the
    oracle's (N, N, D) formulation in float32 and float64 (as test_decomposed_kl for D <= 32).
    The large cases evaluate the oracle on the device: its (N, N, D) float64 tensors are GBs."""
    from behavenet_amd.hip_functions import decomposed_kl_terms
    z, mu, lv = _inputs(N, D)
    wts = torch.tensor([1.3, -0.4, 2.1])
    odev = DEV if N >= 1024 else 'cpu'
    res = {}
    for key, dt in (('f32', torch.float32), ('f64', torch.float64)):
        zi, mi, li = (t.detach().clone().to(odev, dt).requires_grad_(True) for t in (z, mu, lv))
        terms = torch.stack(ref_cpu.decomposed_kl(zi, mi, li))
        (terms * wts.to(odev, dt)).sum().backward()
        res[key] = tuple(t.detach().cpu() for t in (terms, zi.grad, mi.grad, li.grad))
        del zi, mi, li, terms
    if odev == DEV:
        torch.cuda.empty_cache()
    zh, mh, lh = (t.detach().clone().to(DEV).requires_grad_(True) for t in (z, mu, lv))
    th = decomposed_kl_terms(zh, mh, lh)
    (th * wts.to(DEV)).sum().backward()
    close(th, res['f32'][0], res['f64'][0], name='dkl terms')
    close(zh.grad, res['f32'][1], res['f64'][1], name='dkl dz')
    close(mh.grad, res['f32'][2], res['f64'][2], name='dkl dmu')
    close(lh.grad, res['f32'][3], res['f64'][3], name='dkl dlogvar')


def test_wide_decomposed_kl_repeats_bit_for_bit():
    """Fixed-order reductions, no atomics: two calls on the same inputs, identical bits."""
    z, mu, lv = (t.to(DEV) for t in _inputs(200, 64))
    g3 = torch.tensor([0.7, -1.1, 2.3], device=DEV)
    outs = []
    for _ in range(2):
        out3, log_qz, lse = _hip.decomposed_kl_fwd(z, mu, lv)
        grads = _hip.decomposed_kl_bwd(z, mu, lv, log_qz, lse, g3)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (out3, log_qz, lse) + tuple(grads)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('N,D', [(7, 40), (200, 64), (130, 33)])
def test_wide_decomposed_kl_reads_nothing_outside_its_operands(N, D):
    """Every operand between NaN guard bands: a read past a row, a column half or the last row
    turns the result non-finite; the autouse fixture checks that no band was written."""
    z, mu, lv = (guarded(t) for t in _inputs(N, D))
    out3, log_qz, lse = _hip.decomposed_kl_fwd(z, mu, lv)
    finite(out3, 'wide dkl terms')
    finite(log_qz, 'wide dkl log_qz')
    finite(lse, 'wide dkl lse')
    g3 = guarded(torch.tensor([0.7, -1.1, 2.3]))
    out = (guarded(torch.zeros(N, D)), guarded(torch.zeros(N, D)), guarded(torch.zeros(N, D)))
    dz, dmu, dlv = _hip.decomposed_kl_bwd(z, mu, lv, guarded(log_qz), guarded(lse), g3, out=out)
    for t, nm in ((dz, 'dz'), (dmu, 'dmu'), (dlv, 'dlogvar')):
        finite(t, 'wide dkl ' + nm)


def test_more_than_64_latents_are_refused_before_any_launch(monkeypatch):
    """D = 65: a ValueError naming the limit from the Python glue; the library is never called."""
    def no_library():
        raise AssertionError('the library was reached')
    z, mu, lv = (t.to(DEV).requires_grad_(True) for t in _inputs(20, 65))
    monkeypatch.setattr(_hip, 'load', no_library)
    with pytest.raises(ValueError, match='64'):
        hf.decomposed_kl_terms(z, mu, lv)
    with pytest.raises(ValueError, match='64'):
        _hip.decomposed_kl_bwd(z, mu, lv, torch.zeros(20, device=DEV),
                               torch.zeros(20, 65, device=DEV), torch.ones(3, device=DEV))


# ------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model_class,n_lat', [('beta-tcvae', 48), ('beta-tcvae', 64),
                                               ('ps-vae', 64)])
def test_wide_multichunk_variational_vs_oracle(model_class, n_lat):
    """Two-chunk batches (200 + 10 frames) at 48 / 64 latents, as
    test_gpu_model.py::test_multichunk_variational_vs_oracle: the single-pass schedule against
    the oracle's chunk loop, same eps per chunk, gradients on the device's branch pattern."""
    extra = {'vae.beta': 2.0, 'vae.beta_anneal_epochs': 0, 'max_n_epochs': 10,
             'beta_tcvae.beta': 3.0, 'beta_tcvae.beta_anneal_epochs': 5,
             'ps_vae.alpha': 10, 'ps_vae.beta': 5, 'ps_vae.anneal_epochs': 5,
             'conditional_encoder': False}
    n_labels = 4 if model_class == 'ps-vae' else 0
    meta = {'dim': [1, 32, 32], 'n_lat': n_lat, 'model_class': model_class, 'extra_hp': extra,
            'n_labels': n_labels, 'n_frames': 210}
    hip, ora, hp = _pair(meta)
    data_c = case_data(meta)
    data_g = {k: v.to(DEV) for k, v in data_c.items()}
    g = torch.Generator().manual_seed(9)
    eps = [torch.randn((n, n_lat), generator=g).numpy() for n in (200, 10)]
    ora64 = seeded_build(ref_cpu.build_model, case_hparams(meta)).double()
    data64 = {k: v.double() for k, v in data_c.items()}
    for m in (hip, ora, ora64):
        m.train()
        m.curr_epoch = 3
    ora.eps_fn = EpsReplay(eps)
    ora64.eps_fn = EpsReplay([e.astype(np.float64) for e in eps])
    hip_vaes.set_eps_provider(EpsReplay(eps, DEV))
    try:
        hip.zero_grad()
        ora.zero_grad()
        ora64.zero_grad()
        loss_o = ora.loss(data_c, dataset=0, accumulate_grad=False)
        with record_branches(hip) as rec:
            loss_h = hip.loss(data_g, dataset=0, accumulate_grad=True)
        with BranchReplay(rec) as br:
            ora64.loss(data64, dataset=0, accumulate_grad=True)
    finally:
        hip_vaes.set_eps_provider(None)
    br.assert_only_ties()
    assert sorted(loss_h.keys()) == sorted(loss_o.keys())
    for k in loss_o:
        assert loss_h[k] == pytest.approx(loss_o[k], rel=1e-4, abs=1e-6), k
    grads_close_on_same_branches(hip, ora64, '%s/%d' % (model_class, n_lat))


def test_wide_mspsvae_vs_oracle():
    """A two-session MSPSVAE batch (18 + 15 frames, unchunked) at 64 latents: 2 labels, 4
    background, 58 unsupervised latents.  Loss dict against the oracle, gradients against the
    float64 oracle on the device's branch pattern (1e-4 and the encoding.C.bias rule of
    test_gpu_model.py::test_mspsvae_vs_oracle_and_golden: the triplet term cancels there)."""
    from tests.test_oracle_golden import _msps_case
    _, meta, datas_c = _msps_case()
    meta = dict(meta, n_lat=64, extra_hp=dict(meta['extra_hp'], n_background=4))
    hip, ora, hp = _pair(meta)
    datas_g = [{k: v.to(DEV) for k, v in d.items()} for d in datas_c]
    sess = meta['sess']
    n = sum(meta['n_frames'])
    eps = [torch.randn((n, 64), generator=torch.Generator().manual_seed(4)).numpy()]
    ora64 = seeded_build(ref_cpu.build_model, case_hparams(meta)).double()
    for m in (hip, ora, ora64):
        m.train()
        m.curr_epoch = meta['curr_epoch']
    ora.eps_fn = EpsReplay(eps)
    ora64.eps_fn = EpsReplay([e.astype(np.float64) for e in eps])
    hip_vaes.set_eps_provider(EpsReplay(eps, DEV))
    try:
        hip.zero_grad()
        np.random.seed(11)
        loss_o = ora.loss(datas_c, dataset=sess, accumulate_grad=False)
        np.random.seed(11)
        with record_branches(hip) as rec:
            loss_h = hip.loss(datas_g, dataset=sess, accumulate_grad=True)
        np.random.seed(11)
        with BranchReplay(rec) as br:
            ora64.loss([{k: v.double() for k, v in d.items()} for d in datas_c], dataset=sess,
                       accumulate_grad=True)
    finally:
        hip_vaes.set_eps_provider(None)
    br.assert_only_ties()
    assert sorted(loss_h.keys()) == sorted(loss_o.keys())
    assert loss_h['loss_triplet'] > 0
    for k in loss_o:
        assert loss_h[k] == pytest.approx(loss_o[k], rel=1e-4, abs=1e-6), k
    for (k, ph), (_, p64) in zip(hip.named_parameters(), ora64.named_parameters()):
        if p64.grad is None:
            assert ph.grad is None or not ph.requires_grad, k
            continue
        if k == 'encoding.C.bias':
            tol = 1e-5 * hp['ps_vae.delta']
            assert float((ph.grad.cpu().double() - p64.grad).abs().max()) <= tol, k
            continue
        w = p64.grad.numpy()
        err = np.abs(ph.grad.cpu().double().numpy() - w).max() / max(np.abs(w).max(), 1e-30)
        assert err <= 1e-4, 'mspsvae/64 grad %s: %.3e on the device branches' % (k, err)


def test_betatcvae_fit_and_export_at_48_latents(tmp_path):
    """`fit_model` for 'beta-tcvae' over n_ae_latents [8, 48], two epochs each, with
    export_latents: finite metric rows and latents of the grid point's width in the pickle.
    fit() runs these classes eagerly (no HIP graph of their step), so there is no graphed path
    to compare at 48 latents; that is checked too."""
    from behavenet_amd.fitting.ae_grid_search import fit_model
    from behavenet_amd.fitting.graph_step import GraphedLoss
    dim = [1, 32, 32]
    for version, n_lat in enumerate((8, 48)):
        arch = load_handcrafted_arch(list(dim), n_lat, None, check_memory=False)
        hp = base_hparams(arch, 'beta-tcvae', {'vae.beta': 1.0, 'vae.beta_anneal_epochs': 0,
                                               'beta_tcvae.beta': 4.0,
                                               'beta_tcvae.beta_anneal_epochs': 1})
        hp.update({'expt_dir': str(tmp_path), 'max_n_epochs': 2, 'min_n_epochs': 0,
                   'val_check_interval': 1, 'enable_early_stop': False, 'early_stop_history': 10,
                   'rng_seed_train': 0, 'rng_seed_model': 0, 'export_latents': True,
                   'progress_bar': False, 'device': 'cuda', 'n_parallel_gpus': 1})
        vdir = os.path.join(str(tmp_path), 'version_%d' % version)
        os.makedirs(vdir)
        sess = SyntheticSession(10, 40, dim, seed=version, trial_splits='8;1;1;0',
                                name=('lab', 'expt', 'animal', 'sess-0'))
        gen = SyntheticSessionsGenerator([sess], device=DEV, placement='device_u8')

        class Exp(object):
            rows = []

            def log(self, row):
                self.rows.append(dict(row))

            def save(self):
                pass
        exp = Exp()
        exp.version = version
        model = fit_model(hp, gen, exp)
        assert type(model).__name__ == 'BetaTCVAE' and hp['training_completed']
        assert not GraphedLoss(model).supported({'images': torch.zeros((1, 4, 1, 32, 32),
                                                                       device=DEV)})
        train_rows = [r for r in exp.rows if r.get('dataset') == -1 and 'tr_loss' in r]
        assert len(train_rows) == 3, exp.rows          # epoch 0 (untrained) and the two epochs
        for r in exp.rows:
            for k, v in r.items():
                if isinstance(v, (float, np.floating)):
                    assert np.isfinite(v), (n_lat, k, r)
        with open(os.path.join(vdir, 'lab_expt_animal_sess-0_latents.pkl'), 'rb') as f:
            lat = pickle.load(f)
        assert len(lat['latents']) == 10
        assert all(a.shape == (40, n_lat) and np.all(np.isfinite(a)) for a in lat['latents'])


# ------------------------------------------------------------------------------------------
# frame sharded
# ------------------------------------------------------------------------------------------
def test_frame_sharded_psvae_at_48_latents_matches_the_single_process_step(tmp_path):
    """Two gloo ranks on one GPU (tests/dist_gpu_wide_latents.py), each evaluating the decomposed
    KL of the all-gathered 30-frame chunk with 46 unsupervised latents: loss dict against the
    single-process step, the all-reduced gradient against the float64 oracle on the branch
    pattern assembled from the two ranks (as test_gpu_sharding.py does for 8 latents)."""
    from tests.test_gpu_sharding import _child_env, _free_port, _wait_all, _rank_frames, \
        assemble_branches
    from tests import dist_gpu_wide_latents as case
    tmp = str(tmp_path)
    port = _free_port()
    procs, logs = [], []
    for r in range(2):
        env = _child_env(RANK=str(r), WORLD_SIZE='2', LOCAL_RANK='0', MASTER_PORT=str(port),
                         BN_DP_SHARD='frames')
        logs.append(os.path.join(tmp, 'wide_rank%d.log' % r))
        with open(logs[-1], 'wb') as log:
            procs.append(subprocess.Popen(
                [sys.executable, os.path.join(REPO, 'tests', 'dist_gpu_wide_latents.py'), tmp],
                env=env, stdout=log, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                start_new_session=True))
    _wait_all(procs, logs, 240, 'two ranks, PS-VAE at 48 latents')
    assert os.path.exists(os.path.join(tmp, 'done'))
    with open(os.path.join(tmp, 'loss_rank0.json')) as f:
        got = json.load(f)

    model, data, kw = case.build_case()
    try:
        model.zero_grad(set_to_none=True)
        want = model.loss(data, dataset=0, accumulate_grad=True, **kw)
    finally:
        hip_vaes.set_eps_provider(None)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=5e-5, abs=1e-6), k

    recs = [torch.load(os.path.join(tmp, 'branches_rank%d.pt' % r)) for r in range(2)]
    pattern = assemble_branches(recs, [_rank_frames(case.BATCH, case.CHUNK, r, 2)
                                       for r in range(2)], case.BATCH)
    g = np.load(os.path.join(tmp, 'grad.npy'))
    ora, data_o, kw_o = case.build_oracle(torch.float64)
    with BranchReplay(pattern) as br:
        l64 = ora.loss(data_o, dataset=0, accumulate_grad=True, **kw_o)
    br.assert_only_ties()
    for k, v in l64.items():
        assert got[k] == pytest.approx(v, rel=1e-4, abs=1e-6), ('float64 oracle', k)
    g64 = [(k, p.grad.double().numpy()) for k, p in ora.named_parameters() if p.requires_grad]
    assert sum(w.size for _, w in g64) == g.size
    off = 0
    for k, w in g64:
        mine = g[off:off + w.size].reshape(w.shape)
        off += w.size
        err = np.abs(mine - w).max() / max(np.abs(w).max(), 1e-30)
        assert err <= 2e-5, 'ps-vae/48 sharded grad %s: normalised max err %.3e' % (k, err)
