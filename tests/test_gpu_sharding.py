"""Frame-sharded data parallelism (BASELINE configs[2]) on the HIP models.

* one GPU, ranks emulated one after another (``bdist.emulate_rank``): the sum over ranks of the
  per-rank loss contributions and gradients equals the unsharded HIP step and the CPU oracle
  (reference aes.py:751-771: one mean per 200-frame chunk, gradients accumulated over chunks);
* two real processes on the one GPU with a gloo rendezvous (collectives staged through the
  host): the batch-coupled terms that emulation cannot provide -- batch-norm statistics over all
  ranks' frames (aes.py:90-97,332-336) and the decomposed KL on the all-gathered chunk
  (losses.py:321-341) -- and ``fit`` in 'frames' mode against the single-process run."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.models import AE, VAE
from behavenet_amd.models import vaes as hip_vaes
from behavenet_amd.models.ae_model_architecture_generator import load_handcrafted_arch
from oracle import ref_cpu
from tests.branches import record_branches, BranchReplay
from tests.golden_utils import base_hparams, make_frames
from tests.test_gpu_kernels import close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grads(model):
    return [p.grad.detach().clone() for p in model.parameters() if p.requires_grad]


def _rank_frames(batch, chunk, r, R):
    """Global frame indices rank r of R processes, in its processing order (its slice of chunk
    0, then of chunk 1, ...: `shard_chunks`)."""
    with bdist.emulate_rank(r, R):
        _, local, _ = bdist.shard_chunks(batch, chunk)
    return [i for b, e in local for i in range(b, e)]


def assemble_branches(per_rank, frames_of_rank, batch):
    """One whole-batch LeakyReLU branch pattern (tests/branches.py) from the patterns the ranks
    recorded on their own frames: {stack: [bool (batch, C, H, W) | None per layer]}."""
    out = {}
    for stack in per_rank[0]:
        layers = []
        for li, first in enumerate(per_rank[0][stack]):
            if first is None:
                layers.append(None)
                continue
            full = torch.zeros((batch,) + tuple(first.shape[1:]), dtype=torch.bool)
            seen = torch.zeros(batch, dtype=torch.bool)
            for rec, frames in zip(per_rank, frames_of_rank):
                assert rec[stack][li].shape[0] == len(frames)
                if frames:
                    full[frames] = rec[stack][li]
                    seen[frames] = True
            assert bool(seen.all()), 'shards do not cover the batch'
            layers.append(full)
        out[stack] = layers
    return out


def _sum_over_emulated_ranks(model, data, R, chunk_size, **loss_kw):
    """-> (summed loss dict, summed gradients, whole-batch branch pattern of the R passes)."""
    total, loss, recs = None, {}, []
    batch = data['images'].shape[1]
    for r in range(R):
        model.zero_grad(set_to_none=True)
        with bdist.emulate_rank(r, R), record_branches(model) as rec:
            out = model.loss(data, dataset=0, accumulate_grad=True, chunk_size=chunk_size, **loss_kw)
        recs.append(rec)
        g = _grads(model)
        total = g if total is None else [a + b for a, b in zip(total, g)]
        for k, v in out.items():
            loss[k] = loss.get(k, 0.0) + v
    pattern = assemble_branches(recs, [_rank_frames(batch, chunk_size, r, R) for r in range(R)],
                                batch)
    return loss, total, pattern


def _grads_match_oracle_on_branches(g_sum, ora64, name, tol=2e-5):
    """The 2e-5 gate of tests/test_gpu_model.py::grads_close_on_same_branches for a gradient list."""
    for g, (k, po) in zip(g_sum, [(k, p) for k, p in ora64.named_parameters() if p.requires_grad]):
        w = po.grad.numpy()
        err = np.abs(g.cpu().double().numpy() - w).max() / max(np.abs(w).max(), 1e-30)
        assert err <= tol, '%s grad %s: normalised max err %.3e' % (name, k, err)


@pytest.mark.parametrize('dim,n_lat,batch,chunk,R', [
    ([1, 32, 32], 8, 210, 200, 2), ([1, 32, 32], 8, 210, 200, 8),
    ([1, 128, 128], 12, 256, 200, 2), ([1, 128, 128], 12, 256, 200, 8)])
def test_ae_frame_shards_add_up_to_the_single_device_step(dim, n_lat, batch, chunk, R):
    """Sum over ranks of the frame-sharded losses and gradients == the reference's step
    (aes.py:751-771).  Every rank's pass picks its own tilings, so each may put a LeakyReLU
    pre-activation that lies within rounding of zero on either branch; the float64 oracle is
    therefore run ONCE over the whole batch on the branch pattern assembled from the ranks'
    passes, the pattern is checked to differ from the oracle's own only at ties, and the summed
    gradients are then held to the same 2e-5 as every unsharded model test."""
    arch = load_handcrafted_arch(list(dim), n_lat, None, check_memory=False)
    torch.manual_seed(0)
    model = AE(base_hparams(arch, 'ae')).to(DEV)
    x = torch.from_numpy(make_frames(batch, dim, seed=5))
    data = {'images': x.to(DEV)[None]}
    model.zero_grad(set_to_none=True)
    whole = model.loss(data, dataset=0, accumulate_grad=True, chunk_size=chunk)
    shard_loss, g_sum, pattern = _sum_over_emulated_ranks(model, data, R, chunk)
    assert shard_loss['loss'] == pytest.approx(whole['loss'], rel=1e-6)
    torch.manual_seed(0)
    ora64 = ref_cpu.AE(base_hparams(dict(arch), 'ae')).double()
    with BranchReplay(pattern) as br:
        l64 = ora64.loss({'images': x.double()[None]}, dataset=0, accumulate_grad=True,
                         chunk_size=chunk)
    br.assert_only_ties()
    assert shard_loss['loss'] == pytest.approx(l64['loss'], rel=1e-5)
    _grads_match_oracle_on_branches(g_sum, ora64, 'AE shards R=%d' % R)


def test_vae_frame_shards_use_the_single_device_eps():
    dim, batch, chunk, R = [1, 32, 32], 210, 200, 4
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    extra = {'vae.beta': 2.0, 'vae.beta_anneal_epochs': 0, 'max_n_epochs': 10}
    torch.manual_seed(0)
    model = VAE(base_hparams(arch, 'vae', extra)).to(DEV)
    x = torch.from_numpy(make_frames(batch, dim, seed=6))
    data = {'images': x.to(DEV)[None]}
    g = torch.Generator().manual_seed(1)
    eps_chunks = [torch.randn((200, 8), generator=g), torch.randn((10, 8), generator=g)]

    class Replay(object):
        def __init__(self):
            self.i = 0

        def __call__(self, like):
            t = eps_chunks[self.i % 2].to(device=like.device, dtype=like.dtype)
            self.i += 1
            assert t.shape == like.shape
            return t
    try:
        hip_vaes.set_eps_provider(Replay())
        model.zero_grad(set_to_none=True)
        whole = model.loss(data, dataset=0, accumulate_grad=True, chunk_size=chunk)
        hip_vaes.set_eps_provider(Replay())
        shard_loss, g_sum, pattern = _sum_over_emulated_ranks(model, data, R, chunk)
    finally:
        hip_vaes.set_eps_provider(None)
    # (loss_mse is an affine function of loss_ll evaluated AFTER the sum over ranks: not additive)
    for k in ('loss', 'loss_ll', 'loss_kl'):
        assert shard_loss[k] == pytest.approx(whole[k], rel=2e-5, abs=1e-6), k
    torch.manual_seed(0)
    ora64 = ref_cpu.VAE(base_hparams(dict(arch), 'vae', extra)).double()
    ora64.train()
    ora64.eps_fn = Replay()
    with BranchReplay(pattern) as br:
        l64 = ora64.loss({'images': x.double()[None]}, dataset=0, accumulate_grad=True,
                         chunk_size=chunk)
    br.assert_only_ties()
    for k in ('loss', 'loss_ll', 'loss_kl'):
        assert shard_loss[k] == pytest.approx(l64[k], rel=2e-5, abs=1e-6), k
    _grads_match_oracle_on_branches(g_sum, ora64, 'VAE shards R=%d' % R)


def test_batch_coupled_terms_refuse_emulation():
    """Batch-norm statistics and the decomposed KL need the other ranks' data inside the step."""
    dim = [1, 32, 32]
    arch = load_handcrafted_arch(list(dim), 8, None, check_memory=False)
    torch.manual_seed(0)
    model = AE(base_hparams(arch, 'ae', {'ae_batch_norm': True})).to(DEV)
    data = {'images': torch.from_numpy(make_frames(12, dim, seed=1)).to(DEV)[None]}
    with bdist.emulate_rank(0, 2):
        with pytest.raises(RuntimeError):
            model.loss(data, dataset=0, accumulate_grad=True)


def _free_port():
    """A TCP port nobody listens on (bound to 0 and released): two runs never share a rendezvous."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _child_env(**extra):
    """Environment of a child rank: loopback rendezvous on the loopback INTERFACE (gloo otherwise
    picks its interface from the host name, which need not resolve on a fresh box), a fresh port,
    a 60 s ceiling on the rendezvous and every collective, no rank variables inherited."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(MASTER_ADDR='127.0.0.1', GLOO_SOCKET_IFNAME='lo', NCCL_SOCKET_IFNAME='lo',
               BN_DIST_TIMEOUT_S='60', PYTHONFAULTHANDLER='1')
    env['PYTHONPATH'] = REPO + (os.pathsep + env['PYTHONPATH'] if env.get('PYTHONPATH') else '')
    # two ranks + this process share the container's CPU quota (behavenet_amd/hostinfo.py)
    from behavenet_amd.hostinfo import usable_cpus
    env['OMP_NUM_THREADS'] = env['MKL_NUM_THREADS'] = str(max(1, usable_cpus() // 4))
    env.update(extra)
    return env


def _wait_all(procs, logs, limit_s, what):
    """Wait for the child processes (their output goes to FILES: no pipe can fill up and block a
    rank inside a collective); when the limit expires or one fails, kill every one of them --
    whole process groups -- and fail with the tail of every log, so that a stall names its cause
    instead of eating the suite's time limit."""
    import signal
    import time
    t_end = time.time() + limit_s
    failed = None
    try:
        while True:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes):
                failed = 'exit codes %s' % codes
                break
            if all(c == 0 for c in codes):
                return
            if time.time() > t_end:
                failed = 'no exit after %d s (codes %s)' % (limit_s, codes)
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except OSError:
                    p.kill()
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                pass
    tails = []
    for path in logs:
        with open(path, errors='replace') as f:
            tails.append('---- %s ----\n%s' % (os.path.basename(path), f.read()[-3000:]))
    pytest.fail('%s: %s\n%s' % (what, failed, '\n'.join(tails)), pytrace=False)


TWO_RANK_CASES = ['ae_bn', 'psvae', 'betatc', 'vae_bn', 'psvae_bn', 'aemsp', 'refuse', 'shardopt', 'fit']


def _run_two_ranks(tmp, cases, limit_s=240):
    port = _free_port()
    procs, logs = [], []
    for r in range(2):
        env = _child_env(RANK=str(r), WORLD_SIZE='2', LOCAL_RANK='0', MASTER_PORT=str(port),
                         BN_DP_SHARD='frames')
        logs.append(os.path.join(tmp, 'two_ranks_rank%d.log' % r))
        with open(logs[-1], 'wb') as log:
            procs.append(subprocess.Popen(
                [sys.executable, os.path.join(REPO, 'tests', 'dist_gpu_two_ranks.py'),
                 ','.join(cases), tmp], env=env, stdout=log, stderr=subprocess.STDOUT,
                stdin=subprocess.DEVNULL, start_new_session=True))
    _wait_all(procs, logs, limit_s, 'two ranks, cases %s' % ','.join(cases))


@pytest.fixture(scope='module')
def two_rank_dir(tmp_path_factory):
    """ONE pair of rank processes (one rendezvous, one HIP context each) runs all two-rank cases
    and leaves their results here; round 3 started a pair per case (25 s for the first)."""
    tmp = str(tmp_path_factory.mktemp('two_ranks'))
    _run_two_ranks(tmp, TWO_RANK_CASES)
    return tmp


def _two_rank_result(tmp, case):
    assert os.path.exists(os.path.join(tmp, case + '.done')), 'case %s did not complete' % case
    with open(os.path.join(tmp, case + '_rank0.json')) as f:
        return json.load(f)


def test_sharded_optimizer_step_on_two_ranks_equals_the_replicated_step(two_rank_dir):
    """`bdist.sharded_step` with the device kernel (`FlatAdamAMSGrad.step_range` on this rank's half
    of the arena) against all-reduce + the full step, three steps of a frame-sharded AE with batch
    norm: bit-identical parameters on both ranks."""
    assert os.path.exists(os.path.join(two_rank_dir, 'shardopt.done'))
    for r in range(2):
        with open(os.path.join(two_rank_dir, 'shardopt_rank%d.json' % r)) as f:
            got = json.load(f)
        assert got['params_finite'] and got['steps'] == 3, got
        assert got['max_abs_diff'] == 0.0, (r, got)


def test_frame_sharding_is_refused_on_every_rank_for_the_session_coupled_models(two_rank_dir):
    """`MSPSVAE` and the batch-norm variant of `AEMSP` are not served by frame sharding (the triplet
    term couples sessions, reference vaes.py:1040-1048; `AEMSP` itself is since round 4, case
    'aemsp' of the two-rank test): BOTH ranks must raise
    NotImplementedError from `loss()` -- and reach the barrier behind the case, which they only do
    if neither went on into a collective alone."""
    assert os.path.exists(os.path.join(two_rank_dir, 'refuse.done')), 'the ranks did not finish the case'
    for r in range(2):
        with open(os.path.join(two_rank_dir, 'refuse_rank%d.json' % r)) as f:
            got = json.load(f)
        for cls in ('AEMSP', 'MSPSVAE'):
            assert got[cls] is not None and 'frame' in got[cls].lower(), (r, cls, got[cls])


@pytest.mark.parametrize('case', TWO_RANK_CASES[:-3])
def test_two_ranks_on_one_gpu_match_the_single_process_step(two_rank_dir, case):
    """Real collectives (gloo, host-staged) between two processes sharing the GPU: the terms
    emulation cannot provide (SyncBN statistics, the decomposed KL on the all-gathered chunk).
    Loss dict and running statistics against the single-process HIP step; the all-reduced
    gradient -- ALL of it -- against the float64 oracle run on the LeakyReLU branch pattern
    assembled from the two ranks' passes, at the 2e-5 of the unsharded tests."""
    tmp_path = two_rank_dir
    got = _two_rank_result(tmp_path, case)
    from tests.dist_gpu_two_ranks import build_case, build_oracle
    model, data, kw = build_case(case)
    model.zero_grad(set_to_none=True)
    want = model.loss(data, dataset=0, accumulate_grad=True, **kw)
    hip_vaes.set_eps_provider(None)
    for k, v in want.items():
        assert got['loss'][k] == pytest.approx(v, rel=5e-5, abs=1e-6), k
    for k, v in got.get('buffers', {}).items():          # batch-norm running statistics
        b = dict(model.named_buffers())[k].float().cpu().numpy()
        np.testing.assert_allclose(np.asarray(v), b.reshape(-1)[:len(v)], rtol=1e-4, atol=1e-6)

    recs = [torch.load(os.path.join(str(tmp_path), '%s_branches_rank%d.pt' % (case, r)))
            for r in range(2)]
    pattern = assemble_branches(recs, [_rank_frames(44, 30, r, 2) for r in range(2)], 44)
    g = np.load(os.path.join(str(tmp_path), case + '_grad.npy'))

    def oracle_grads(dtype):
        ora, data_o, kw_o = build_oracle(case, dtype)
        with BranchReplay(pattern) as br:
            loss = ora.loss(data_o, dataset=0, accumulate_grad=True, **kw_o)
        # (AEMSP's U matrix takes no part in the loss: no gradient in the oracle, a zero one in the
        # model's flat gradient arena)
        named = [(k, (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy())
                 for k, p in ora.named_parameters() if p.requires_grad]
        return loss, named, br
    l64, g64, br = oracle_grads(torch.float64)
    br.assert_only_ties()
    for k, v in l64.items():
        assert got['loss'][k] == pytest.approx(v, rel=1e-4, abs=1e-6), ('float64 oracle', k)
    assert sum(w.size for _, w in g64) == g.size
    g32 = oracle_grads(torch.float32)[1] if case.endswith('_bn') else None
    names = {k for k, _ in g64}
    off = 0
    for i, (k, w) in enumerate(g64):
        mine = g[off:off + w.size].reshape(w.shape)
        off += w.size
        scale = max(np.abs(w).max(), 1e-30)
        err = np.abs(mine - w).max() / scale
        tol = 2e-5
        if g32 is not None:
            from tests.test_gpu_model import _bias_before_batchnorm
            if _bias_before_batchnorm(k, names):
                continue        # analytically zero: both sides compute rounding noise
            # batch norm over 30 / 14 values per channel at the deepest layers: the fp32
            # reference is itself off the float64 answer by more than 2e-5 (DESIGN.md section 2,
            # `cond`) -- the bar is then the reference's own distance, on the same branches
            tol = max(tol, 2 * np.abs(g32[i][1] - w).max() / scale)
        assert err <= tol, '%s grad %s: normalised max err %.3e (tol %.1e)' % (case, k, err, tol)


def test_fit_in_frames_mode_matches_single_process(two_rank_dir, tmp_path):
    got = _two_rank_result(two_rank_dir, 'fit')
    from tests.dist_gpu_two_ranks import run_fit
    want = run_fit(os.path.join(str(tmp_path), 'single'))
    assert len(got['rows']) == len(want['rows'])
    for a, b in zip(got['rows'], want['rows']):
        assert a.keys() == b.keys()
        for k, v in b.items():
            if isinstance(v, float):
                assert a[k] == pytest.approx(v, rel=1e-4), k
            else:
                assert a[k] == v, k
    # 16 Adam steps.  Adam normalises every gradient element by its own magnitude, so where the
    # gradient is rounding noise (or a LeakyReLU tie fell the other way on the 16-frame shards)
    # a weight moves by up to lr per step in either run: bound every element by the full travel
    # and all but a few by 2 % of it
    travel = 16 * 1e-4
    diff = np.abs(np.asarray(got['param_sample']) - np.asarray(want['param_sample']))
    assert diff.max() <= travel
    assert np.mean(diff > 0.02 * travel + 1e-3 * np.abs(want['param_sample'])) <= 0.02


def _bench_line(cmd, env, tmp_path, limit_s=240):
    log = os.path.join(str(tmp_path), 'bench_%d.log' % len(os.listdir(str(tmp_path))))
    env = dict(env, BN_BENCH_DETAIL=log + '.detail.json')
    with open(log, 'wb') as f:
        proc = subprocess.Popen(cmd, env=env, cwd=REPO, stdout=f, stderr=subprocess.STDOUT,
                                stdin=subprocess.DEVNULL, start_new_session=True)
    _wait_all([proc], [log], limit_s, ' '.join(cmd[-8:]))
    with open(log, errors='replace') as f:
        out = f.read()
    lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out[-3000:]
    # the line the driver parses stays small; the full record of a --full run sits in the detail file it names
    assert len(lines[0]) < 4096
    d = json.loads(lines[0])
    if '--full' in cmd:
        with open(os.path.join(REPO, d['detail_file'])) as f:
            d['detail'] = json.load(f)
    else:
        # a plain run prints its line and writes no detail file
        assert 'detail_file' not in d and not os.path.exists(env['BN_BENCH_DETAIL'])
    return d


@pytest.mark.parametrize('launcher', ['torchrun', 'self'])
def test_bench_two_ranks_control_flow(launcher, tmp_path):
    """`bench.py --gpus 2` both ways -- as the driver launches it (torch.distributed.run, one
    process per rank) and PLAINLY (`python bench.py --gpus 2`: the script starts its own ranks, as
    the reference's entry point forks its per-GPU processes, ae_grid_search.py:173-181) -- with both
    ranks on the one GPU over gloo: parameter broadcast, per-step gradient all-reduce (mean over
    the ranks' trials), barrier-bracketed timing, max over ranks, one JSON line from rank 0 with
    the whole-job value and what the collective library saw."""
    env = _child_env(BN_DIST_BACKEND='gloo')
    tail = [os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '1', '--full',
            '--no-cpu-baseline', '--no-secondary']
    if launcher == 'torchrun':
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
               '--master-addr', '127.0.0.1', '--master-port', str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail
    d = _bench_line(cmd, env, tmp_path)
    assert d['n_gpus'] == 2 and d['steps'] == 4 and d['scaling'] == 'weak'
    assert d['config']['global_frames_per_step'] == 512
    assert abs(d['value'] - 512 * 1e3 / d['ms_per_step']) <= 0.01 * d['value']
    assert np.isfinite(d['final_loss'])
    ar = d['allreduce']
    assert ar['world_size'] == 2 and ar['backend'].startswith('gloo') and ar['op'] == 'mean'
    # (the flat arena pads every parameter to 16 bytes)
    assert sum(d['detail']['allreduce']['bucket_bytes']) == ar['gradient_bytes']
    assert 8758285 * 4 <= ar['gradient_bytes'] <= 8758285 * 4 + 16 * 24
    assert ar['allreduce_alone_ms'] > 0


def test_bench_two_ranks_sharded_optimizer(tmp_path):
    """`python bench.py --gpus 2 --shard-optimizer`: the step is reduce-scatter -> Adam on half of
    the arena -> all-gather; the same trajectory as the replicated step (same seeds, same trials:
    the reported loss agrees to rounding)."""
    env = _child_env(BN_DIST_BACKEND='gloo')
    tail = ['--gpus', '2', '--steps', '4', '--warmup', '1', '--no-cpu-baseline', '--no-secondary']
    ds = _bench_line([sys.executable, os.path.join(REPO, 'bench.py')] + tail + ['--shard-optimizer'],
                     env, tmp_path)
    dr = _bench_line([sys.executable, os.path.join(REPO, 'bench.py')] + tail, env, tmp_path)
    assert ds['n_gpus'] == 2 and ds['allreduce']['chosen'].startswith('sharded optimizer')
    assert ds['allreduce']['gradient_bytes'] % (2 * 16) == 0          # two equal 16-byte aligned shards
    assert ds['final_loss'] == pytest.approx(dr['final_loss'], rel=1e-5)


def test_bench_two_ranks_frame_sharded(tmp_path):
    """`python bench.py --gpus 2 --shard frames`: the strong-scaling (parity-exact) reading of
    BASELINE configs[2] -- one 256-frame trial per step, 128 frames per rank, summed gradients;
    the loss it reports is the single-device loss of the same trajectory."""
    # (BN_BENCH_PRIME: the same number of untimed priming steps in both runs -- a single process
    # otherwise primes until its step time has settled)
    env = _child_env(BN_DIST_BACKEND='gloo', BN_BENCH_PRIME='24')
    tail = ['--steps', '4', '--warmup', '1', '--no-cpu-baseline', '--no-secondary']
    d2 = _bench_line([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--shard',
                      'frames'] + tail, env, tmp_path)
    d1 = _bench_line([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + tail, env,
                     tmp_path)
    assert d2['n_gpus'] == 2 and d2['scaling'] == 'strong'
    assert d2['config']['global_frames_per_step'] == 256
    assert d2['config']['frames_per_step_per_gpu'] == 128
    assert abs(d2['value'] - 256 * 1e3 / d2['ms_per_step']) <= 0.01 * d2['value']
    assert d2['allreduce']['op'] == 'sum' and d2['allreduce']['world_size'] == 2
    assert d2['roofline']['algorithmic_bytes_per_launch_avg'] == 128 * 589824
    # same model seed, same trials, same order: after 24 + 1 + 4 steps the two-rank trajectory
    # reports the single-device loss (Adam on rounding-level gradient differences: 1e-4)
    assert d2['final_loss'] == pytest.approx(d1['final_loss'], rel=1e-4)


@pytest.mark.parametrize('launcher', ['torchrun', 'self'])
def test_bench_rank_dies_mid_run_error_line(launcher, tmp_path):
    """the first real N > 1 run happens on the driver's box -- if a rank dies in
    the middle of the timed steps (BN_BENCH_FAULT: rank 1 leaves without a word in front of timed
    step 2) the job must END, non-zero, with ONE JSON line that carries an `error` field, within
    180 s -- not hang in a collective."""
    import time
    env = _child_env(BN_DIST_BACKEND='gloo', BN_BENCH_FAULT='1:2', BN_BENCH_WATCHDOG_S='60',
                     BN_DIST_TIMEOUT_S='60')
    tail = [os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '6', '--warmup', '1',
            '--no-cpu-baseline', '--no-secondary']
    if launcher == 'torchrun':
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
               '--master-addr', '127.0.0.1', '--master-port', str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail
    t0 = time.time()
    proc = subprocess.Popen(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=180)
    except subprocess.TimeoutExpired:
        import signal
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        pytest.fail('bench.py --gpus 2 with a dead rank was still running after 180 s')
    assert proc.returncode != 0, out[-2000:]
    lines = [json.loads(l) for l in out.splitlines() if l.startswith('{') and '"metric"' in l]
    assert len(lines) == 1, (out[-3000:], err[-3000:])
    assert lines[0].get('error') and lines[0]['value'] is None
    assert time.time() - t0 < 180


def test_bench_four_ranks_frame_sharded_defaults(tmp_path):
    """Round 5 defaults of frame sharding over >= 4 ranks -- the step recorded into a HIP graph (its one
    collective, the per-chunk loss table, issued behind the replay), reduce-scatter -> Adam on 1/4 of the arena ->
    all-gather -- with four real processes on the one GPU over gloo: the trajectory reports the single-device
    loss, and the line says what ran."""
    env = _child_env(BN_DIST_BACKEND='gloo', BN_BENCH_PRIME='24')
    tail = ['--steps', '4', '--warmup', '1', '--full', '--no-cpu-baseline', '--no-secondary', '--no-pmc']
    # (started by torch.distributed.run itself: this process, the launcher and the four ranks are six processes
    # with the GPU open, the most a shared machine allows; a plain `bench.py --gpus 4` would add a seventh -- the
    # script's own launch is covered with two ranks above)
    d4 = _bench_line([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4',
                      '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
                      os.path.join(REPO, 'bench.py'), '--gpus', '4', '--shard', 'frames'] + tail,
                     env, tmp_path, limit_s=400)
    d1 = _bench_line([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + tail, env, tmp_path)
    assert d4['n_gpus'] == 4 and d4['scaling'] == 'strong' and d4['hip_graph'] is True
    ar = d4['allreduce']
    assert ar['shard_optimizer'] is True and ar['world_size'] == 4 and ar['op'] == 'sum'
    assert ar['gradient_bytes'] % (4 * 16) == 0
    full = d4['detail']['allreduce']
    assert len(full['devices']) == 4 and len(full['single_gpu_reference']['ms_per_step_per_rank']) == 4
    assert ar['single_gpu_ms_per_step_max'] == full['single_gpu_reference']['ms_per_step_max']
    assert d4['config']['frames_per_step_per_gpu'] == 64
    assert d4['final_loss'] == pytest.approx(d1['final_loss'], rel=1e-4)


def test_bench_two_ranks_frame_sharded_mixed_graph_and_eager(tmp_path):
    """a rank whose graph capture fails keeps launching eagerly while its peer replays (BN_GRAPH_FAULT_RANK:
    rank 1's capture raises).  The collectives must still line up -- the job ends, reports the single-device loss --
    and the record says which ranks replay."""
    env = _child_env(BN_DIST_BACKEND='gloo', BN_BENCH_PRIME='24', BN_GRAPH='1', BN_GRAPH_FAULT_RANK='1')
    tail = ['--steps', '4', '--warmup', '1', '--full', '--no-cpu-baseline', '--no-secondary', '--no-pmc']
    d2 = _bench_line([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--shard', 'frames'] + tail,
                     env, tmp_path, limit_s=400)
    env1 = _child_env(BN_DIST_BACKEND='gloo', BN_BENCH_PRIME='24')
    d1 = _bench_line([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + tail, env1, tmp_path)
    assert d2['n_gpus'] == 2 and d2['hip_graph'] is True
    assert d2['detail']['hip_graph_ranks_recorded'] == [True, False]
    assert d2['final_loss'] == pytest.approx(d1['final_loss'], rel=1e-4)

