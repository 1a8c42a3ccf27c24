"""The float64 references of tests/elementwise_refs.py are right (no GPU): each agrees with torch autograd of its
defining formula in float64 to 1e-12 relative, Adam with torch.optim.Adam(amsgrad=True) over 8 steps, the uint8
conversion with numpy bit for bit; and on every decomposed-KL case of tests/test_gpu_elementwise.py the fp32 oracle
lies within 1e-5 of the float64 oracle, a tenth of the 1e-4 the device is held to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_refs as refs

F32, F64 = torch.float32, torch.float64
RTOL = 1e-12


def agree(got, want, name):
    assert got.dtype == F64 and got.shape == want.shape, name
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got - want).abs().max()) <= RTOL * scale, name


def leaf(t):
    return t.detach().to(F64).requires_grad_(True)


def torch_act(x, act):
    if act == refs.ACT_LRELU:
        return F.leaky_relu(x, refs.SLOPE)
    return torch.sigmoid(x) if act == refs.ACT_SIGMOID else x * 1.0


@pytest.mark.parametrize('act', refs.ACTS, ids=[refs.ACT_IDS[a] for a in refs.ACTS])
def test_activations_match_autograd(act):
    pre, _, dy = refs.act_inputs(1027, act)
    pre = pre[pre != 0]          # at 0 autograd's LeakyReLU and the gradient-from-output agree, sigmoid's too; the
    dy = dy[:pre.numel()]        # zeros are there for the kernels' branches, not for this identity
    x = leaf(pre)
    y = torch_act(x, act)
    y.backward(dy.to(F64))
    agree(refs.act_fwd(pre, act), y.detach(), 'act_fwd')
    agree(refs.act_bwd(dy, y.detach(), act), x.grad, 'act_bwd')


def test_leaky_relu_gradient_at_zero_output_is_the_slope():
    y = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    got = refs.act_bwd(torch.ones(4), y, refs.ACT_LRELU)
    assert got.tolist() == [refs.SLOPE, refs.SLOPE, 1.0, refs.SLOPE]


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('gscale', [None, 0.7])
def test_squared_error_matches_autograd(masked, gscale):
    pred, target, mask = refs.sqerr_inputs((5, 1028), masked)
    gs = None if gscale is None else torch.tensor(gscale)
    p = leaf(pred)
    d = (p - target.to(F64)) ** 2
    if masked:
        d = d * mask.to(F64)
    sums = d.sum(dim=1)
    agree(refs.sqerr_frame_sums(pred, target, mask), sums.detach(), 'frame sums')
    scale = 0.1
    (sums.sum() * scale * (1.0 if gs is None else gs.to(F64))).backward()
    agree(refs.sqerr_bwd(pred, target, mask, scale, gs), p.grad, 'sqerr bwd')
    agree(refs.reduce_sum(sums.detach(), 0.2), sums.detach().sum() * 0.2, 'reduce_sum')


@pytest.mark.parametrize('grouped', [False, True])
def test_scale_frames_matches_a_loop(grouped):
    t, fs, gs, gof = refs.scale_frames_inputs(5, 12, grouped)
    want = t.to(F64).clone()
    for n in range(5):
        want[n] *= fs[n].double() * (gs[gof[n]].double() if grouped else 1.0)
    agree(refs.scale_frames(t, fs, gs, gof), want, 'scale_frames')


@pytest.mark.parametrize('gscale', [None, 0.7])
def test_variational_tail_matches_autograd(gscale):
    mu, lv, eps, dz = refs.latent_inputs((201, 65))
    m, l = leaf(mu), leaf(lv)
    z = eps.to(F64) * torch.exp(l) + m
    z.backward(dz.to(F64))
    agree(refs.reparam_fwd(mu, lv, eps), z.detach(), 'reparam_fwd')
    # the reference takes z as the kernel does, an fp32 tensor: give it the float64 z through its own subtraction
    agree(refs.reparam_bwd(dz, z.detach(), mu), l.grad, 'reparam_bwd')

    m, l = leaf(mu), leaf(lv)
    rows = 0.5 * torch.sum(l.exp() - l + m.pow(2) - 1, dim=1)
    agree(refs.kl_rows(mu, lv), rows.detach(), 'kl_rows')
    gs = None if gscale is None else torch.tensor(gscale)
    scale = 1.0 / 201
    (rows.sum() * scale * (1.0 if gs is None else gs.to(F64))).backward()
    dmu, dlv = refs.kl_bwd(mu, lv, scale, gs)
    agree(dmu, m.grad, 'kl dmu')
    agree(dlv, l.grad, 'kl dlogvar')


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_matches_torch_optim_over_8_steps(wd):
    n = 1027
    h = refs.ADAM_HYPER
    ref = refs.adam_start(n).to(F64).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=h['lr'], betas=(h['b1'], h['b2']), eps=h['eps'], weight_decay=wd, amsgrad=True)
    p = refs.adam_start(n).to(F64)
    m, v, vmax = (torch.zeros(n, dtype=F64) for _ in range(3))
    held = 0
    for step in range(1, 9):
        g = refs.adam_grad(n, step).to(F64)
        ref.grad = g.clone()
        opt.step()
        p, m, v, vmax = refs.adam_amsgrad(p, g, m, v, vmax, wd=wd, step=step, **h)
        held += int((vmax > v).sum())
        st = opt.state[ref]
        for got, want, name in ((p, ref.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v'),
                                (vmax, st['max_exp_avg_sq'], 'vmax')):
            agree(got, want, 'adam %s step %d' % (name, step))
    assert held > n              # the small gradients of steps 3 and 4 leave vmax above v


def test_adam_emulation_differs_from_float64_by_the_rounding_of_the_betas():
    """The fp32 emulation of the kernel's formula is the reference up to rounding; its largest term is
    1 - fp32(0.999) evaluated in fp32, 1.29e-5 below 0.001, which v and vmax carry in full."""
    n = 1027
    h = refs.ADAM_HYPER
    p = refs.adam_start(n)
    g = refs.adam_grad(n, 1)
    z = torch.zeros(n)
    emul = refs.adam_amsgrad_emulated(p, g, z, z, z, wd=0.01, step=1, **h)
    want = refs.adam_amsgrad(p, g, z, z, z, wd=0.01, step=1, **h)
    errs = [refs.rel_err(e, w) for e, w in zip(emul, want)]
    assert errs[0] <= 2e-7 and errs[1] <= 5e-7, errs
    omb2 = float(np.float32(1) - np.float32(0.999))
    for e in errs[2:]:
        assert abs(e - abs(omb2 / 0.001 - 1.0)) <= 3e-7, errs


def test_u8_reference_is_numpy_on_all_levels():
    levels = np.arange(256, dtype=np.uint8)
    want = levels.astype(np.float32) / 255
    got = refs.u8_to_unit_float(levels)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(refs.grey_levels(1027))) == 256


def test_stride_sizes_reach_the_second_trip():
    threads = refs.EW_GRID_THREADS
    n4 = refs.N_VEC_STRIDE >> 2
    assert (n4 + 1 + 255) // 256 > refs.EW_MAX_BLOCKS and threads < n4 < 2 * threads and refs.N_VEC_STRIDE % 4 == 3
    assert threads < refs.N_SCALAR_STRIDE < 2 * threads


@pytest.mark.parametrize('case', refs.DKL_CASES, ids=refs.DKL_IDS)
def test_fp32_oracle_is_within_1e5_of_float64_on_every_decomposed_kl_case(case):
    res = refs.dkl_reference(*case)
    names = ('terms', 'dz', 'dmu', 'dlogvar', 'log_qz', 'lse')
    errs = {n: refs.rel_err(a, b) for n, a, b in zip(names, res['f32'], res['f64'])}
    print('FIGURE dkl-cpu %dx%d-%s: %s' % (case + (' '.join('%s %.2e' % kv for kv in errs.items()),)))
    for t in res['f64']:
        assert bool(torch.isfinite(t).all())
    for n, e in errs.items():
        assert e <= 1e-5, (n, e)
