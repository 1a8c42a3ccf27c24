"""The reference of the PS-VAE latent head (tests/psvae_head_refs.py) WITHOUT a GPU: anchored to the oracle's own
loss functions, its autograd held against finite differences, and the closed forms k_psvae_head_bwd evaluates held
against that autograd in float64 -- so what tests/test_gpu_psvae_head.py compares the kernels with is the node
the models differentiate, read correctly.
"""
import pytest
import torch

from oracle import ref_cpu
from tests import psvae_head_refs as refs


def _f64(case, masked, bias):
    t = refs.make_inputs(case, masked, bias)
    return {k: (None if v is None else v.double()) for k, v in t.items()}


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_reference_is_the_oracles_label_likelihood_and_kl_on_one_chunk(masked, bias):
    """One chunk, sample mode: z is the oracle's reparameterisation, y_hat its DiagLinear, ll_y its gaussian_ll
    of the labels, KL_s its kl_div_to_std_normal of the supervised block, the three other columns its
    decomposed_kl of the unsupervised block, and T the sum of PSVAE.loss without the pixel term."""
    case = (37, 5, 3, ((0, 37),))
    t = _f64(case, masked, bias)
    N, L, U, bounds = case
    out = refs.whole_node(t['y'], t['w'], t['logvar'], t['eps'], t['Dw'], t['Db'], t['labels'], t['lmask'], bounds,
                          refs.ALPHA, refs.KL, refs.BETA)
    mu = torch.cat([t['y'], t['w']], dim=1)
    z = ref_cpu.reparameterize(mu, t['logvar'], t['eps'])
    D = ref_cpu.DiagLinear(L, bias=bias).double()
    with torch.no_grad():
        D.weight.copy_(t['Dw'])
        if bias:
            D.bias.copy_(t['Db'])
        y_hat = D(t['y'])
    ll_y = ref_cpu.gaussian_ll(t['labels'], y_hat, t['lmask'])
    kl_s = ref_cpu.kl_div_to_std_normal(mu[:, :L], t['logvar'][:, :L])
    mi, tc, dwkl = ref_cpu.decomposed_kl(z[:, L:], mu[:, L:], t['logvar'][:, L:])
    total = -refs.ALPHA * ll_y + kl_s + refs.KL * mi + refs.BETA * tc + refs.KL * dwkl
    assert torch.allclose(out['z'], z, rtol=0, atol=1e-15)
    assert torch.allclose(out['yhat'], y_hat, rtol=0, atol=1e-15)
    want = torch.stack([ll_y, kl_s, mi, tc, dwkl])
    assert torch.allclose(out['cols5'][0], want, rtol=1e-13, atol=1e-13), (out['cols5'][0], want)
    assert torch.allclose(out['T'][0], total, rtol=1e-13, atol=1e-13)
    assert torch.equal(out['z_u'], out['z'][:, L:]) and torch.equal(out['lv_u'], t['logvar'][:, L:])


def test_mean_mode_against_sample_mode():
    """eps = 0 is the oracle's mean mode (z = mu = [y | w]); the label likelihood and the supervised KL are
    functions of the means and log-variances alone and do not move with eps."""
    case = (37, 5, 3, ((0, 20), (20, 37)))
    t = _f64(case, True, True)
    args = lambda eps: (t['y'], t['w'], t['logvar'], eps, t['Dw'], t['Db'], t['labels'], t['lmask'],  # noqa: E731
                        case[3], t['dkl3'])
    sample, mean = refs.forward(*args(t['eps'])), refs.forward(*args(torch.zeros_like(t['eps'])))
    assert torch.equal(mean['z'], torch.cat([t['y'], t['w']], dim=1))
    assert not torch.equal(sample['z'], mean['z'])
    for k in ('yhat', 'row_sq', 'row_kl', 'T', 'cols5', 'lv_u'):
        assert torch.equal(sample[k], mean[k]), k
    # per chunk means: the two chunks' terms are those of the chunks evaluated alone
    for c, (b, e) in enumerate(case[3]):
        alone = refs.forward(t['y'][b:e], t['w'][b:e], t['logvar'][b:e], t['eps'][b:e], t['Dw'], t['Db'],
                             t['labels'][b:e], t['lmask'][b:e], ((0, e - b),), t['dkl3'][c:c + 1])
        assert torch.allclose(alone['T'][0], sample['T'][c], rtol=1e-14, atol=0)


@pytest.mark.parametrize('masked', [False, True])
def test_autograd_of_the_reference_against_finite_differences(masked):
    case = (5, 3, 2, ((0, 3), (3, 5)))
    t = _f64(case, masked, True)

    def objective(y, w, logvar, Dw, Db):
        out = refs.forward(y, w, logvar, t['eps'], Dw, Db, t['labels'], t['lmask'], case[3], t['dkl3'])
        return (t['dz'] * out['z']).sum() + (t['gT'] * out['T']).sum() + (t['gz_u'] * out['z_u']).sum() \
            + (t['gmu_u'] * w).sum() + (t['glv_u'] * out['lv_u']).sum()
    leaves = [t[k].clone().requires_grad_(True) for k in ('y', 'w', 'logvar', 'Dw', 'Db')]
    assert torch.autograd.gradcheck(objective, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)
    # ... and evaluate() differentiates that objective
    res = refs.evaluate(t, case[3], torch.float64)
    grads = torch.autograd.grad(objective(*leaves), leaves)
    for k, g in zip(('dy', 'dw', 'dlogvar', 'dDw', 'dDb'), grads):
        assert torch.allclose(res[k], g, rtol=1e-13, atol=1e-15), k


def _kernel_closed_forms(t, bounds, yhat, alpha):
    """What k_psvae_head_bwd evaluates, line by line, in the dtype of its inputs."""
    N, L = t['y'].shape
    dy, dw = torch.zeros_like(t['y']), torch.zeros_like(t['w'])
    dlogvar = torch.zeros_like(t['logvar'])
    dDw, dDb = torch.zeros_like(t['Dw']), torch.zeros_like(t['Dw'])
    for c, (b, e) in enumerate(bounds):
        g, inv = t['gT'][c], 1.0 / (e - b)
        m, lv = t['y'][b:e], t['logvar'][b:e, :L]
        d = yhat[b:e] - t['labels'][b:e]
        if t['lmask'] is not None:
            d = d * t['lmask'][b:e]
        dyh = g * alpha * d * inv
        gz = t['dz'][b:e, :L]
        dy[b:e] = gz + g * inv * m + dyh * t['Dw']
        dlogvar[b:e, :L] = gz * t['eps'][b:e, :L] * torch.exp(lv) + g * inv * 0.5 * (torch.exp(lv) - 1)
        dDw += (dyh * m).sum(dim=0)
        dDb += dyh.sum(dim=0)
    lv = t['logvar'][:, L:]
    gz = t['dz'][:, L:] + t['gz_u']
    dw = gz + t['gmu_u']
    dlogvar[:, L:] = gz * t['eps'][:, L:] * torch.exp(lv) + t['glv_u']
    return {'dy': dy, 'dw': dw, 'dlogvar': dlogvar, 'dDw': dDw, 'dDb': dDb}


@pytest.mark.parametrize('case', refs.CASES, ids=[refs.case_id(c) for c in refs.CASES])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_the_kernels_closed_forms_are_the_autograd_of_the_reference(case, masked, bias):
    t = _f64(case, masked, bias)
    res = refs.evaluate(t, case[3], torch.float64)
    got = _kernel_closed_forms(t, case[3], res['yhat'], refs.ALPHA)
    for k, v in got.items():
        scale = max(float(res[k].abs().max()), 1e-30)
        assert float((v - res[k]).abs().max()) <= 1e-12 * scale, k
    # the per-row terms handed to close(sum_of=...) sum to the two column sums
    assert torch.allclose(res['dDw_terms'].sum(dim=0), res['dDw'], rtol=1e-10, atol=1e-14)
    assert torch.allclose(res['dDb_terms'].sum(dim=0), res['dDb'], rtol=1e-10, atol=1e-14)


def test_fp32_error_of_the_reference_leaves_the_floor_in_charge():
    """The fp32 CPU evaluation is within 1e-6 of float64 on every output of every case (relative to the output's
    maximum), so the 3e-6 floor of ``close`` is what the device is held to."""
    worst = 0.0
    for case in refs.CASES:
        t = refs.make_inputs(case, True, True)
        r32, r64 = refs.evaluate(t, case[3], torch.float32), refs.evaluate(t, case[3], torch.float64)
        for k in ('z', 'yhat', 'row_sq', 'row_kl', 'T', 'dy', 'dw', 'dlogvar'):
            scale = max(float(r64[k].abs().max()), 1e-30)
            worst = max(worst, float((r32[k].double() - r64[k]).abs().max()) / scale)
    assert worst <= 1e-6, worst


def test_case_list_reaches_the_label_blocks_and_row_loops():
    blocks = {(-(-L // 8), L % 8) for N, L, U, b in refs.CASES}
    assert {(1, 1), (1, 4), (2, 3), (1, 0), (2, 0), (3, 1)} == blocks
    assert any(e - b > 256 for N, L, U, bs in refs.CASES for b, e in bs)      # a chunk longer than a workgroup
    assert any(N > 512 for N, L, U, bs in refs.CASES)                         # three row workgroups
    assert any(L + U == 64 for N, L, U, bs in refs.CASES)                     # the widest latent block
    for N, L, U, bs in refs.CASES:
        assert bs[0][0] == 0 and bs[-1][1] == N and all(a[1] == b[0] for a, b in zip(bs, bs[1:]))
    assert any(len(bs) > 1 for N, L, U, bs in refs.CASES)                     # more than one chunk
