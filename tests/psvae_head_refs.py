"""The PS-VAE latent head (csrc/psvae_head.hip: k_psvae_head_rows, _combine, _bwd) as plain torch expressions,
generic in dtype: evaluated in float32 they are the CPU result the device is compared with, in float64 the
reference both are judged against.  The gradients come from autograd, never from a closed form.

The node WITHOUT the decomposed KL (its three terms per chunk, ``dkl3``, are a given input, and what its backward
pass hands down -- ``gz_u``, ``gmu_u``, ``glv_u`` -- are given gradients of z_u, w and lv_u):

    mu = [y | w]      z = mu + eps * exp(logvar)      yhat = y * Dw (+ Db)
    row_sq[n] = sum_l (yhat - labels)^2 (* lmask)     row_kl[n] = 0.5 sum_l (exp(lv) - lv + y^2 - 1)   (l < L)
    per chunk c:  ll_y = -0.5 ln(2 pi) L - 0.5 mean(row_sq)      KL_s = mean(row_kl)
                  T[c] = -alpha ll_y + KL_s + kl MI + beta TC + kl DWKL        cols5[c] = (ll_y, KL_s, MI, TC, DWKL)

``whole_node`` is the same with the three terms taken from oracle/ref_cpu.decomposed_kl per chunk, i.e. everything
``behavenet_amd.hip_functions.psvae_head`` computes.
"""
import math

import torch

LN2PI = math.log(2 * math.pi)

# (N, L, U, chunk bounds): tests/test_gpu_psvae_head.py
CASES = [
    (7, 1, 1, ((0, 7),)),                                   # minimal
    (210, 4, 8, ((0, 200), (200, 210))),                    # the shipped shape
    (530, 11, 5, ((0, 200), (200, 457), (457, 530))),       # second label block; a chunk of 257 rows; 3 row workgroups
    (300, 8, 56, ((0, 300),)),                              # exactly one full block; D = 64
    (260, 16, 3, ((0, 130), (130, 260))),                   # two full blocks
    (64, 17, 2, ((0, 40), (40, 64))),                       # a third block holding one label
]
ALPHA, KL, BETA = 10.0, 0.6, 5.0


def case_id(case):
    return 'N%d_L%d_U%d' % case[:3]


def make_inputs(case, masked, bias, seed=0):
    """float32 inputs of a case (CPU).  ``masked``: an lmask with one fully masked column and one fully masked row;
    ``gT`` is non-uniform and of mixed sign."""
    N, L, U, bounds = case
    g = torch.Generator().manual_seed(1000 * N + 10 * L + U + seed)
    r = lambda *s: torch.rand(s, generator=g)               # noqa: E731
    t = {'y': r(N, L) - 0.5, 'w': r(N, U) - 0.5, 'logvar': r(N, L + U) - 0.7,
         'eps': torch.randn((N, L + U), generator=g), 'Dw': r(L) + 0.5, 'Db': (r(L) - 0.5) if bias else None,
         'labels': r(N, L) - 0.5, 'lmask': None,
         'dkl3': r(len(bounds), 3) * 2 - 0.5,
         'dz': r(N, L + U) - 0.5, 'gT': r(len(bounds)) + 0.3,
         'gz_u': r(N, U) - 0.5, 'gmu_u': r(N, U) - 0.5, 'glv_u': r(N, U) - 0.5}
    t['gT'][::2] *= -1.0
    if len(bounds) == 1:
        t['gT'][0] = -0.7
    if masked:
        m = (r(N, L) > 0.3).float()
        m[:, L // 2] = 0.0
        m[N // 3, :] = 0.0
        t['lmask'] = m
    return t


def _to(t, dtype):
    return None if t is None else t.detach().clone().to(dtype)


def forward(y, w, logvar, eps, Dw, Db, labels, lmask, bounds, dkl3, alpha=ALPHA, kl=KL, beta=BETA):
    """-> dict of z, z_u, lv_u, yhat, row_sq, row_kl, T, cols5 (differentiable)."""
    L = y.shape[1]
    mu = torch.cat([y, w], dim=1)
    z = mu + eps * torch.exp(logvar)
    yhat = y * Dw
    if Db is not None:
        yhat = yhat + Db
    d = (yhat - labels) ** 2
    if lmask is not None:
        d = d * lmask
    row_sq = d.sum(dim=1)
    lv_s = logvar[:, :L]
    row_kl = 0.5 * (torch.exp(lv_s) - lv_s + y ** 2 - 1).sum(dim=1)
    T, cols5 = [], []
    for c, (b, e) in enumerate(bounds):
        ll_y = -0.5 * LN2PI * L - 0.5 * row_sq[b:e].mean()
        kl_s = row_kl[b:e].mean()
        mi, tc, dwkl = dkl3[c]
        cols5.append(torch.stack([ll_y, kl_s, mi, tc, dwkl]))
        T.append(-alpha * ll_y + kl_s + kl * mi + beta * tc + kl * dwkl)
    return {'z': z, 'z_u': z[:, L:], 'lv_u': logvar[:, L:], 'yhat': yhat, 'row_sq': row_sq, 'row_kl': row_kl,
            'T': torch.stack(T), 'cols5': torch.stack(cols5)}


def evaluate(inputs, bounds, dtype, alpha=ALPHA, kl=KL, beta=BETA):
    """Values and autograd gradients of the node in ``dtype``: the objective
    sum(dz z) + sum(gT T) + sum(gz_u z_u) + sum(gmu_u w) + sum(glv_u lv_u) is differentiated with respect to
    y, w, logvar, Dw and Db -- exactly what k_psvae_head_bwd is handed.  Without a bias the gradient ``dDb`` is the
    one of a zero bias (the kernel writes the column sums wherever it is given a buffer)."""
    t = {k: _to(v, dtype) for k, v in inputs.items()}
    L = t['y'].shape[1]
    Db = t['Db'] if t['Db'] is not None else torch.zeros(L, dtype=dtype)
    leaves = [t['y'], t['w'], t['logvar'], t['Dw'], Db]
    for p in leaves:
        p.requires_grad_(True)
    out = forward(t['y'], t['w'], t['logvar'], t['eps'], t['Dw'], Db, t['labels'], t['lmask'], bounds, t['dkl3'],
                  alpha, kl, beta)
    obj = (t['dz'] * out['z']).sum() + (t['gT'] * out['T']).sum() + (t['gz_u'] * out['z_u']).sum() \
        + (t['gmu_u'] * t['w']).sum() + (t['glv_u'] * out['lv_u']).sum()
    dy, dw, dlogvar, dDw, dDb = torch.autograd.grad(obj, leaves)
    res = {k: v.detach() for k, v in out.items()}
    res.update(dy=dy, dw=dw, dlogvar=dlogvar, dDw=dDw, dDb=dDb)
    # the per-row terms of the two column sums (for ``close(sum_of=...)``): d(gT T)/d yhat, and times y
    dyh = torch.zeros_like(res['yhat'])
    for c, (b, e) in enumerate(bounds):
        d = res['yhat'][b:e] - t['labels'][b:e]
        if t['lmask'] is not None:
            d = d * t['lmask'][b:e]
        dyh[b:e] = t['gT'][c] * alpha * d / (e - b)
    res['dDb_terms'] = dyh
    res['dDw_terms'] = dyh * t['y'].detach()
    return res


def whole_node(y, w, logvar, eps, Dw, Db, labels, lmask, bounds, alpha, kl, beta):
    """The full expression behind hip_functions.psvae_head: the decomposed KL of the unsupervised block per chunk by
    oracle/ref_cpu -> dict as ``forward``."""
    from oracle import ref_cpu
    L = y.shape[1]
    z = torch.cat([y, w], dim=1) + eps * torch.exp(logvar)
    dkl3 = [torch.stack(ref_cpu.decomposed_kl(z[b:e, L:], w[b:e], logvar[b:e, L:])) for b, e in bounds]
    return forward(y, w, logvar, eps, Dw, Db, labels, lmask, bounds, dkl3, alpha, kl, beta)
