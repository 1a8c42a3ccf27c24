"""The kernels of csrc/elementwise.hip and csrc/decomposed_kl.hip against float64 on the MI355X, on every path.

References and inputs: tests/elementwise_refs.py (checked without a GPU by tests/test_elementwise_refs_cpu.py).
Gate: ``tests.test_gpu_kernels.close`` as it stands, always with the float64 result: the device's error against
float64, over the result's maximum, is at most 1e-4 and at most max(8 x the fp32 CPU result's error, 3e-6).  The
fp32 CPU result is the same reference evaluated in float32; for Adam it is torch.optim.Adam in fp32.

Paths (EW_THREADS = 256, EW_MAX_BLOCKS = 2048, 524288 threads; sizes derived in elementwise_refs.py):
  * float4 path on the tail sizes 1, 3, 4, 5, 1023, 1027 (tail loop after ``n4 << 2`` alone, vectors alone, both)
    and at N_VEC_STRIDE = 2 098 179, where block 0 runs the float4 loop a second time and n % 4 == 3;
  * scalar path (``vec == 0``) on operands that start 4 bytes past a 16-byte boundary, one operand at a time and
    all together, at the tail sizes and at N_SCALAR_STRIDE = 524 547 (second trip of the scalar loop);
  * the null and non-null branches of ``mask``, ``gscale`` and ``group_scale``;
  * k_scale_frames past 64 x 256 vectors (3, 66736) and past 64 x 256 scalars (2, 16461) per row;
  * k_kl_rows with a ragged last block of four rows and D past the 64 lanes; k_reduce_sum past 256 inputs;
  * Adam's write-through 16-byte buffer stores (``vec == 2``) and its scalar path, over 8 steps, and one step at
    step 1000 from non-zero moments;
  * both generations of the decomposed KL at N just below, at and just above their row-loop strides (256; 128), in
    three input regimes.
Every tensor a kernel writes through an ``out=`` argument or in place lies in a frame of NaN sentinels (64 floats
on either side, inside the test's own allocation) that must keep their bits; inputs lie in such frames too, so a
read outside an operand shows as a NaN.

NOT covered: Adam's ``vec == 1`` variant (plain float4 stores) is taken only by an arena of 2 GiB or more, five of
which do not belong in a test.  The tail loops after ``n4 << 2`` cannot take a second trip (fewer than 4 floats).

Figures measured on the MI355X (largest over all cases of a family; e_hip / e_cpu = error against float64 over the
result's maximum, of the device and of the fp32 CPU result):

    family                         e_hip     e_cpu     cases
    act_bwd                        1.1e-07   1.1e-07   51
    act_fwd                        9.2e-08   8.9e-08   18
    sqerr_frame_sums               1.1e-07   8.4e-08   29
    reduce_sum                     8.6e-08   1.1e-07   24
    sqerr_bwd                      7.2e-08   7.2e-08   56
    scale_frames                   1.0e-07   1.0e-07   12
    reparam_fwd                    6.3e-08   7.0e-08    6
    reparam_bwd                    6.4e-08   6.4e-08    6
    kl_bwd dmu / dlogvar           1.3e-07   1.2e-07   12
    kl_rows                        1.0e-07   1.4e-07   60
    kl mean (reduce_sum of rows)   9.1e-08   2.1e-07   60
    adam p                         1.8e-07   1.8e-07   20 (every step)
    adam m                         6.3e-07   3.9e-07   20
    adam v, vmax                   1.3e-05   2.8e-07   20   e_emul 1.3e-05: see below
    dkl prior terms                1.4e-07   1.3e-07   21
    dkl prior dz / dmu / dlogvar   4.0e-06   3.3e-06   21
    dkl posterior terms            9.8e-08   1.6e-07   21
    dkl posterior gradients        3.4e-07   4.4e-07   21
    dkl posterior log_qz / lse     2.1e-07   2.0e-07   21
    dkl separated terms            1.4e-07   1.0e-07   21
    dkl separated gradients        3.9e-07   5.2e-07   21
    dkl separated log_qz / lse     2.4e-07   1.5e-07   21
    u8_to_unit_float               bit for bit          9

``close`` asks for e_hip <= max(8 x e_cpu, 3e-6).  Every family but two lies under the 3e-6 floor alone, with 4.7x
room at the least (adam m: 1 - b1 is subtracted in fp32, 2.2e-7 above the 0.1 torch multiplies by).  The 'prior'
gradients of the decomposed KL sit above the floor, as the fp32 oracle does (127 x 64: 3.3e-6), at 0.27 of
8 x e_cpu at the most.

The one case of the ``e_emul`` clause -- Adam's v and vmax, in every case that starts from zero moments:
e_hip 1.28e-05 .. 1.31e-05, e_cpu <= 2.8e-07, e_emul equal to e_hip to all four printed digits in each case.  The
kernel receives beta2 as fp32(0.999) = 0.99900001287 and forms 1 - beta2 in fp32: 0.00099998713, 1.29e-5 below the
0.001 that torch multiplies g^2 by, and v = (1 - beta2) sum_k beta2^k g_k^2 carries that factor whole.  The fp32
numpy emulation of the kernel's own formula (``refs.adam_amsgrad_emulated``) shows the same figure, so it is the
rounding of the formula and no indexing error; v and vmax are held to max(8 x e_cpu, 8 x e_emul, 3e-6) and, as ever,
to 1e-4 (7.7x room).  p feels it as 6e-6 of an update of 1e-3 and stays at the fp32 oracle's own 1.8e-7; from
non-zero moments (step 1000) v and vmax are at 2.9e-6.
"""
import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from tests import elementwise_refs as refs
from tests.elementwise_refs import F32, F64, N_SCALAR_STRIDE, N_VEC_STRIDE, SLOPE, TAIL_SIZES
from tests.test_gpu_kernels import close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ACT_PARAMS = pytest.mark.parametrize('act', refs.ACTS, ids=[refs.ACT_IDS[a] for a in refs.ACTS])

# ---------------------------------------------------------------------------------------------------------------
# gate and frames
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF          # a quiet NaN with a payload no kernel produces
PAD = 64
_frames = []


def check(got, want, want64, name):
    """``close`` with the float64 result, after printing both errors (pytest -s)."""
    print('FIGURE %s: e_hip %.3e e_cpu %.3e' % (name, refs.rel_err(got, want64), refs.rel_err(want, want64)))
    close(got, want, want64, name=name)


def check_emulated(got, want, emul, want64, name):
    """For a result whose formula, evaluated term by term in fp32 on the CPU (``emul``), is itself further from
    float64 than the fp32 CPU result: 1e-4 as ever, and max(8 x e_cpu, 8 x e_emul, 3e-6)."""
    e_hip, e_cpu, e_emul = (refs.rel_err(t, want64) for t in (got, want, emul))
    print('FIGURE %s: e_hip %.3e e_cpu %.3e e_emul %.3e' % (name, e_hip, e_cpu, e_emul))
    assert got.shape == want64.shape and bool(torch.isfinite(got).all()), name
    assert e_hip <= 1e-4, '%s: err vs f64 %.3e' % (name, e_hip)
    assert e_hip <= max(8 * e_cpu, 8 * e_emul, 3e-6), \
        '%s: hip err %.3e vs f64, fp32 oracle %.3e, fp32 emulation of the kernel %.3e' % (name, e_hip, e_cpu, e_emul)


def framed(t, misalign=False):
    """A contiguous device view holding ``t`` (a CPU fp32 tensor) inside a larger buffer of sentinels, 64 floats
    before it and at least 64 after; it starts at float 64 (16-byte aligned) or 65 (``misalign``: scalar path)."""
    n = t.numel()
    off = PAD + (1 if misalign else 0)
    raw = torch.full((off + n + PAD + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    view = raw.view(torch.float32)[off:off + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 if misalign else 0)
    _frames.append((raw, off, n))
    return view


def framed_out(shape, misalign=False):
    """A framed output: NaN until written, so an element the kernel skips fails ``close``."""
    return framed(torch.full(tuple(shape), float('nan')), misalign)


def framed_u8(u8, byte_off):
    n = u8.size
    raw = torch.full((byte_off + n + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    view = raw[byte_off:byte_off + n]
    view.copy_(torch.from_numpy(u8))
    assert view.data_ptr() % 16 == byte_off % 16
    return view


def untouched():
    """The sentinels around every framed tensor of this test still have their bits."""
    torch.cuda.synchronize()
    for raw, off, n in _frames:
        assert bool((raw[:off] == SENTINEL).all()), 'write before a framed tensor'
        assert bool((raw[off + n:] == SENTINEL).all()), 'write past the end of a framed tensor'


@pytest.fixture(autouse=True)
def _frames_of_one_test():
    _frames.clear()
    yield
    try:
        untouched()
    finally:
        _frames.clear()


def mis_id(mis):
    return ''.join('m' if m else 'a' for m in mis)


# ---------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------
# (n, (dy, y, out) misaligned)
ACT_BWD_CASES = [(n, (m, m, m)) for n in TAIL_SIZES for m in (False, True)] + \
                [(N_VEC_STRIDE, (False, False, False)), (N_SCALAR_STRIDE, (True, True, True)),
                 (1027, (True, False, False)), (1027, (False, True, False)), (1027, (False, False, True))]


@ACT_PARAMS
@pytest.mark.parametrize('n,mis', ACT_BWD_CASES, ids=['%d-%s' % (n, mis_id(m)) for n, m in ACT_BWD_CASES])
def test_act_bwd(act, n, mis):
    _, y, dy = refs.act_inputs(n, act)
    out = framed_out((n,), mis[2])
    got = _hip.act_bwd(framed(dy, mis[0]), framed(y, mis[1]), act, SLOPE, out=out)
    untouched()
    assert got.data_ptr() == out.data_ptr()
    check(got, refs.act_bwd(dy, y, act, dtype=F32), refs.act_bwd(dy, y, act), 'act_bwd')


@ACT_PARAMS
@pytest.mark.parametrize('n', [1, 1027, N_SCALAR_STRIDE])
@pytest.mark.parametrize('misalign', [False, True], ids=['a', 'm'])
def test_act_fwd(act, n, misalign):
    pre, _, _ = refs.act_inputs(n, act)
    got = _hip.act_fwd(framed(pre, misalign), act, SLOPE)
    check(got, refs.act_fwd(pre, act, dtype=F32), refs.act_fwd(pre, act), 'act_fwd')


# ---------------------------------------------------------------------------------------------------------------
# squared error
# ---------------------------------------------------------------------------------------------------------------
SQ_SHAPES = [(3, 1), (3, 4), (5, 252), (5, 1028), (4, 1023), (2, 16384)]
# (shape, (pred, target, mask) misaligned, masked)
SQ_SUM_CASES = [(s, (m, m, m), k) for s in SQ_SHAPES for m in (False, True) for k in (False, True)] + \
               [((5, 1028), (False, False, True), True), ((5, 1028), (True, False, False), True),
                ((5, 1028), (True, False, False), False)]


def _sq_id(c):
    return '%dx%d-%s-%s' % (c[0] + (mis_id(c[1]), 'mask' if c[2] else 'nomask'))


@pytest.mark.parametrize('shape,mis,masked', SQ_SUM_CASES, ids=[_sq_id(c) for c in SQ_SUM_CASES])
def test_sqerr_frame_sums(shape, mis, masked):
    pred, target, mask = refs.sqerr_inputs(shape, masked)
    got = _hip.sqerr_frame_sums(framed(pred, mis[0]), framed(target, mis[1]),
                                framed(mask, mis[2]) if masked else None)
    check(got, refs.sqerr_frame_sums(pred, target, mask, dtype=F32), refs.sqerr_frame_sums(pred, target, mask),
          'sqerr_frame_sums')


@pytest.mark.parametrize('misalign', [False, True], ids=['a', 'm'])
def test_sqerr_frame_sums_of_a_fully_masked_frame_is_exactly_zero(misalign):
    pred, target, mask = refs.sqerr_inputs((5, 1028), True)
    mask[1] = 0.0
    got = _hip.sqerr_frame_sums(framed(pred, misalign), framed(target, misalign), framed(mask, misalign))
    assert float(got[1]) == 0.0 and not np.signbit(float(got[1]))
    check(got, refs.sqerr_frame_sums(pred, target, mask, dtype=F32), refs.sqerr_frame_sums(pred, target, mask),
          'sqerr_frame_sums')


@pytest.mark.parametrize('n', [1, 37, 255, 256, 257, 1000])
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
def test_reduce_sum(n, mean):
    t = refs.positive_inputs(n)
    scale = 1.0 / n if mean else 1.0
    for misalign in (False, True):
        got = _hip.reduce_sum(framed(t, misalign), scale)
        check(got, refs.reduce_sum(t, scale, dtype=F32), refs.reduce_sum(t, scale), 'reduce_sum')


# (n, (pred, target, mask, out) misaligned)
SQ_BWD_CASES = [(n, (m,) * 4) for n in TAIL_SIZES for m in (False, True)] + \
               [(N_VEC_STRIDE, (False,) * 4), (N_SCALAR_STRIDE, (False, False, False, True))]


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('gscale', [None, 0.7], ids=['nogscale', 'gscale'])
@pytest.mark.parametrize('n,mis', SQ_BWD_CASES, ids=['%d-%s' % (n, mis_id(m)) for n, m in SQ_BWD_CASES])
def test_sqerr_bwd(n, mis, masked, gscale):
    pred, target, mask = refs.sqerr_inputs((n,), masked)
    gs = None if gscale is None else torch.tensor(gscale)
    out = framed_out((n,), mis[3])
    got = _hip.sqerr_bwd(framed(pred, mis[0]), framed(target, mis[1]), framed(mask, mis[2]) if masked else None,
                         0.1, None if gs is None else gs.to(DEV), out=out)
    untouched()
    assert got.data_ptr() == out.data_ptr()
    check(got, refs.sqerr_bwd(pred, target, mask, 0.1, gs, dtype=F32), refs.sqerr_bwd(pred, target, mask, 0.1, gs),
          'sqerr_bwd')


# (3, 66736): 16684 vectors per row, the 64 x 256 threads of a row run the float4 loop twice; (2, 16461): D % 4 == 1,
# scalar, 16461 > 16384 floats per row (two frames cannot name three groups: they name two, unsorted)
SCALE_CASES = [((3, 4), False), ((5, 1028), False), ((4, 1023), False), ((3, 66736), False), ((2, 16461), False),
               ((5, 1028), True)]


@pytest.mark.parametrize('grouped', [False, True], ids=['nogroups', 'groups'])
@pytest.mark.parametrize('shape,misalign', SCALE_CASES,
                         ids=['%dx%d-%s' % (s + ('m' if m else 'a',)) for s, m in SCALE_CASES])
def test_scale_frames_in_place(shape, misalign, grouped):
    t, fs, gs, gof = refs.scale_frames_inputs(shape[0], shape[1], grouped)
    td = framed(t, misalign)
    got = _hip.scale_frames(td, fs.to(DEV), gs.to(DEV) if grouped else None, gof.to(DEV) if grouped else None)
    untouched()
    assert got.data_ptr() == td.data_ptr()
    check(got, refs.scale_frames(t, fs, gs, gof, dtype=F32), refs.scale_frames(t, fs, gs, gof), 'scale_frames')


# ---------------------------------------------------------------------------------------------------------------
# variational tail
# ---------------------------------------------------------------------------------------------------------------
TAIL_N = pytest.mark.parametrize('n', [1, 1027, N_SCALAR_STRIDE])
ALIGN = pytest.mark.parametrize('misalign', [False, True], ids=['a', 'm'])


@TAIL_N
@ALIGN
def test_reparam_fwd(n, misalign):
    mu, lv, eps, _ = refs.latent_inputs((n,))
    got = _hip.reparam_fwd(framed(mu, misalign), framed(lv, misalign), framed(eps, misalign))
    check(got, refs.reparam_fwd(mu, lv, eps, dtype=F32), refs.reparam_fwd(mu, lv, eps), 'reparam_fwd')


@TAIL_N
@ALIGN
def test_reparam_bwd(n, misalign):
    mu, lv, eps, dz = refs.latent_inputs((n,))
    z = refs.reparam_fwd(mu, lv, eps, dtype=F32)
    got = _hip.reparam_bwd(framed(dz, misalign), framed(z, misalign), framed(mu, misalign))
    check(got, refs.reparam_bwd(dz, z, mu, dtype=F32), refs.reparam_bwd(dz, z, mu), 'reparam_bwd')


@TAIL_N
@ALIGN
@pytest.mark.parametrize('gscale', [None, 0.7], ids=['nogscale', 'gscale'])
def test_kl_bwd(n, misalign, gscale):
    mu, lv, _, _ = refs.latent_inputs((n,))
    gs = None if gscale is None else torch.tensor(gscale)
    out = (framed_out((n,), misalign), framed_out((n,), misalign))
    dmu, dlv = _hip.kl_bwd(framed(mu, misalign), framed(lv, misalign), 0.01, None if gs is None else gs.to(DEV),
                           out=out)
    untouched()
    assert dmu.data_ptr() == out[0].data_ptr() and dlv.data_ptr() == out[1].data_ptr()
    w32, w64 = refs.kl_bwd(mu, lv, 0.01, gs, dtype=F32), refs.kl_bwd(mu, lv, 0.01, gs)
    check(dmu, w32[0], w64[0], 'kl_bwd dmu')
    check(dlv, w32[1], w64[1], 'kl_bwd dlogvar')


@pytest.mark.parametrize('N', [1, 3, 4, 5, 201])
@pytest.mark.parametrize('D', [1, 12, 63, 64, 65, 200])
def test_kl_rows_and_their_mean(N, D):
    mu, lv, _, _ = refs.latent_inputs((N, D))
    w32, w64 = refs.kl_rows(mu, lv, dtype=F32), refs.kl_rows(mu, lv)
    for misalign in (False, True):
        rows = _hip.kl_rows(framed(mu, misalign), framed(lv, misalign))
        check(rows, w32, w64, 'kl_rows')
        check(_hip.reduce_sum(rows, 1.0 / N), refs.reduce_sum(w32, 1.0 / N, dtype=F32), w64.mean(), 'kl mean')


# ---------------------------------------------------------------------------------------------------------------
# Adam (amsgrad)
# ---------------------------------------------------------------------------------------------------------------
ALL_A, ALL_M = (False,) * 5, (True,) * 5
# (n, steps, (p, g, m, v, vmax) misaligned)
ADAM_CASES = [(n, 8, ALL_A) for n in (1, 3, 4, 5, 1027)] + \
             [(N_VEC_STRIDE, 3, ALL_A), (1027, 8, (False, True, False, False, False)), (1027, 8, ALL_M),
              (N_SCALAR_STRIDE, 3, ALL_M)]
ADAM_NAMES = ('p', 'm', 'v', 'vmax')


def _torch_adam(p, wd):
    h = refs.ADAM_HYPER
    ref = p.clone().requires_grad_(True)
    return ref, torch.optim.Adam([ref], lr=h['lr'], betas=(h['b1'], h['b2']), eps=h['eps'], weight_decay=wd,
                                 amsgrad=True)


def _adam_step_everywhere(step, g, wd, ref, opt, s64, semul, dev, mis_g):
    """One step of torch's fp32 Adam, the float64 reference, the fp32 emulation and the kernel; the kernel's four
    arenas are compared with all three and their frames checked."""
    h = refs.ADAM_HYPER
    ref.grad = g.clone()
    opt.step()
    s64 = refs.adam_amsgrad(s64[0], g, *s64[1:], wd=wd, step=step, **h)
    semul = refs.adam_amsgrad_emulated(semul[0], g, *semul[1:], wd=wd, step=step, **h)
    _hip.adam_amsgrad_step(dev[0], framed(g, mis_g), dev[1], dev[2], dev[3], h['lr'], h['b1'], h['b2'], h['eps'],
                           wd, step)
    untouched()
    st = opt.state[ref]
    want = (ref.detach(), st['exp_avg'], st['exp_avg_sq'], st['max_exp_avg_sq'])
    for k, name in enumerate(ADAM_NAMES):
        if name in ('v', 'vmax'):
            # 1 - b2 is subtracted in fp32 from fp32(0.999): 1.29e-5 below 0.001, and v is that times g^2.  Measured
            # from zero moments: e_hip 1.28e-5 .. 1.31e-5, e_cpu <= 2.8e-7, e_emul = e_hip to four digits -- the
            # formula's rounding (module docstring)
            check_emulated(dev[k], want[k], semul[k], s64[k], 'adam %s' % name)
        else:
            check(dev[k], want[k], s64[k], 'adam %s' % name)
    return s64, semul


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('n,steps,mis', ADAM_CASES, ids=['%d-%s' % (n, mis_id(m)) for n, _, m in ADAM_CASES])
def test_adam_amsgrad_from_zero_moments(n, steps, mis, wd):
    p0 = refs.adam_start(n)
    zero = torch.zeros(n)
    ref, opt = _torch_adam(p0, wd)
    s64 = (p0.double(),) + (zero.double(),) * 3
    semul = (p0,) + (zero,) * 3
    dev = [framed(t, m) for t, m in zip((p0, zero, zero, zero), (mis[0],) + mis[2:])]
    for step in range(1, steps + 1):
        s64, semul = _adam_step_everywhere(step, refs.adam_grad(n, step), wd, ref, opt, s64, semul, dev, mis[1])


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_amsgrad_at_step_1000_from_nonzero_moments(wd):
    """Bias corrections near 1 (1 - 0.9^1000 = 1, 1 - 0.999^1000 = 0.632) on moments of a run's size: the float64
    reference's state after 8 steps, rounded to fp32, is where all four start."""
    n = 1027
    h = refs.ADAM_HYPER
    s64 = (refs.adam_start(n).double(),) + (torch.zeros(n, dtype=F64),) * 3
    for step in range(1, 9):
        s64 = refs.adam_amsgrad(s64[0], refs.adam_grad(n, step), *s64[1:], wd=wd, step=step, **h)
    start = tuple(t.to(F32) for t in s64)
    assert float(start[2].min()) > 0 and bool((start[3] >= start[2]).all())
    ref, opt = _torch_adam(start[0], wd)
    opt.state[ref] = {'step': torch.tensor(999.0), 'exp_avg': start[1].clone(), 'exp_avg_sq': start[2].clone(),
                      'max_exp_avg_sq': start[3].clone()}
    dev = [framed(t) for t in start]
    _adam_step_everywhere(1000, refs.adam_grad(n, 9), wd, ref, opt, tuple(t.double() for t in start), start, dev,
                          False)
    assert float(opt.state[ref]['step']) == 1000.0


# ---------------------------------------------------------------------------------------------------------------
# uint8 -> float / 255
# ---------------------------------------------------------------------------------------------------------------
U8_CASES = [(n, 64) for n in (1, 3, 4, 5, 1027, N_VEC_STRIDE)] + [(1027, 65), (1027, 66), (1027, 67)]


@pytest.mark.parametrize('n,byte_off', U8_CASES, ids=['%d@%d' % c for c in U8_CASES])
def test_u8_to_unit_float_bit_for_bit(n, byte_off):
    u8 = refs.grey_levels(n)
    got = _hip.u8_to_unit_float(framed_u8(u8, byte_off)).cpu().numpy()
    want = refs.u8_to_unit_float(u8)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# decomposed KL
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', refs.DKL_CASES, ids=refs.DKL_IDS)
def test_decomposed_kl(case):
    """Values and all three input gradients under upstream weights (1.3, -0.4, 2.1), as test_decomposed_kl of
    tests/test_gpu_kernels.py; off the 'prior' regime also the saved logsumexps."""
    from behavenet_amd.hip_functions import decomposed_kl_terms
    regime = case[2]
    res = refs.dkl_reference(*case)
    w32, w64 = res['f32'], res['f64']
    zh, mh, lh = (t.to(DEV).requires_grad_(True) for t in refs.dkl_inputs(*case))
    th = decomposed_kl_terms(zh, mh, lh)
    (th * torch.tensor(refs.DKL_WEIGHTS, device=DEV)).sum().backward()
    check(th, w32[0], w64[0], 'dkl %s terms' % regime)
    check(zh.grad, w32[1], w64[1], 'dkl %s dz' % regime)
    check(mh.grad, w32[2], w64[2], 'dkl %s dmu' % regime)
    check(lh.grad, w32[3], w64[3], 'dkl %s dlogvar' % regime)
    if regime != 'prior':
        _, log_qz, lse = _hip.decomposed_kl_fwd(zh.detach(), mh.detach(), lh.detach())
        assert bool(torch.isfinite(log_qz).all()) and bool(torch.isfinite(lse).all())
        check(log_qz, w32[4], w64[4], 'dkl %s log_qz' % regime)
        check(lse, w32[5], w64[5], 'dkl %s lse' % regime)


@pytest.mark.parametrize('N,D', [(257, 32), (257, 64)], ids=['narrow', 'wide'])
def test_decomposed_kl_repeats_bit_for_bit(N, D):
    """Fixed reduction order in both generations: the same inputs twice, identical bits."""
    z, mu, lv = (t.to(DEV) for t in refs.dkl_inputs(N, D, 'separated'))
    g3 = torch.tensor(refs.DKL_WEIGHTS, device=DEV)
    outs = []
    for _ in range(2):
        out3, log_qz, lse = _hip.decomposed_kl_fwd(z, mu, lv)
        grads = _hip.decomposed_kl_bwd(z, mu, lv, log_qz, lse, g3)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (out3, log_qz, lse) + tuple(grads)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
