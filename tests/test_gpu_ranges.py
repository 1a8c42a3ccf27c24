"""Percentile ranges of latents and labels, selected on the device ("ranges").

1. ``bn_column_count`` / ``bn_column_select`` by direct C calls on operands between guard bands, the outputs pre-filled
   with a sentinel and the workspace guarded too: every value is compared with ``==`` against
   ``tests/ranges_refs.select_ref`` (``np.sort``), NaN positions included; the input keeps its bits; a second call
   gives the same bits.  Every value family of tests/ranges_refs at every shape of SHAPES.
2. ``compute_range`` on device tensors and on numpy lists against ``np.nanpercentile``, exactly.
3. Whole models (the small golden cases, one AE and one PS-VAE): ``latent_ranges`` against ``compute_range`` of the
   latents ``export_latents`` pickled, exactly; ``get_input_range``; the ranges fed to ``traverse_latents``.
"""

import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.data.data_generator import SyntheticSession, SyntheticSessionsGenerator
from behavenet_amd.fitting.eval import (compute_range as eval_compute_range, export_latents, latent_ranges,
                                        latent_ranges_device, traverse_latents)
from behavenet_amd.plotting.cond_ae_utils import compute_range, get_input_range
from tests import ranges_refs as refs
from tests.test_gpu_encode_bf16 import _small
from tests.test_gpu_guard_bands import guarded, _bands_stay_untouched  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG, E_SHAPE = -1, -2
SENTINEL = -77.0
PAD = 7.0e7          # what lies in the columns from d to ld: finite, so a kernel that counted them would show


# ------------------------------------------------------------------------------------------ 1: the kernel
def _three_slabs(d, r):
    """The smallest n whose rows fall into three row blocks with a shorter last one (csrc/column_select.hip's
    partition, restated in ``_hip.column_select_plan``)."""
    n = 2 * max(_hip.COLUMN_SELECT_MIN_ELEMS // d, 1) + 1
    while True:
        _, _, slabs, rows = _hip.column_select_plan(n, d, r)
        if slabs == 3 and n % rows:
            return n
        n += 1


N_THREE = _three_slabs(4, 8)
assert N_THREE < 4 * 10 ** 5 and all(_three_slabs(4, r) == N_THREE for r in (1, 6))
NS = [1, 2, 63, 64, 65, 257, 4099]
DS = [1, 3, 16, 17, 64, 65]
RS = [1, 6, 8]
# (n, d, r, ld, offset in elements off the 16-byte boundary): every n with every d, r taking turns; every r at the
# largest table and at three row blocks; a leading dimension of d + 5; a table 4 bytes off a 16-byte boundary
SHAPES = [(n, d, RS[(i + j) % 3], d, 0) for i, n in enumerate(NS) for j, d in enumerate(DS)]
SHAPES += [(4099, d, r, d, 0) for d in (16, 65) for r in RS]
SHAPES += [(N_THREE, 4, r, 4, 0) for r in RS]
SHAPES += [(257, 17, 6, 22, 0), (4099, 16, 6, 16, 1), (65, 3, 8, 8, 1), (4099, 64, 1, 69, 3)]
SHAPES = sorted(set(SHAPES))


def _place(x, ld=None, offset=0):
    """The table on the device between guard bands, with leading dimension ``ld`` (PAD in the columns from d on; the
    last row ends after its d values) and ``offset`` ELEMENTS off its 16-byte boundary -> (view (n, d), whole)."""
    n, d = x.shape
    ld = d if ld is None else ld
    host = np.full(offset + (n - 1) * ld + d, PAD, dtype=np.float32)
    for i in range(n) if ld != d else ():
        host[offset + i * ld:offset + i * ld + d] = x[i]
    if ld == d:
        host[offset:] = x.reshape(-1)
    whole = guarded(torch.from_numpy(host))
    assert whole.data_ptr() % 16 == 0
    view = torch.as_strided(whole, (n, d), (ld, 1), whole.storage_offset() + offset)
    return view, whole


def _int64(values):
    """int64 values on the device between guard bands."""
    values = torch.as_tensor(np.ascontiguousarray(values), dtype=torch.int64)
    t = guarded(torch.zeros(2 * max(values.numel(), 1))).view(torch.int64)[:values.numel()].view(values.shape)
    t.copy_(values)
    return t


def _workspace(n, d, r):
    nbytes = _hip.load().bn_column_select_ws_bytes(n, d, r)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = guarded(torch.full((nbytes // 4,), float('nan')))
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def _count(xd, ld, ws, nbytes, n_valid, n=None, d=None):
    n, d = (xd.shape[0] if n is None else n), (xd.shape[1] if d is None else d)
    return _hip.load().bn_column_count(xd.data_ptr(), n, d, ld, n_valid.data_ptr(), ws.data_ptr(), nbytes,
                                       torch.cuda.current_stream().cuda_stream)


def _select(xd, ld, ranks, out, ws, nbytes, n=None, d=None, r=None):
    n, d = (xd.shape[0] if n is None else n), (xd.shape[1] if d is None else d)
    r = ranks.shape[0] if r is None else r
    return _hip.load().bn_column_select(xd.data_ptr(), n, d, ld, ranks.data_ptr(), r, out.data_ptr(), ws.data_ptr(),
                                        nbytes, torch.cuda.current_stream().cuda_stream)


def _same_values(got, want, what):
    """``==`` on the values (so the two zeros are one) and the same NaN positions."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), (what, got, want)


def _check(x, r, ld=None, offset=0):
    n, d = x.shape
    ld = d if ld is None else ld
    what = (n, d, r, ld, offset)
    xd, whole = _place(x, ld, offset)
    before = whole.view(torch.int32).clone()
    ws, nbytes = _workspace(n, d, r)
    want_valid = refs.count_ref(x)
    n_valid = _int64(np.full(d, -5))
    assert _count(xd, ld, ws, nbytes, n_valid) == 0, what
    assert np.array_equal(n_valid.cpu().numpy(), want_valid), what
    ranks = refs.ranks_for(want_valid, r)
    want = refs.select_ref(x, ranks)
    ranks_d = _int64(ranks)
    out = guarded(torch.full((r, d), SENTINEL))
    assert _select(xd, ld, ranks_d, out, ws, nbytes) == 0, what
    first = out.clone()
    _same_values(first.cpu().numpy(), want, what)
    # the same bits from a second call, on a workspace that now holds the first call's
    out.fill_(SENTINEL)
    assert _select(xd, ld, ranks_d, out, ws, nbytes) == 0, what
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), what
    # neither the table nor the ranks were written
    assert torch.equal(whole.view(torch.int32), before), what
    assert np.array_equal(ranks_d.cpu().numpy(), ranks), what
    return want


@pytest.mark.parametrize('name', refs.FAMILIES)
def test_kernel_against_the_sorted_column(name):
    for n, d, r, ld, offset in SHAPES:
        x = refs.family(name, n, d)
        want = _check(x, r, ld, offset)
        if r >= 6:
            assert np.isnan(want[4:6]).all()          # ranks -1 and n_valid
        if name == 'all-nan column':
            assert np.isnan(want[:, d // 2]).all()
        assert not np.isnan(want[:2][:, ~np.isnan(x).all(axis=0)]).any()          # ranks 0 and n_valid - 1


def test_the_three_row_blocks_have_a_ragged_tail():
    for r in RS:
        cols, col_groups, slabs, rows = _hip.column_select_plan(N_THREE, 4, r)
        assert (col_groups, slabs) == (1, 3) and 0 < N_THREE - 2 * rows < rows
    # and several column groups are in SHAPES: d = 65 with six and eight slots a column
    assert _hip.column_select_plan(4099, 65, 6)[1] == 7 and _hip.column_select_plan(4099, 65, 8)[1] == 10
    assert _hip.column_select_plan(4099, 65, 8)[2] > 1


def test_refusals_write_nothing():
    x = refs.family('normal', 65, 4)
    xd, whole = _place(x, 9)
    ws, nbytes = _workspace(65, 4, 8)
    ranks = _int64(refs.ranks_for(refs.count_ref(x), 8))
    out = guarded(torch.full((8, 4), SENTINEL))
    n_valid = _int64(np.full(4, -5))
    need = _hip.load().bn_column_select_ws_bytes(65, 4, 6)
    assert _select(xd, 9, ranks, out, ws, need - 1, r=6) == E_SHAPE          # a workspace one byte short
    assert _select(xd, 3, ranks, out, ws, nbytes) == E_SHAPE                 # d > ld
    assert _select(xd, 9, ranks, out, ws, nbytes, r=9) == E_SHAPE
    assert _select(xd, 9, ranks, out, ws, nbytes, r=0) == E_SHAPE
    assert _select(xd, 9, ranks, out, ws, nbytes, n=0) == E_SHAPE
    assert _select(xd, 9, ranks, out, ws, nbytes, d=0) == E_SHAPE
    assert _select(xd, 1030, ranks, out, ws, nbytes, d=1025) == E_SHAPE
    assert _count(xd, 3, ws, nbytes, n_valid) == E_SHAPE
    assert _count(xd, 9, ws, nbytes, n_valid, n=0) == E_SHAPE
    assert _count(xd, 9, ws, 3, n_valid) == E_SHAPE
    lib, st = _hip.load(), torch.cuda.current_stream().cuda_stream
    assert lib.bn_column_select(None, 65, 4, 9, ranks.data_ptr(), 6, out.data_ptr(), ws.data_ptr(), nbytes, st) == E_ARG
    assert lib.bn_column_select(xd.data_ptr(), 65, 4, 9, None, 6, out.data_ptr(), ws.data_ptr(), nbytes, st) == E_ARG
    assert lib.bn_column_select(xd.data_ptr(), 65, 4, 9, ranks.data_ptr(), 6, None, ws.data_ptr(), nbytes, st) == E_ARG
    assert lib.bn_column_select(xd.data_ptr(), 65, 4, 9, ranks.data_ptr(), 6, out.data_ptr(), None, nbytes, st) == E_ARG
    assert lib.bn_column_select(xd.data_ptr() + 2, 65, 4, 9, ranks.data_ptr(), 6, out.data_ptr(), ws.data_ptr(), nbytes,
                                st) == E_SHAPE
    assert lib.bn_column_select(xd.data_ptr(), 65, 4, 9, ranks.data_ptr(), 6, out.data_ptr(), ws.data_ptr() + 4, nbytes,
                                st) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((n_valid == -5).all()) and bool(torch.isnan(ws).all())


def test_wrappers():
    x = refs.family('ten percent nan', 4099, 17)
    xd, _ = _place(x, 22, 1)
    want_valid = refs.count_ref(x)
    got = _hip.column_count(xd)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want_valid)
    ranks = refs.ranks_for(want_valid, 6)
    for given in (ranks, torch.from_numpy(ranks).to(DEV)):
        out = _hip.column_select(xd, given)
        assert out.is_cuda and out.dtype == torch.float32
        _same_values(out.cpu().numpy(), refs.select_ref(x, ranks), 'wrapper')
    # a column slice of a contiguous table is a table with a leading dimension
    wide = torch.from_numpy(x).to(DEV)
    _same_values(_hip.column_select(wide[:, 2:9], ranks[:, 2:9]).cpu().numpy(), refs.select_ref(x[:, 2:9], ranks[:, 2:9]),
                 'slice')
    with pytest.raises(ValueError, match='rows must be contiguous'):
        _hip.column_count(wide[:8, :5].t())
    with pytest.raises(ValueError, match='expected ranks'):
        _hip.column_select(wide, ranks[:, :5])
    with pytest.raises(ValueError, match='ranks a column'):
        _hip.column_select(wide, np.zeros((9, 17), dtype=np.int64))
    with pytest.raises(ValueError, match='1 to 1024 columns'):
        _hip.column_count(torch.zeros((2, 1025), device=DEV))


# ------------------------------------------------------------------------------------------ 2: compute_range
def _want(values, min_p=5, max_p=95):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # (an all-NaN column)
        return {'min': np.nanpercentile(values, min_p, axis=0), 'max': np.nanpercentile(values, max_p, axis=0),
                'med': np.nanpercentile(values, 50, axis=0)}


def _same(got, want, what=''):
    assert sorted(got) == ['max', 'med', 'min']
    for k in want:
        assert isinstance(got[k], np.ndarray) and want[k].dtype == np.float32
        _same_values(got[k], want[k], (what, k))


@pytest.mark.parametrize('min_p,max_p', [(5, 95), (15, 85)])
@pytest.mark.parametrize('name', refs.FAMILIES)
def test_compute_range_is_nanpercentile(name, min_p, max_p):
    x = refs.family(name, 4099, 16)
    want = _want(x, min_p, max_p)
    _same(compute_range([torch.from_numpy(x).to(DEV)], min_p=min_p, max_p=max_p), want, name)
    _same(compute_range([x[:1000], np.array([]), x[1000:]], min_p=min_p, max_p=max_p), want, name)


def test_compute_range_on_a_list_like_a_latents_pickle():
    rng = np.random.default_rng(5)
    lens = rng.integers(20, 101, size=40)
    trials = [rng.standard_normal((int(t), 12)).astype(np.float32) for t in lens]
    listed = []
    for i, t in enumerate(trials):
        listed.append(t)
        if i % 4 == 1:
            listed.append(np.array([]))          # a gap trial
    for min_p, max_p in [(5, 95), (15, 85)]:
        want = _want(np.vstack(trials), min_p, max_p)
        _same(compute_range(listed, min_p, max_p), want)
        _same(eval_compute_range(listed, min_p, max_p), want)
        on_device = [torch.from_numpy(t).to(DEV) if len(t) else t for t in listed]
        _same(compute_range(on_device, min_p, max_p), want)
        mixed = [torch.from_numpy(t).to(DEV) if i % 3 == 0 and len(t) else t for i, t in enumerate(listed)]
        _same(compute_range(mixed, min_p, max_p), want)


# ------------------------------------------------------------------------------------------ 3: whole models
LENS = [20, 33, 12, 27, 16, 40, 12, 25, 18]          # one block of 4 | gap | 1 | gap | 1 | gap trials


def _model(golden, root):
    model, meta = _small(golden=golden, n=8, extra={'expt_dir': root})
    model.eval()
    model.version = 0
    os.makedirs(os.path.join(root, 'version_0'), exist_ok=True)
    return model, meta


def _generator(meta, n_sessions=1, n_labels=0):
    sessions = [SyntheticSession(len(LENS), LENS, meta['dim'], seed=3 + s, n_labels=n_labels, trial_splits='4;1;1;1',
                                 name=('lab', 'expt', 'animal', 'sess%d' % s)) for s in range(n_sessions)]
    return SyntheticSessionsGenerator(sessions, device=DEV, placement='device_u8')


def _pickled(files):
    out = []
    for path in files:
        with open(path, 'rb') as f:
            out.append(pickle.load(f)['latents'])
    return out


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('golden', ['ae_cfg1', 'psvae_cfg4'])
def test_latent_ranges_are_the_ranges_of_the_exported_latents(golden, dtype, tmp_path):
    model, meta = _model(golden, str(tmp_path))
    model.hparams['hip_encode_dtype'] = dtype
    gen = _generator(meta, n_labels=meta['n_labels'])
    latents = _pickled(export_latents(gen, model))[0]
    assert sum(len(l) == 0 for l in latents) == 3          # the gap trials
    for min_p, max_p in [(5, 95), (15, 85)]:
        want = compute_range(latents, min_p, max_p)
        _same(want, _want(np.vstack([l for l in latents if len(l)]), min_p, max_p))
        got = latent_ranges(gen, model, min_p=min_p, max_p=max_p)
        assert got['min'].shape == (np.vstack([l for l in latents if len(l)]).shape[1],)
        _same(got, want, golden)
    dev = latent_ranges_device(gen, model)
    assert dev.is_cuda and dev.dtype == torch.float32
    want = compute_range(latents)
    assert np.array_equal(dev.cpu().numpy(), np.stack([want['min'], want['max'], want['med']]), equal_nan=True)
    # the ranges are what the traversals take
    base = np.vstack([l for l in latents if len(l)])[:1]
    image = traverse_latents(model, base, got['min'], got['max'], [0, 1], 3, '1d')
    assert image.dtype == np.uint8 and image.shape == (2 * meta['dim'][1], 3 * meta['dim'][2])


def test_sessions_of_a_two_session_generator_and_get_input_range(tmp_path):
    root = str(tmp_path)
    model, meta = _model('ae_cfg1', root)
    gen = _generator(meta, n_sessions=2, n_labels=4)
    hp = dict(model.hparams)
    ids = [{'lab': 'lab', 'expt': 'expt', 'animal': 'animal', 'session': 'sess%d' % s} for s in range(2)]
    # without a pickle: the latents are computed
    computed = [get_input_range('latents', hp, sess_ids=ids, sess_idx=s, model=model, data_gen=gen) for s in range(2)]
    both = get_input_range('latents', hp, sess_ids=ids, sess_idx=[0, 1], model=model, data_gen=gen)
    assert not any(f.endswith('.pkl') for f in os.listdir(os.path.join(root, 'version_0')))
    files = export_latents(gen, model)
    assert [os.path.basename(f) for f in files] == ['lab_expt_animal_sess%d_latents.pkl' % s for s in range(2)]
    latents = _pickled(files)
    for s in range(2):
        want = compute_range(latents[s])
        _same(computed[s], want, s)
        _same(latent_ranges(gen, model, s), want, s)
        # with the pickle present: the same dict, and no model is needed
        _same(get_input_range('latents', hp, sess_ids=ids, sess_idx=s), want, s)
    assert not np.array_equal(computed[0]['min'], computed[1]['min'])
    want = compute_range(latents[0] + latents[1])
    _same(both, want)
    _same(latent_ranges(gen, model), want)
    _same(latent_ranges(gen, model, [1, 0]), want)
    _same(get_input_range('latents', hp, sess_ids=ids, sess_idx=[0, 1]), want)
    with pytest.raises(ValueError, match='sessions'):
        latent_ranges(gen, model, 2)
    # labels, masked
    rng = np.random.default_rng(9)
    for sess in gen.datasets:
        sess.labels_masks = [(rng.random(l.shape) < 0.7).astype(np.float32) for l in sess.labels]
    for sessions in (0, [1, 0]):
        host, masked = [], []
        for s in ([sessions] if isinstance(sessions, int) else sessions):
            ds = gen.datasets[s]
            for k in ('train', 'val', 'test'):
                for t in ds.batch_idxs[k]:
                    host.append(ds.labels[int(t)])
                    masked.append(np.where(ds.labels_masks[int(t)] == 0, np.float32(np.nan), ds.labels[int(t)]))
        assert len(host) == 6 * (1 if isinstance(sessions, int) else 2)
        _same(get_input_range('labels', hp, sess_idx=sessions, data_gen=gen), _want(np.vstack(host)))
        _same(get_input_range('labels', hp, sess_idx=sessions, data_gen=gen, apply_label_masks=True, min_p=15, max_p=85),
              _want(np.vstack(masked), 15, 85))
    with pytest.raises(ValueError, match='data_gen'):
        get_input_range('labels', hp, sess_idx=0)
