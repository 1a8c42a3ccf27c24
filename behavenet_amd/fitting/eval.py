"""Inference-only passes over every trial: latents -> ``*_latents.pkl`` (BASELINE config 5), per-frame
reconstruction errors -> ``*_frame_errors.pkl``, uint8 reconstructions -> ``*_reconstructions.npz`` and per-pixel
error / moment maps -> ``*_pixel_stats.pkl``; latent traversals as uint8 mosaics and movies, decoded in one batch
and tiled on the device, point-path traversal movies and session-swap movies among them; reconstruction movies
(original, reconstruction, residual) as uint8 strips; the
percentile ranges of latents and labels, selected on the device; the per-trial label R^2 and MSE of the models
with supervised latents -> ``r2_supervised.csv``, reduced on the device; and the correlation matrices of the latents
per batch, trial or session -> ``corr_unsupervised.csv``, from second moments reduced on the device.

Mirror of ``export_latents`` in the reference ``behavenet/fitting/eval.py:6-118``: same pickle
schema ``{'latents': [per-trial (T x D) arrays, empty for gap trials], 'trials': batch_idxs}``
and file name ``<lab>_<expt>_<animal>_<session>_latents.pkl`` so the ARHMM stage can read it.
Differences below the surface: runs under ``torch.no_grad()`` (the reference builds an unused
graph), accepts device-resident ``uint8`` frames (converted by ``bn_u8_to_unit_float``), and
under ``torch.distributed`` shards trials round-robin over ranks and gathers on rank 0.
"""

import contextlib
import csv
import inspect
import os
import pickle

import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import classifier as _clf
from behavenet_amd.fitting import distributed as bdist
from behavenet_amd.data.utils import label_maps_of
from behavenet_amd.hip_functions import (DECODE_DTYPES, ENCODE_DTYPES, FrameErrRequest, FrameU8Request,
                                         decode_precision, encode_precision, quantising_frames, scoring_frames)
from behavenet_amd.models.aes import encoder_input

__all__ = ['export_latents', 'encode_trial', 'encode_trial_device', 'get_reconstruction', 'export_frame_errors',
           'frame_errors', 'frame_errors_device', 'export_reconstructions', 'reconstruct_trial',
           'reconstruct_trial_device', 'export_pixel_stats', 'pixel_stats', 'pixel_stats_device',
           'summarise_pixel_stats', 'traversal_points', 'traverse_latents', 'traverse_latents_device',
           'traversal_movie', 'traversal_movie_device', 'path_points', 'path_movie_src', 'point_path_movie',
           'point_path_movie_device', 'swap_points', 'swap_layout', 'session_swap_movie', 'session_swap_movie_device',
           'background_medians', 'reconstruction_movie', 'reconstruction_movie_device',
           'percentile_plan', 'percentile_lerp', 'column_percentiles', 'compute_range', 'latent_ranges',
           'latent_ranges_device', 'summarise_label_sums', 'label_r2', 'export_label_r2', 'summarise_gram',
           'latent_correlations', 'export_latent_correlations', 'session_classifier', 'export_session_classifier',
           'classify_table', 'score_table', 'fit_arhmm', 'fit_arhmm_tables', 'export_states', 'export_arhmm',
           'arhmm_grid', 'arhmm_grid_groups', 'fit_arhmm_grid', 'fit_arhmm_grid_tables',
           'arhmm_grid_runs', 'arhmm_grid_states', 'arhmm_grid_selection', 'export_states_grid',
           'check_export_arhmm_grid', 'export_arhmm_grid']


def encode_trial(model, y, sess=None, labels_2d=None, chunk_size=200):
    """Latents (T x D numpy) of one trial, encoded in 200-frame chunks (ref eval.py:51-97)."""
    return encode_trial_device(model, y, sess, labels_2d, chunk_size).cpu().numpy()


def _dtype_key(model, key, env, allowed):
    """``hparams[key]``, else the environment's ``env``, else 'f32'; a value outside ``allowed`` is a ValueError."""
    dtype = model.hparams.get(key, os.environ.get(env, 'f32'))
    if dtype not in allowed:
        raise ValueError("hparams['%s'] (or %s) must be one of %s, got %r" % (key, env, allowed, dtype))
    return dtype


def encode_dtype_of(model):
    """'f32' (default) or 'bf16': ``hparams['hip_encode_dtype']``, else the environment's BN_ENCODE_DTYPE.
    bf16 runs the conv encoder on bf16 operands with fp32 accumulation (hip_functions.conv_stack_bf16)
    for a model in eval mode; it costs about 1e-3 of max|z|."""
    return _dtype_key(model, 'hip_encode_dtype', 'BN_ENCODE_DTYPE', ENCODE_DTYPES)


def decode_dtype_of(model):
    """'f32' (default) or 'bf16': ``hparams['hip_decode_dtype']``, else the environment's BN_DECODE_DTYPE.
    bf16 runs the transposed-conv decoder on bf16 operands with fp32 accumulation
    (hip_functions.convT_stack_bf16) in ``get_reconstruction``; it costs about one grey level of 255 on a
    reconstruction."""
    return _dtype_key(model, 'hip_decode_dtype', 'BN_DECODE_DTYPE', DECODE_DTYPES)


def _model_frames(model, y, labels_2d, floats=None):
    """The frames as the model takes them.  Stored uint8 frames have to be converted before the model sees them
    (``floats``, where the caller has that copy already): for the linear models, and where dense label maps
    (N, L, H, W) are concatenated onto the float tensor.  Conv encoders take the stored uint8 frames as they are:
    value / 255 is fused into the first layer, csrc k_down_c1s<.., U8>; label COORDINATES (N, 2 L) go with the uint8
    frames into the one pass that builds the encoder's input (``models.aes.encoder_input`` divides by 255 there)."""
    dense = labels_2d is not None and not (torch.is_tensor(labels_2d) and labels_2d.dim() == 2)
    if y.dtype == torch.uint8 and (dense or model.hparams.get('model_type', 'conv') != 'conv'):
        return _hip.u8_to_unit_float(y.contiguous()) if floats is None else floats
    return y


def encode_trial_device(model, y, sess=None, labels_2d=None, chunk_size=200):
    """The same latents as a DEVICE tensor: nothing waits for the host (``export_latents`` keeps
    the trials' latents on the device and fetches them once at the end)."""
    with encode_precision(encode_dtype_of(model)):
        return _encode_trial_device(model, y, sess, labels_2d, chunk_size)


def _encode_trial_device(model, y, sess, labels_2d, chunk_size):
    mc = model.hparams['model_class']
    y = _model_frames(model, y, labels_2d)
    n = y.shape[0]
    parts = []
    with torch.no_grad():
        for beg in range(0, n, chunk_size):
            end = min(beg + chunk_size, n)
            y_in = encoder_input(y[beg:end], None if labels_2d is None else labels_2d[beg:end])
            out = model.encoding(y_in, dataset=sess)
            if mc == 'ps-vae':
                cur = torch.cat([out[0], out[1]], dim=1)
            elif mc == 'msps-vae':
                cur = torch.cat([out[0], out[1], out[2]], dim=1)
            else:
                cur = out[0]
            if mc == 'cond-ae-msp':
                cur = model.U(cur)
            parts.append(cur)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


class _GraphedTrialEncoder(object):
    """``encode_trial_device`` as a HIP graph per trial shape: a trial's encode is ~25 launches of
    20-200 us issued through autograd-free Python and ctypes in 0.6-0.9 ms of host time -- longer than
    the device needs for them (0.69 ms for 256 frames of 128x128) once the trials come from a file-backed
    generator that also keeps the main thread busy.  Recorded after the first trial of a shape (same
    kernels on the same operands: bit-identical latents), replayed with the trial copied into the
    graph's static input; trials with extra input channels, host tensors and shapes beyond
    ``max_graphs`` run eagerly.  Opt-in: ``hparams['hip_graph_encode'] = True`` / ``BN_GRAPH_ENCODE=1``."""

    def __init__(self, model, warmup=1, max_graphs=6):
        self.model, self.warmup, self.max_graphs = model, int(warmup), int(max_graphs)
        self._graphs, self._seen, self._refused, self._pool = {}, {}, set(), None
        self.n_replays = self.n_eager = 0
        # opt-in: measured (tools/probe_export.py, one MI355X, idle host) 0.72 ms per 256-frame trial replayed
        # against 0.70 ms launched eagerly -- the encoder is bound by the device; for hosts that are not idle
        self.enabled = bool(model.hparams.get('hip_graph_encode', os.environ.get('BN_GRAPH_ENCODE', '0') == '1'))
        # The reference encodes a trial in chunks of 200 frames (eval.py:51-97): that bounds ITS memory
        # use, nothing else -- in eval mode frames are independent through every encoder (batch norm
        # normalises with the running estimates).  A 256-frame trial as 200 + 56 frames is two passes,
        # the second on a quarter-filled chip: 0.91 ms against 0.69 ms for one pass (tools/probe_export.py).
        # Device-resident trials are therefore encoded whole, up to ``export_chunk_frames`` frames a pass.
        self.chunk = int(model.hparams.get('export_chunk_frames', 1024))

    def __call__(self, y, sess=None, labels_2d=None):
        if not self.enabled or labels_2d is not None or not y.is_cuda or not y.is_contiguous():
            self.n_eager += 1
            return encode_trial_device(self.model, y, sess, labels_2d, self.chunk)
        key = (tuple(y.shape), y.dtype, repr(sess), encode_dtype_of(self.model))
        rec = self._graphs.get(key)
        if rec is None:
            n = self._seen[key] = self._seen.get(key, 0) + 1
            if n <= self.warmup or key in self._refused or len(self._graphs) >= self.max_graphs:
                self.n_eager += 1
                return encode_trial_device(self.model, y, sess, labels_2d, self.chunk)
            rec = self._record(key, y, sess)
            if rec is None:
                self.n_eager += 1
                return encode_trial_device(self.model, y, sess, labels_2d, self.chunk)
        static_in, graph, out = rec
        static_in.copy_(y, non_blocking=True)
        graph.replay()
        self.n_replays += 1
        return out.clone()

    def _record(self, key, y, sess):
        import warnings
        static_in = torch.empty_like(y)
        static_in.copy_(y)
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        try:
            # thread_local: the generator's reader threads and copy stream keep working meanwhile
            with torch.cuda.graph(graph, pool=self._pool, capture_error_mode='thread_local'):
                out = encode_trial_device(self.model, static_in, sess, None, self.chunk)
        except Exception as err:                        # noqa: BLE001 (reported, then eager)
            torch.cuda.synchronize()
            self._refused.add(key)
            warnings.warn('HIP graph capture of the trial encoder failed (%s: %s); trials of shape %s '
                          'stay on eager launches' % (type(err).__name__, err, key[0]))
            return None
        rec = (static_in, graph, out)
        self._graphs[key] = rec
        return rec


def _is_cond_encoder(model):
    """A cond-AE whose ENCODER sees the labels too (as ``labels_sc``: dense maps or coordinates)."""
    return model.hparams['model_class'] == 'cond-ae' and model.hparams.get('conditional_encoder', False)


def _batch_fields(model, data):
    """``(masks, labels, labels_2d)`` of a one-trial batch: the masks if it has any, the labels for the conditional
    classes, ``labels_sc`` for a conditional encoder; None otherwise."""
    masks = data['masks'][0] if 'masks' in data else None
    labels = data['labels'][0] if model.hparams['model_class'] in ('cond-ae', 'cond-vae') else None
    labels_2d = data['labels_sc'][0] if _is_cond_encoder(model) else None
    return masks, labels, labels_2d


def _export_setup(model):
    """The exporters' frames per forward pass; an invalid dtype key is an error before any trial is read."""
    decode_dtype_of(model), encode_dtype_of(model)
    return int(model.hparams.get('export_chunk_frames', 1024))


def _export_per_trial(who, data_generator, model, on_device_fn, on_host_fn=None, sink=None, sink_sharded=False,
                      dtypes=('train', 'val', 'test')):
    """The trial walk the exporters share: every train / val / test trial of every session (or the trials of the splits
    ``dtypes`` alone, in that order; the trials of other splits are not read) goes once through
    ``on_device_fn(images, sess, data, trial)`` (device-resident frames; the results stay on the device and come to
    the host in ONE transfer at the end) or ``on_host_fn(images, sess, data, trial)`` (-> numpy; by default the
    device function's result brought to the host).  Under ``torch.distributed`` a trial is owned by its identity and
    the results are gathered on rank 0.
    -> per session a list with one array per trial (empty for trials in no split), or None on the other ranks.

    With ``sink`` nothing piles up: every result, device tensor or numpy array, goes to ``sink(sess, trial, result)``
    as soon as its trial is done and the returned lists stay empty.  Such a walk is one process's: the caller runs
    it on ONE rank, which owns every trial and enters no collective -- unless ``sink_sharded``: then every rank
    walks the trials it owns into its own sink, and what the sinks hold is the caller's to gather."""
    # multi-session generators serve lists of batches for training; trials are exported one by
    # one (the reference's MSPSVAE.export_latents rebuilds a one-session-per-batch generator,
    # vaes.py:1198-1216)
    single = {'return_multiple': False} \
        if getattr(data_generator, 'n_sessions_per_batch', 1) > 1 else {}
    model.eval()
    if on_host_fn is None:
        def on_host_fn(*args):
            return on_device_fn(*args).cpu().numpy()
    rank, world = (0, 1) if (sink is not None and not sink_sharded) else (bdist.rank(), bdist.world_size())

    results = [[np.array([]) for _ in range(ds.n_trials)] for ds in data_generator.datasets]
    # which rank encodes a trial is a function of the trial's identity (its position in the
    # sorted list of all (session, trial) pairs), not of the order in which the generator
    # happens to serve it on this rank
    wanted = sorted((s_, int(t)) for s_, ds in enumerate(data_generator.datasets)
                    for dt in dtypes for t in ds.batch_idxs[dt])
    owner = {key: i % world for i, key in enumerate(wanted)}
    # generators that can be told to pass over a trial (this package's) are asked not to read,
    # copy or convert the other ranks' trials -- round 4 fetched every trial on every rank -- and to
    # hand out stored uint8 frames as they are (the first conv layer converts in flight)
    try:
        can_skip = 'skip' in inspect.signature(data_generator.next_batch).parameters
    except (TypeError, ValueError):
        can_skip = False
    skip = {'skip': (lambda s_, t_: owner.get((s_, int(t_)), rank) != rank)} \
        if (can_skip and world > 1) else {}
    # (a conditional encoder takes them too once its label maps are built on the device: hip_label_maps = 'device';
    # a generator that serves dense maps all the same is still served, models.aes.encoder_input converts for them)
    conv_u8 = model.hparams.get('model_type', 'conv') == 'conv' and \
        (not _is_cond_encoder(model) or label_maps_of(model.hparams) == 'device')
    serve_prev = getattr(data_generator, 'serve_uint8', None)
    if serve_prev is not None and conv_u8:
        data_generator.serve_uint8 = True
    on_device = {}          # (session, trial) -> device tensor: ONE transfer to the host at the end
    try:
        for dtype in dtypes:
            data_generator.reset_iterators(dtype)
            n_batches = data_generator.n_tot_batches[dtype]
            if single and dtype == 'train':      # the multi generator counts training ITERATIONS
                n_batches = sum(ds.n_batches['train'] for ds in data_generator.datasets)
            for _ in range(n_batches):
                data, sess = data_generator.next_batch(dtype, **single, **skip)
                if data is None:
                    # the generator ran dry before its own count: the remaining trials would be
                    # exported EMPTY without a word
                    raise RuntimeError('%s: the generator ended after %d of %d %s batches'
                                       % (who, _, n_batches, dtype))
                if not isinstance(data, dict):       # SKIPPED: another rank's trial
                    continue
                idx = data['batch_idx']
                idx = idx.item() if hasattr(idx, 'item') else int(idx)
                if owner[(sess, idx)] != rank:
                    continue
                images = data['images'][0]
                if not torch.is_tensor(images):      # generators serving numpy arrays (as_numpy)
                    images = torch.from_numpy(np.asarray(images))
                if sink is not None:
                    sink(sess, idx, (on_device_fn if images.is_cuda else on_host_fn)(images, sess, data, idx))
                elif images.is_cuda:
                    on_device[(sess, idx)] = on_device_fn(images, sess, data, idx)
                else:
                    results[sess][idx] = on_host_fn(images, sess, data, idx)
    finally:
        if serve_prev is not None:
            data_generator.serve_uint8 = serve_prev
    if on_device:
        keys = list(on_device)
        flat = torch.cat([on_device[k] for k in keys], dim=0).cpu().numpy()
        pos = 0
        for k in keys:
            n = on_device[k].shape[0]
            results[k[0]][k[1]] = flat[pos:pos + n].copy()
            pos += n
        del on_device

    if world > 1 and sink is None:
        import torch.distributed as dist
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(results, gathered, dst=0)
        if rank != 0:
            return None
        for other in gathered[1:]:
            for s, per_sess in enumerate(other):
                for i, arr in enumerate(per_sess):
                    if arr.size:
                        results[s][i] = arr
        missing = [key for key in wanted if results[key[0]][key[1]].size == 0]
        if missing:
            raise RuntimeError('%s: %d trials were %s by no rank, e.g. %s' % (
                who, len(missing), 'encoded' if who == 'export_latents' else 'scored', missing[:3]))
    return results


def _version_path(src, *names):
    """``<expt_dir>/version_<n>/<names ...>`` of ``src``: a model (``hparams['expt_dir']``, ``version``) or an hparams
    dict (``['expt_dir']``, ``['version']``)."""
    expt_dir, version = (src['expt_dir'], src['version']) if isinstance(src, dict) \
        else (src.hparams['expt_dir'], src.version)
    return os.path.join(expt_dir, 'version_%i' % version, *names)


def _session_filename(src, dataset, filename, suffix, *dirs):
    """``filename``, or ``<lab>_<expt>_<animal>_<session>_<suffix>`` in the version directory of ``src`` (a model or
    an hparams dict, ``_version_path``), below its directories ``dirs``."""
    if filename is not None:
        return filename
    sess_id = '%s_%s_%s_%s_%s' % (dataset.lab, dataset.expt, dataset.animal, dataset.session, suffix)
    return _version_path(src, *dirs, sess_id)


def _write_csv(filename, header, rows):
    """``header`` and ``rows`` as a table written with the ``csv`` module: a NaN float is an empty field (as pandas
    writes it), any other float ``repr(float(v))``, ints and strings as they are.  -> ``filename``."""
    def field(v):
        return v if not isinstance(v, (float, np.floating)) else '' if np.isnan(v) else repr(float(v))
    with open(filename, 'w', newline='') as f:
        writer = csv.writer(f, lineterminator='\n')
        writer.writerow(header)
        writer.writerows([field(v) for v in row] for row in rows)
    return filename


def _write_per_session(data_generator, src, filename, suffix, key, results, what):
    filenames = []
    for sess, dataset in enumerate(data_generator.datasets):
        out = _session_filename(src, dataset, filename, suffix + '.pkl')
        print('saving %s %i of %i:\n%s' % (what, sess + 1, data_generator.n_datasets, out))
        with open(out, 'wb') as f:
            pickle.dump({key: results[sess], 'trials': dataset.batch_idxs}, f)
        filenames.append(out)
    return filenames


def export_latents(data_generator, model, filename=None):
    """Encode train/val/test trials of every session and pickle them (ref eval.py:6-118)."""
    encode = _GraphedTrialEncoder(model)
    # (host trials go through ``encode_trial``: 200-frame chunks, as the reference encodes them)
    latents = _export_per_trial(
        'export_latents', data_generator, model,
        lambda images, sess, data, trial: encode(images, sess, _batch_fields(model, data)[2]),
        lambda images, sess, data, trial: encode_trial(model, images, sess, _batch_fields(model, data)[2]))
    if latents is None:
        return []
    return _write_per_session(data_generator, model, filename, 'latents', 'latents', latents, 'latents')


# which element of ``model(x)`` holds the latents (the reconstruction is always element 0): AE / cond-AE -> (x_hat, z);
# AEMSP -> (x_hat, z, y); VAE / beta-TC-VAE / cond-VAE -> (x_hat, z, mu, logvar); PS-VAE / MSPS-VAE -> (x_hat, sample,
# mu, logvar, y_hat), where the reference takes mu
_LATENTS_AT = {'ae': 1, 'cond-ae': 1, 'cond-ae-msp': 1, 'vae': 1, 'beta-tcvae': 1, 'cond-vae': 1, 'ps-vae': 2,
               'msps-vae': 2}


def _complete_latents(model, z, labels, apply_inverse_transform):
    """Latents as the decoder takes them: cond-AE / cond-VAE get their ``labels`` appended, AEMSP / PS-VAE / MSPS-VAE
    latents given in the transformed space are mapped back (``apply_inverse_transform``)."""
    cls = model.hparams['model_class']
    if cls in ('cond-ae', 'cond-vae'):
        return torch.cat((z, labels), dim=1)
    if cls in ('cond-ae-msp', 'ps-vae', 'msps-vae') and apply_inverse_transform:
        return model.get_inverse_transformed_latents(z, as_numpy=False)
    return z


def get_reconstruction(model, inputs, dataset=None, return_latents=False, labels=None, labels_2d=None,
                       apply_inverse_transform=True, use_mean=True, as_uint8=False):
    """Images from images (through the whole model) or from latents (through the decoder) as numpy arrays
    (ref fitting/eval.py:286-374; the caller of ``forward`` / ``decoding`` behind the reference's plotting code).

    ``inputs`` with two dimensions are latents, anything else images.  Latents of the label-aware classes are
    completed first: cond-AE / cond-VAE get ``labels`` appended, AEMSP / PS-VAE / MSPS-VAE latents given in the
    transformed space are mapped back (``apply_inverse_transform``).  ``use_mean`` picks the posterior mean for the
    variational classes -- except cond-VAE, which the reference calls without it (kept: it samples there).
    Runs under ``no_grad`` in eval mode.

    ``as_uint8=True`` returns the reconstruction as ``np.uint8`` grey levels, quantised on the device
    (``_hip.unit_float_to_u8``'s rule; a served bf16 decoder writes them in its last layer): a quarter of the copy to
    the host.  The latents are returned as before."""
    cls = model.hparams['model_class']
    model.eval()
    # (arrays go where the model's parameters are -- the reference sends them to hparams['device'], which a model
    # moved with .to() no longer matches)
    t = inputs if torch.is_tensor(inputs) else torch.Tensor(inputs).to(next(model.parameters()).device)
    # (the only place that asks for the bf16 decoder; the encoder half of the image branch stays fp32 whatever
    # hparams['hip_encode_dtype'] says)
    with torch.no_grad(), decode_precision(decode_dtype_of(model)), \
            (quantising_frames() if as_uint8 else contextlib.nullcontext()) as req:
        if t.dim() != 2:
            if cls not in _LATENTS_AT:
                raise ValueError('Invalid model class %s' % cls)
            kwargs = {'dataset': dataset}
            if cls in ('vae', 'beta-tcvae', 'ps-vae', 'msps-vae'):
                kwargs['use_mean'] = use_mean
            elif cls in ('cond-ae', 'cond-vae'):
                kwargs.update(labels=labels, labels_2d=labels_2d)
            out = model(t, **kwargs)
            recon, latents = out[0], out[_LATENTS_AT[cls]]
        else:
            t = _complete_latents(model, t, labels, apply_inverse_transform)
            recon, latents = model.decoding(t, None, None, dataset=None), t
        if as_uint8:
            recon = req.frames if req.frames is not None else _hip.unit_float_to_u8(recon.contiguous())
    recon, latents = recon.detach().cpu().numpy(), latents.detach().cpu().numpy()
    return (recon, latents) if return_latents else recon


# ------------------------------------------------------------------------------------------ a trial in chunks
def _forward_kwargs(cls, sess):
    """How ``_forward_chunks`` calls each class's ``forward`` (the conditional classes get their chunk's labels
    on top): the posterior mean for every variational class, cond-VAE included -- a score must not depend on a draw."""
    kwargs = {'dataset': sess}
    if cls in ('vae', 'beta-tcvae', 'ps-vae', 'msps-vae', 'cond-vae'):
        kwargs['use_mean'] = True
    return kwargs


def _check_frames(who, y):
    if not torch.is_tensor(y) or y.dim() != 4:
        raise ValueError('%s: expected frames (T, C, H, W), got %s'
                         % (who, tuple(y.shape) if torch.is_tensor(y) else type(y).__name__))
    if y.dtype not in (torch.uint8, torch.float32):
        raise ValueError('%s: frames must be uint8 or float32, got %s' % (who, y.dtype))


def _trial_masks(masks, y):
    """``(masks, per_frame)`` for the frames ``y`` of a trial: fp32 and contiguous, per-frame masks
    (models.aes.frame_masks) as they came, one mask for the trial -- (C, H, W) or (1, C, H, W) -- as (C, H, W);
    ``(None, False)`` without masks.  A chunk's mask is ``masks[beg:end] if per_frame else masks``."""
    if masks is None:
        return None, False
    if masks.dim() == y.dim() and masks.shape[0] == 1:
        masks = masks[0]
    return masks.float().contiguous(), masks.dim() == y.dim()


def _forward_chunks(who, model, y, sess, labels, labels_2d, chunk_size, per_chunk, request=None, x=None):
    """One trial through ``model`` in chunks of ``chunk_size`` frames, inside whatever precision blocks the caller
    opened: eval mode, ``no_grad``, ``_forward_kwargs`` plus the chunk's labels for the conditional classes.
    ``y``: fp32 frames or stored uint8 frames (T, C, H, W); ``x``: the frames as the model takes them, where the
    caller has them already (``_model_frames``).  ``request(beg, end)``, if given, is the context manager the chunk's
    ONE model call runs in (``scoring_frames``, ``quantising_frames``); it is closed again when
    ``per_chunk(beg, end, x_hat, req)`` gets the reconstruction and what the request yielded (None without one).

    A function with a callback, not a generator: the requests are thread-local and a consumer that stopped early
    would leave one open until the generator is collected."""
    cls = model.hparams['model_class']
    if cls not in _LATENTS_AT:
        raise ValueError('Invalid model class %s' % cls)
    _check_frames(who, y)
    model.eval()
    y = y.contiguous()
    x = _model_frames(model, y, labels_2d) if x is None else x
    kwargs = _forward_kwargs(cls, sess)
    n = y.shape[0]
    with torch.no_grad():
        for beg in range(0, n, chunk_size):
            end = min(beg + chunk_size, n)
            if cls in ('cond-ae', 'cond-vae'):
                kwargs.update(labels=labels[beg:end], labels_2d=None if labels_2d is None else labels_2d[beg:end])
            with (contextlib.nullcontext() if request is None else request(beg, end)) as req:
                x_hat = model(x[beg:end], **kwargs)[0]
            per_chunk(beg, end, x_hat, req)


# ------------------------------------------------------------------------------------------ frame errors
def _frame_errors_device(model, y, sess, masks, labels, labels_2d, chunk_size, fused=True):
    """``frame_errors_device`` inside whatever precision blocks the caller opened.  ``fused=False`` keeps the
    decoder from scoring in its last layer (tools/bench_frame_errors.py measures both)."""
    y = y.contiguous()
    masks, per_frame = _trial_masks(masks, y)
    out = torch.empty((y.shape[0],), dtype=torch.float32, device=y.device)

    def request(beg, end):
        # (the TARGET stays uint8 where the frames are stored so: the kernels divide by 255 as bn_u8_to_unit_float
        # does; a single mask is expanded because ``_hip._err_operands`` asks for the target's shape)
        target, mask = y[beg:end], masks
        if per_frame:
            mask = masks[beg:end]
        elif masks is not None:
            mask = masks.expand_as(target).contiguous()
        operands = (target, mask, 1.0 / target[0].numel())
        return scoring_frames(*operands) if fused else contextlib.nullcontext(FrameErrRequest(*operands))

    def score(beg, end, x_hat, req):
        scores = req.scores
        if scores is None:
            scores = _hip.frame_sq_err(x_hat.contiguous().view(req.target.shape), req.target, req.mask, req.scale)
        out[beg:end].copy_(scores)

    _forward_chunks('frame_errors', model, y, sess, labels, labels_2d, chunk_size, score, request)
    return out


def frame_errors_device(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200):
    """Per-frame reconstruction error of one trial as an fp32 DEVICE tensor (T,):

        mse[n] = mean over (C, H, W) of (x_hat[n] - y[n])^2 * mask

    -- the reference's ``losses.mse`` (losses.py:56-59) of one frame, the full C H W in the denominator with
    masks too.  ``y``: fp32 frames or stored uint8 frames (value / 255); ``masks``: one (C, H, W) mask for the
    trial or one per frame.  Eval mode, ``no_grad``, the posterior mean for every variational class.  The
    squared errors are reduced on the device (``bn_frame_sq_err``); a frame's value does not depend on
    ``chunk_size`` or on its position in the trial.

    Three lanes: by default the model's own fp32 ``forward`` gives x_hat (every class and architecture);
    ``hparams['hip_decode_dtype'] = 'bf16'`` runs a served decoder on its bf16 stack, whose layer onto the frame
    scores the frames in its epilogue so that x_hat is never written (``bn_convT2d_last_bf16_sqerr``);
    ``hparams['hip_encode_dtype'] = 'bf16'`` does the same for the encoder half.  The keys are independent, and
    this is the one entry point that honours both."""
    with encode_precision(encode_dtype_of(model)), decode_precision(decode_dtype_of(model)):
        return _frame_errors_device(model, y, sess, masks, labels, labels_2d, chunk_size)


def frame_errors(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200):
    """``frame_errors_device`` as a numpy array (T,)."""
    return frame_errors_device(model, y, sess, masks, labels, labels_2d, chunk_size).cpu().numpy()


def export_frame_errors(data_generator, model, filename=None):
    """Score train/val/test trials of every session and pickle the per-frame errors next to the latents:
    ``{'mse': [per-trial (T,) float32 arrays, empty for trials in no split], 'trials': batch_idxs}`` in
    ``<lab>_<expt>_<animal>_<session>_frame_errors.pkl``.  The trial walk is ``export_latents``' (ownership by
    identity under ``torch.distributed``, stored uint8 frames where the model takes them, one transfer to the host
    at the end); every trial goes through ``frame_errors_device`` with the batch's masks and, for the conditional
    classes, labels.  Launched eagerly: the scoring has no HIP-graph replay (``hip_graph_encode`` covers the
    latents alone)."""
    chunk = _export_setup(model)

    def score(images, sess, data, trial):
        return frame_errors_device(model, images, sess, *_batch_fields(model, data), chunk)
    errors = _export_per_trial('export_frame_errors', data_generator, model, score)
    if errors is None:
        return []
    return _write_per_session(data_generator, model, filename, 'frame_errors', 'mse', errors, 'frame errors')


# ------------------------------------------------------------------------------------------ reconstructions
def _reconstruct_trial_device(model, y, sess, labels, labels_2d, chunk_size, fused=True):
    """``reconstruct_trial_device`` inside whatever precision blocks the caller opened.  ``fused=False`` keeps the
    decoder from quantising in its last layer (tools/bench_reconstructions.py measures both)."""
    out = None

    def request(beg, end):
        return quantising_frames() if fused else contextlib.nullcontext(FrameU8Request())

    def store(beg, end, x_hat, req):
        nonlocal out
        frames = req.frames
        if frames is None:
            frames = _hip.unit_float_to_u8(x_hat.contiguous())
        if end - beg == len(y):
            out = frames          # (one pass: the decoder's own tensor, no copy)
            return
        if out is None:
            out = torch.empty((len(y),) + tuple(frames.shape[1:]), dtype=torch.uint8, device=frames.device)
        out[beg:end].copy_(frames)

    _forward_chunks('reconstruct_trial', model, y, sess, labels, labels_2d, chunk_size, store, request)
    if out is None:          # (a trial without frames)
        out = torch.empty((0,) + tuple(y.shape[1:]), dtype=torch.uint8, device=y.device)
    return out


def reconstruct_trial_device(model, y, sess=None, labels=None, labels_2d=None, chunk_size=200):
    """The reconstruction of one trial as stored grey levels, a uint8 DEVICE tensor (T, C, H, W):

        u8 = NaN -> 0, else clamp(rint(x_hat * 255), 0, 255)

    -- fp32 product, round half to even (``bn_unit_float_to_u8``), the inverse of the ``value / 255`` by which stored
    frames are read.  ``y``: fp32 frames or stored uint8 frames.  Eval mode, ``no_grad``, the posterior mean for every
    variational class, cond-VAE included.  A frame's bytes do not depend on ``chunk_size`` or on its position in the
    trial.

    By default the model's own fp32 ``forward`` gives x_hat (every class and architecture) and
    ``bn_unit_float_to_u8`` quantises it; ``hparams['hip_decode_dtype'] = 'bf16'`` runs a served decoder on its bf16
    stack, whose layer onto the frame writes the grey levels itself so that the fp32 x_hat is never written
    (``bn_convT2d_last_bf16_u8``); ``hparams['hip_encode_dtype'] = 'bf16'`` does the same for the encoder half.  The
    keys are independent."""
    with encode_precision(encode_dtype_of(model)), decode_precision(decode_dtype_of(model)):
        return _reconstruct_trial_device(model, y, sess, labels, labels_2d, chunk_size)


def reconstruct_trial(model, y, sess=None, labels=None, labels_2d=None, chunk_size=200):
    """``reconstruct_trial_device`` as a numpy array (T, C, H, W) of uint8."""
    return reconstruct_trial_device(model, y, sess, labels, labels_2d, chunk_size).cpu().numpy()


class _PinnedTrialSink(object):
    """Where ``export_reconstructions`` sends a trial's device result: into one of TWO pinned host buffers, copied
    on a side stream so that trial k's copy runs under trial k + 1's kernels.  An event guards each buffer: before
    a buffer is used again its copy is waited for and the filled buffer handed to ``write(sess, trial, array)``
    (trial k - 1 is written while trial k is copied).  Host memory stays bounded by two trials, device memory by
    the results whose copies are in flight.  Host results go to ``write`` as they are."""

    def __init__(self, write):
        self._write = write
        self._stream = None
        self._slots = [{'buf': None, 'event': None, 'pending': None} for _ in range(2)]
        self._turn = 0

    def _drain(self, slot):
        if slot['pending'] is not None:
            sess, trial, view = slot['pending']
            slot['event'].synchronize()
            slot['pending'] = None
            self._write(sess, trial, view.numpy())

    def __call__(self, sess, trial, result):
        if not torch.is_tensor(result):
            self._write(sess, trial, np.asarray(result))
            return
        if not result.is_cuda:
            self._write(sess, trial, result.numpy())
            return
        result = result.contiguous()
        slot = self._slots[self._turn]
        self._turn ^= 1
        self._drain(slot)
        nbytes = result.numel() * result.element_size()
        if slot['buf'] is None or slot['buf'].numel() < nbytes:
            slot['buf'] = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=result.device)
        if slot['event'] is None:
            slot['event'] = torch.cuda.Event()
        view = slot['buf'][:nbytes].view(result.dtype).view(result.shape)
        self._stream.wait_stream(torch.cuda.current_stream(result.device))
        with torch.cuda.stream(self._stream):
            view.copy_(result, non_blocking=True)
            slot['event'].record(self._stream)
        result.record_stream(self._stream)          # (the result's memory is not reused before the copy has read it)
        slot['pending'] = (sess, trial, view)

    def flush(self):
        """Hand over what is still in flight, oldest first."""
        for slot in (self._slots[self._turn], self._slots[self._turn ^ 1]):
            self._drain(slot)


def export_reconstructions(data_generator, model, filename=None):
    """Reconstruct train/val/test trials of every session and write them next to the latents as a trial store,
    ``<lab>_<expt>_<animal>_<session>_reconstructions.npz``: ``images/trial_%04i`` holds the uint8 (T, C, H, W)
    reconstruction of that trial (``reconstruct_trial_device``: quantised on the device, a quarter of the fp32 copy)
    and a (0, C, H, W) member stands for each trial in no split, so ``open_trial_store(path).read('images', t)``
    lines up with the session's own store and a data generator serves the file as ``images``.

    The trial walk is ``export_latents``', with the batch's labels for the conditional classes, except that
    nothing piles up on the device: each trial leaves through two pinned buffers on a side stream while the next
    one is computed (``_PinnedTrialSink``) and is appended to its store at once (``NpzSessionWriter``; the file
    takes its name when it is complete).  Launched eagerly.  Under ``torch.distributed`` rank 0 alone walks and
    writes every trial -- frames are too large to gather as objects -- and the other ranks return [] at once.
    ``filename`` names the one file of a single-session generator (``ValueError`` with several sessions).
    -> the list of file names."""
    from behavenet_amd.data.trial_store import NpzSessionWriter
    chunk = _export_setup(model)
    if bdist.world_size() > 1 and bdist.rank() != 0:
        return []

    def reconstruct(images, sess, data, trial):
        return reconstruct_trial_device(model, images, sess, *_batch_fields(model, data)[1:], chunk)

    if filename is not None and data_generator.n_datasets > 1:
        raise ValueError('export_reconstructions: one file per session; an explicit filename serves one session, '
                         'the generator has %i' % data_generator.n_datasets)
    filenames = [_session_filename(model, dataset, filename, 'reconstructions.npz')
                 for dataset in data_generator.datasets]
    writers, frame_shape = {}, {}

    def write(sess, trial, array):
        if sess not in writers:
            print('saving reconstructions %i of %i:\n%s' % (sess + 1, data_generator.n_datasets, filenames[sess]))
            writers[sess] = NpzSessionWriter(filenames[sess])
        writers[sess].write('images', trial, array)
        frame_shape[sess] = tuple(array.shape[1:])

    sink = _PinnedTrialSink(write)
    try:
        _export_per_trial('export_reconstructions', data_generator, model, reconstruct, sink=sink)
        sink.flush()
        for sess, dataset in enumerate(data_generator.datasets):
            if sess not in writers:
                continue          # (a session without a train / val / test trial: no frame shape, no store)
            split = set(int(t) for dt in ('train', 'val', 'test') for t in dataset.batch_idxs[dt])
            for trial in range(dataset.n_trials):
                if trial not in split:
                    writers[sess].write('images', trial, np.empty((0,) + frame_shape[sess], dtype=np.uint8))
    except BaseException:
        for w in writers.values():
            w.abort()
        raise
    return [writers[sess].close() for sess in sorted(writers)]


# ------------------------------------------------------------------------------------------ pixel stats
_PIXEL_SPLITS = ('train', 'val', 'test')


def _pixel_stats_device(model, y, sess, masks, labels, labels_2d, chunk_size, out):
    """``pixel_stats_device`` inside whatever precision blocks the caller opened."""
    _check_frames('pixel_stats', y)          # (before ``out`` is held against their shape)
    y = y.contiguous()
    if out is None:
        out = torch.zeros((4,) + tuple(y.shape[1:]), dtype=torch.float64, device=y.device)
    elif tuple(out.shape) != (4,) + tuple(y.shape[1:]) or out.dtype != torch.float64:
        raise ValueError('pixel_stats: out must be a float64 tensor of shape %s, got %s %s'
                         % ((4,) + tuple(y.shape[1:]), out.dtype, tuple(out.shape)))
    # (one mask for the trial is handed to the kernel as it is, not expanded)
    masks, per_frame = _trial_masks(masks, y)

    def accumulate(beg, end, x_hat, req):
        # (the TARGET stays uint8 where the frames are stored so: the kernel divides by 255 as bn_u8_to_unit_float
        # does)
        target = y[beg:end]
        _hip.pixel_stats_accum(x_hat.contiguous().view(target.shape), target, masks[beg:end] if per_frame else masks,
                               out)

    _forward_chunks('pixel_stats', model, y, sess, labels, labels_2d, chunk_size, accumulate)
    return out


def pixel_stats_device(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200, out=None):
    """Per-pixel sums over the frames of one trial as a float64 DEVICE tensor (4, C, H, W):

        [0] sse = sum_n (x_hat[n] - y[n])^2 * mask        [1] w  = sum_n mask
        [2] s1  = sum_n mask * y[n]                       [3] s2 = sum_n mask * y[n]^2

    -- what ``summarise_pixel_stats`` turns into per-pixel MSE and R^2 maps.  With ``out`` the sums are ADDED onto
    that tensor, which is returned: a session's trials accumulate on the device.  ``frame_errors_device``'s contract
    otherwise: ``y`` fp32 frames or stored uint8 frames (value / 255); ``masks`` one (C, H, W) mask for the trial or
    one per frame; eval mode, ``no_grad``, the posterior mean for every variational class.  The squared-error terms
    are ``bn_frame_sq_err``'s in fp32; every sum is float64 in a fixed order (``bn_pixel_stats_accum``), which
    ``chunk_size`` changes and nothing else.

    ``hparams['hip_encode_dtype']`` and ``hparams['hip_decode_dtype']`` are honoured independently, each under its own
    eligibility rules; the decoder writes its fp32 x_hat on every lane and the kernel reads it (no scoring or
    quantising request is opened)."""
    with encode_precision(encode_dtype_of(model)), decode_precision(decode_dtype_of(model)):
        return _pixel_stats_device(model, y, sess, masks, labels, labels_2d, chunk_size, out)


def pixel_stats(model, y, sess=None, masks=None, labels=None, labels_2d=None, chunk_size=200, out=None):
    """``pixel_stats_device`` as a numpy array (4, C, H, W) of float64."""
    return pixel_stats_device(model, y, sess, masks, labels, labels_2d, chunk_size, out).cpu().numpy()


def summarise_pixel_stats(acc, n_frames):
    """Maps and scalars from the (4, C, H, W) sums of ``n_frames`` frames, numpy float64 on the host:

        mse_map  = sse / n_frames                       mean_map = s1 / w
        var_map  = max(s2 / w - mean_map^2, 0)          r2_map   = 1 - sse / (s2 - s1^2 / w)
        mse      = sum(sse) / (n_frames * C H W)        r2       = 1 - sum(sse) / sum(s2 - s1^2 / w)

    ``mse`` is the mean of ``frame_errors`` over the same frames (the reference's denominator, masks included);
    ``r2`` without masks is sklearn's ``r2_score(..., multioutput='variance_weighted')`` with pixels as outputs, the
    definition of ``models.vaes._r2_variance_weighted``.  A pixel whose (mask-weighted) variance is zero -- its
    denominator no larger than the rounding of the float64 sums it is the difference of -- has NaN in ``r2_map`` and
    adds nothing to the scalar's denominator; a pixel of zero weight has NaN in ``mean_map`` and ``var_map`` too."""
    acc = np.asarray(acc, dtype=np.float64)
    if acc.ndim < 2 or acc.shape[0] != 4:
        raise ValueError('summarise_pixel_stats: expected sums (4, C, H, W), got %s' % (acc.shape,))
    n_frames = int(n_frames)
    if n_frames <= 0:
        raise ValueError('summarise_pixel_stats: n_frames must be positive, got %d' % n_frames)
    sse, w, s1, s2 = acc
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = s1 / w
        var = np.maximum(s2 / w - mean * mean, 0.0)
        var[np.isnan(mean)] = np.nan
        denom = s2 - s1 * s1 / w
        # s2 and s1^2 / w each carry up to ~n_frames roundings of 2^-53: a difference below that is no variance
        denom[~(denom > 4.0 * (n_frames + 4) * 2.0 ** -53 * s2)] = 0.0
        r2_map = np.where(denom > 0, 1.0 - sse / denom, np.nan)
        total = float(denom.sum())
        r2 = 1.0 - float(sse.sum()) / total if total > 0 else float('nan')
    return {'mse_map': sse / n_frames, 'mean_map': mean, 'var_map': var, 'r2_map': r2_map,
            'mse': float(sse.sum()) / (n_frames * sse.size), 'r2': r2}


def export_pixel_stats(data_generator, model, filename=None):
    """Accumulate the per-pixel sums of ``pixel_stats_device`` over the train / val / test trials of every session
    and pickle them next to the latents, ``<lab>_<expt>_<animal>_<session>_pixel_stats.pkl``:

        {'stats': {split: (4, C, H, W) float64}, 'n_frames': {split: int},
         'summary': {split: {'mse': float, 'r2': float}, or None for a split without frames}, 'trials': batch_idxs}

    (``summarise_pixel_stats(stats[split], n_frames[split])`` gives the maps).  The trial walk is ``export_latents``'
    (ownership by identity under ``torch.distributed``, stored uint8 frames where the model takes them), with the
    batch's masks and, for the conditional classes, labels; a trial's split is the one ``dataset.batch_idxs`` lists it
    in.  Every trial is added onto its (session, split) accumulator ON THE DEVICE; the accumulators alone come to
    the host.  Under ``torch.distributed`` they are gathered on rank 0 and added in rank order, and the other ranks
    return [].  Launched eagerly.  -> the list of file names."""
    chunk = _export_setup(model)
    split_of = {(s_, int(t)): dt for s_, ds in enumerate(data_generator.datasets)
                for dt in _PIXEL_SPLITS for t in ds.batch_idxs[dt]}
    accs, n_frames, done = {}, {}, []

    def accumulate(images, sess, data, trial):
        key = (sess, split_of[(sess, trial)])
        accs[key] = pixel_stats_device(model, images, sess, *_batch_fields(model, data), chunk, out=accs.get(key))
        n_frames[key] = n_frames.get(key, 0) + int(images.shape[0])
        return None

    _export_per_trial('export_pixel_stats', data_generator, model, accumulate, accumulate,
                      sink=lambda sess, trial, result: done.append((sess, trial)), sink_sharded=True)
    mine = ({k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)) for k, v in accs.items()},
            n_frames, done)
    if bdist.world_size() > 1:
        import torch.distributed as dist
        gathered = [None] * bdist.world_size() if bdist.rank() == 0 else None
        dist.gather_object(mine, gathered, dst=0)
        if bdist.rank() != 0:
            return []
        accs, n_frames, done = {}, {}, []
        for r_accs, r_frames, r_done in gathered:          # (rank order: the sum's order is the ranks')
            for k, v in r_accs.items():
                accs[k] = accs[k] + v if k in accs else v
                n_frames[k] = n_frames.get(k, 0) + r_frames[k]
            done.extend(r_done)
        missing = sorted(set(split_of) - set(done))
        if missing:
            raise RuntimeError('export_pixel_stats: %d trials were accumulated by no rank, e.g. %s'
                               % (len(missing), missing[:3]))
    else:
        accs = mine[0]

    filenames = []
    for sess, dataset in enumerate(data_generator.datasets):
        out = _session_filename(model, dataset, filename, 'pixel_stats.pkl')
        print('saving pixel stats %i of %i:\n%s' % (sess + 1, data_generator.n_datasets, out))
        shapes = [accs[(sess, dt)].shape for dt in _PIXEL_SPLITS if (sess, dt) in accs]
        empty = np.zeros(shapes[0] if shapes else (4, 0, 0, 0), dtype=np.float64)
        stats = {dt: accs.get((sess, dt), empty.copy()) for dt in _PIXEL_SPLITS}
        frames = {dt: int(n_frames.get((sess, dt), 0)) for dt in _PIXEL_SPLITS}
        summary = {}
        for dt in _PIXEL_SPLITS:
            summary[dt] = None
            if frames[dt]:
                full = summarise_pixel_stats(stats[dt], frames[dt])
                summary[dt] = {'mse': full['mse'], 'r2': full['r2']}
        with open(out, 'wb') as f:
            pickle.dump({'stats': stats, 'n_frames': frames, 'summary': summary, 'trials': dataset.batch_idxs}, f)
        filenames.append(out)
    return filenames


# ------------------------------------------------------------------------------------------ latent traversals
def traversal_points(base, mins, maxes, input_idxs, n_frames, mode='1d'):
    """The points of a latent (or label) traversal as one float32 table ``(P, D)`` -> ``(table, (rows, cols))``:
    the values of the reference's ``interpolate_1d`` / ``interpolate_2d`` (plotting/cond_ae_utils.py), every row a
    copy of ``base`` -- (D,) or (1, D) -- with the swept dimensions overwritten by
    ``vals[k] = np.linspace(mins[input_idxs[k]], maxes[input_idxs[k]], n_frames)`` and cast to float32 as
    ``torch.from_numpy(...).float()`` casts.  Panel (i0, i1) is row ``i0 * cols + i1``.

    ``mode='1d'``: ``rows = len(input_idxs)``, ``cols = n_frames``; panel (i0, i1) changes dimension ``input_idxs[i0]``
    to ``vals[i0][i1]``.  ``mode='2d'``: exactly two indices, ``rows = cols = n_frames``; panel (i0, i1) sets
    ``input_idxs[0]`` to ``vals[0][i0]`` and ``input_idxs[1]`` to ``vals[1][i1]``.  Host numpy: the table is a few KB
    and is uploaded once."""
    base = np.asarray(base)
    if base.ndim == 2 and base.shape[0] == 1:
        base = base[0]
    if base.ndim != 1:
        raise ValueError('traversal_points: expected one base point (D,) or (1, D), got %s' % (base.shape,))
    input_idxs = [int(d) for d in input_idxs]
    n_frames = int(n_frames)
    if n_frames < 1:
        raise ValueError('traversal_points: n_frames must be at least 1, got %d' % n_frames)
    if mode not in ('1d', '2d'):
        raise ValueError("traversal_points: mode must be '1d' or '2d', got %r" % (mode,))
    if mode == '2d' and len(input_idxs) != 2:
        raise ValueError('traversal_points: a 2-d traversal sweeps exactly two dimensions, got %d' % len(input_idxs))
    for d in input_idxs:
        if not 0 <= d < base.shape[0]:
            raise ValueError('traversal_points: dimension %d of a base point with %d' % (d, base.shape[0]))
    vals = [np.linspace(mins[d], maxes[d], n_frames) for d in input_idxs]
    rows, cols = (len(input_idxs), n_frames) if mode == '1d' else (n_frames, n_frames)
    # (the assignment casts the float64 values to the base's dtype, as the reference's does)
    table = np.repeat(base[None, :], rows * cols, axis=0).reshape(rows, cols, base.shape[0])
    if mode == '1d':
        for i0, d in enumerate(input_idxs):
            table[i0, :, d] = vals[i0]
    else:
        table[:, :, input_idxs[0]] = vals[0][:, None]
        table[:, :, input_idxs[1]] = vals[1][None, :]
    return np.ascontiguousarray(table.reshape(rows * cols, base.shape[0]).astype(np.float32)), (rows, cols)


def _crop_window(crop_kwargs):
    """``(y_min, x_min, Hc, Wc)`` of the reference's ``crop_kwargs`` (keys x_0, x_ext, y_0, y_ext: the window
    [y_0 - y_ext, y_0 + y_ext) x [x_0 - x_ext, x_0 + x_ext) of ``get_crop``), or the whole frame for None."""
    if not crop_kwargs:
        return None
    y_0, y_ext, x_0, x_ext = (int(crop_kwargs[k]) for k in ('y_0', 'y_ext', 'x_0', 'x_ext'))
    return y_0 - y_ext, x_0 - x_ext, 2 * y_ext, 2 * x_ext


def _checked_crop(model, n_points, ch, crop_kwargs):
    """``_crop_window(crop_kwargs)``, checked with channel ``ch`` against the ``n_points`` frames the model will
    decode: argument errors before anything is decoded."""
    crop = _crop_window(crop_kwargs)
    _hip.check_mosaic_args((n_points, int(model.hparams['n_input_channels']), int(model.hparams['y_pixels']),
                            int(model.hparams['x_pixels'])), ch, crop)
    return crop


def _point_labels(model, labels, n):
    """(n, L) fp32 device labels for the conditional classes from one row (1, L) / (L,) or one per point; else None."""
    if model.hparams['model_class'] not in ('cond-ae', 'cond-vae'):
        return None
    if labels is None:
        raise ValueError('a %s decodes latents together with labels: labels_0 is needed'
                         % model.hparams['model_class'])
    dev = next(model.parameters()).device
    labels = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    labels = labels.to(dev).float()
    if labels.dim() == 1:
        labels = labels[None]
    if labels.shape[0] == 1:
        labels = labels.expand(n, labels.shape[1])
    if labels.dim() != 2 or labels.shape[0] != n:
        raise ValueError('expected labels (1, L) or (%d, L), got %s' % (n, tuple(labels.shape)))
    return labels


def decode_points_device(model, points, labels=None, apply_inverse_transform=True, chunk_size=200):
    """A table of latents ``(P, D)`` through the path ``get_reconstruction`` takes for 2-D inputs, in chunks of
    ``chunk_size`` points, the frames left on the DEVICE: cond-AE / cond-VAE get ``labels`` (one row for all, or one
    per point) appended, AEMSP / PS-VAE / MSPS-VAE latents are mapped back (``apply_inverse_transform``).  Eval mode,
    ``no_grad``.  Returns ``(P, C, H, W)`` fp32 unit floats -- or, under ``hparams['hip_decode_dtype'] = 'bf16'`` on a
    served decoder, the uint8 grey levels its last layer writes (``quantising_frames``)."""
    cls = model.hparams['model_class']
    if cls not in _LATENTS_AT:
        raise ValueError('Invalid model class %s' % cls)
    model.eval()
    dev = next(model.parameters()).device
    t = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    t = t.to(dev).float()
    if t.dim() != 2:
        raise ValueError('expected a table of points (P, D), got %s' % (tuple(t.shape),))
    n = t.shape[0]
    labels = _point_labels(model, labels, n)
    dtype = decode_dtype_of(model)
    parts = []
    with torch.no_grad(), decode_precision(dtype):
        for beg in range(0, n, chunk_size):
            z = _complete_latents(model, t[beg:beg + chunk_size],
                                  None if labels is None else labels[beg:beg + chunk_size], apply_inverse_transform)
            with (quantising_frames() if dtype == 'bf16' else contextlib.nullcontext()) as req:
                x_hat = model.decoding(z, None, None, dataset=None)
            parts.append(req.frames if req is not None and req.frames is not None else x_hat)
    if not parts:
        raise ValueError('a traversal needs at least one point')
    if len(set(p.dtype for p in parts)) != 1:          # (a decoder is served for every chunk or for none)
        parts = [p if p.dtype == torch.uint8 else _hip.unit_float_to_u8(p.contiguous()) for p in parts]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def traverse_latents_device(model, latents_0, mins, maxes, input_idxs, n_frames, mode='1d', labels_0=None,
                            apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """A latent traversal as ONE uint8 DEVICE image ``(rows * Hc, cols * Wc)``: what the reference shows with
    ``interpolate_1d`` / ``interpolate_2d`` + ``plot_1d_frame_array`` / ``plot_2d_frame_array``
    (plotting/cond_ae_utils.py) after P single-frame ``get_reconstruction`` calls and P copies to the host.

    ``traversal_points`` makes the ``(P, D)`` table from ``latents_0``, ``decode_points_device`` decodes it in one
    batch, and one launch (``bn_frame_mosaic_u8``) picks channel ``ch``, crops to ``crop_kwargs`` (the reference's
    keys x_0, x_ext, y_0, y_ext; zero-filled past the bottom and right edge as ``get_crop`` fills; a negative origin
    is a ValueError), quantises (``unit_float_to_u8``'s rule) and tiles panel (i0, i1) at row i0, column i1.  Only
    the image crosses to the host.  ``labels_0``: the labels of a cond-AE / cond-VAE.

    The bytes are the quantised frames of the decoder called on each chunk.  Where the fp32 decoder's kernels choose
    their route by the batch size (2x128x128 frames: batches up to 16 against 24 and more), a frame's x_hat moves in
    its last bits with ``chunk_size`` and with P, as ``get_reconstruction``'s does, and a grey level may turn where
    ``x_hat * 255`` lies at a half."""
    table, (rows, cols) = traversal_points(latents_0, mins, maxes, input_idxs, n_frames, mode)
    crop = _checked_crop(model, table.shape[0], ch, crop_kwargs)
    frames = decode_points_device(model, table, labels_0, apply_inverse_transform, chunk_size)
    src = np.arange(rows * cols, dtype=np.int32).reshape(1, rows, cols)
    return _hip.frame_mosaic_u8(frames, src, ch, crop)[0]


def traverse_latents(model, latents_0, mins, maxes, input_idxs, n_frames, mode='1d', labels_0=None,
                     apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """``traverse_latents_device`` as a numpy array ``(rows * Hc, cols * Wc)`` of uint8."""
    return traverse_latents_device(model, latents_0, mins, maxes, input_idxs, n_frames, mode, labels_0,
                                   apply_inverse_transform, crop_kwargs, ch, chunk_size).cpu().numpy()


def movie_src(n_base, n_dims, n_frames, n_cols, beg=0, end=None):
    """The source table ``(end - beg, n_rows, n_cols)`` of movie frames ``[beg, end)``: at time ``b * n_frames + i``
    panel ``k`` -- row ``k // n_cols``, column ``k % n_cols`` -- shows point ``(b * n_dims + k) * n_frames + i`` of the
    movie's table; panels from ``n_dims`` on are blank (-1)."""
    end = n_base * n_frames if end is None else end
    n_rows = -(-n_dims // n_cols)
    t = np.arange(beg, end)
    b, i = t // n_frames, t % n_frames
    src = np.full((end - beg, n_rows * n_cols), -1, dtype=np.int32)
    src[:, :n_dims] = (b[:, None] * n_dims + np.arange(n_dims)[None, :]) * n_frames + i[:, None]
    return src.reshape(end - beg, n_rows, n_cols)


def traversal_movie_device(model, base_latents, mins, maxes, input_idxs, n_frames, n_cols=None, labels_0=None,
                           apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """The frames of the reference's latent traversal movie (``make_latent_traversal_movie``,
    plotting/cond_ae_utils.py) as a uint8 DEVICE tensor ``(B * n_frames, n_rows * Hc, n_cols * Wc)``: one panel per
    swept dimension, row-major in ``n_cols`` columns (default 3, the reference's) and ``n_rows = ceil(K / n_cols)``
    rows, trailing panels blank (zeros); the base points ``base_latents`` (B, D) follow each other in time.  At time
    ``b * n_frames + i`` panel ``k`` shows base ``b`` with dimension ``input_idxs[k]`` at
    ``np.linspace(mins[d], maxes[d], n_frames)[i]``.

    All ``B * K * n_frames`` points are decoded in one batched pass (``decode_points_device``) and tiled by one
    mosaic launch per ``chunk_size`` movie frames; only the movie crosses to the host.  ``labels_0``: (1, L) or
    (B, L) labels of a cond-AE / cond-VAE; the other arguments as in ``traverse_latents_device``."""
    base = np.asarray(base_latents)
    if base.ndim == 1:
        base = base[None]
    if base.ndim != 2 or base.shape[0] < 1:
        raise ValueError('traversal_movie: expected base points (B, D), got %s' % (base.shape,))
    n_base, n_dims = base.shape[0], len(input_idxs)
    n_cols = 3 if n_cols is None else int(n_cols)
    if n_dims < 1 or n_cols < 1:
        raise ValueError('traversal_movie: %d swept dimensions in %d columns' % (n_dims, n_cols))
    tables = [traversal_points(b, mins, maxes, input_idxs, n_frames, '1d')[0] for b in base]
    table = np.concatenate(tables, axis=0)
    per_base = n_dims * int(n_frames)
    crop = _checked_crop(model, table.shape[0], ch, crop_kwargs)
    labels = _point_labels(model, labels_0, n_base)
    if labels is not None:
        labels = labels.repeat_interleave(per_base, dim=0)
    frames = decode_points_device(model, table, labels, apply_inverse_transform, chunk_size)
    n_t = n_base * int(n_frames)
    parts = []
    for beg in range(0, n_t, chunk_size):          # (one launch per chunk of time)
        src = movie_src(n_base, n_dims, int(n_frames), n_cols, beg, min(beg + chunk_size, n_t))
        parts.append(_hip.frame_mosaic_u8(frames, src, ch, crop))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def traversal_movie(model, base_latents, mins, maxes, input_idxs, n_frames, n_cols=None, labels_0=None,
                    apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """``traversal_movie_device`` as a numpy array ``(B * n_frames, n_rows * Hc, n_cols * Wc)`` of uint8."""
    return traversal_movie_device(model, base_latents, mins, maxes, input_idxs, n_frames, n_cols, labels_0,
                                  apply_inverse_transform, crop_kwargs, ch, chunk_size).cpu().numpy()


# ------------------------------------------------------------------------------------------ point paths
def path_points(points, n_frames):
    """Every step of the path through ``points`` (n_points, D), as the reference's ``interpolate_point_path`` walks
    it (plotting/cond_ae_utils.py:786-802): leg ``p`` from ``points[p]`` to ``points[p + 1]`` has ``n_frames[p] + 1``
    steps ``p0 + pn * ((p1 - p0) / n_frames[p])``, ``pn = 0 .. n_frames[p]`` -- both ends, so the end of one leg and
    the start of the next both appear.  ``n_frames``: an int for every leg, or one per leg (another length is the
    reference's AssertionError).  The arithmetic is numpy's in the dtype of ``points``.  -> ``(sum(n_frames + 1),
    D)``."""
    points = np.asarray(points)
    if points.ndim != 2:
        raise ValueError('path_points: expected points (n_points, D), got %s' % (points.shape,))
    n_points = points.shape[0]
    if isinstance(n_frames, (int, np.integer)):
        n_frames = [n_frames] * (n_points - 1)
    assert len(n_frames) == (n_points - 1)
    n_frames = [int(n) for n in n_frames]
    if any(n < 1 for n in n_frames):
        raise ValueError('path_points: a leg needs at least one frame, got n_frames %s' % (n_frames,))
    legs = []
    for p, n in enumerate(n_frames):
        p0, p1 = points[None, p], points[None, p + 1]
        p_vec = (p1 - p0) / n
        # (a Python int times the vector, for every pn at once: the step number in the vector's own dtype)
        legs.append(p0 + np.arange(n + 1).astype(p_vec.dtype)[:, None] * p_vec)
    if not legs:
        return np.zeros((0, points.shape[1]), dtype=points.dtype)
    return np.concatenate(legs, axis=0)


def path_movie_src(n_base, n_panels, n_steps, n_buffer_frames, n_cols, order_idxs=None, beg=0, end=None):
    """The source table ``(end - beg, n_rows, n_cols)`` of frames ``[beg, end)`` of a point-path movie.  A base point
    takes ``n_steps`` movie frames and, where there are several base points, ``n_buffer_frames`` blank ones after
    them (every panel -1), the last base point included.  At step ``i`` of base ``b`` position ``j`` of the grid --
    row ``j // n_cols``, column ``j % n_cols`` -- shows panel ``k = order_idxs[j]`` (default: ``j``), which is point
    ``(b * n_panels + k) * n_steps + i`` of the movie's table; positions past ``len(order_idxs)`` are blank."""
    order = np.arange(n_panels) if order_idxs is None else np.asarray(order_idxs, dtype=np.int64).reshape(-1)
    per_base = n_steps + (n_buffer_frames if n_base > 1 else 0)
    end = n_base * per_base if end is None else end
    n_rows = -(-len(order) // n_cols)
    t = np.arange(beg, end)
    b, i = t // per_base, t % per_base
    src = np.full((end - beg, n_rows * n_cols), -1, dtype=np.int32)
    shown = (b[:, None] * n_panels + order[None, :]) * n_steps + i[:, None]
    src[:, :len(order)] = np.where(i[:, None] < n_steps, shown, -1)
    return src.reshape(end - beg, n_rows, n_cols)


def _mosaic_in_chunks(frames, src_of, n_t, ch, crop, chunk_size):
    """One mosaic launch per ``chunk_size`` movie frames, ``src_of(beg, end)`` naming their sources."""
    parts = [_hip.frame_mosaic_u8(frames, src_of(beg, min(beg + chunk_size, n_t)), ch, crop)
             for beg in range(0, n_t, chunk_size)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def point_path_movie_device(model, base_latents, panels, n_frames=10, n_buffer_frames=5, n_cols=3, order_idxs=None,
                            labels_0=None, apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """The frames the reference's ``make_latent_traversal_movie`` plays (plotting/cond_ae_utils.py:2400-2511, through
    ``interpolate_point_path``) as a uint8 DEVICE tensor ``(T, n_rows * Hc, n_cols * n_ch * Wc)``.

    ``panels`` is a list of ``(dim, lo, hi)``; the caller lists the label dimensions first and the latent dimensions
    after them, as the reference does.  For base point ``b`` of ``base_latents`` (B, D) and panel ``k`` the path runs
    through three points, the base row with ``dim`` set to ``lo``, ``hi`` and ``lo`` again: min -> max -> min in two
    legs of ``n_frames + 1`` steps (``path_points``; the turning point appears twice).  Panel ``k`` sits at row ``k //
    n_cols``, column ``k % n_cols`` after ``order_idxs`` (a list of panel numbers, default all in order) is applied;
    trailing positions are blank.  With B > 1, ``n_buffer_frames`` all-zero frames follow every base point, the last
    one included, as in the reference; so ``T = B * (2 * (n_frames + 1) + n_buffer_frames)``, or ``2 * (n_frames +
    1)`` for one base point.

    All ``B * K * 2 * (n_frames + 1)`` points are decoded in one batched pass (``decode_points_device``, which honours
    ``hparams['hip_decode_dtype']`` as ``traversal_movie_device`` does) and tiled by one mosaic launch per
    ``chunk_size`` movie frames; only the movie crosses to the host.  ``ch``: one channel, None for all channels side
    by side in every panel, or ``(ch0, n_ch)`` (``_hip.frame_mosaic_u8``).  ``labels_0``: (1, L) or (B, L) labels of a
    cond-AE / cond-VAE, whose panels sweep latents here (a label path of those classes goes through the whole model:
    ``plotting.cond_ae_utils.interpolate_point_path``).

    Departure: the reference crops its label panels alone, so its figure has panels of two sizes; a mosaic has one
    window, ``crop_kwargs``, for every panel."""
    base = np.asarray(base_latents)
    if base.ndim == 1:
        base = base[None]
    if base.ndim != 2 or base.shape[0] < 1:
        raise ValueError('point_path_movie: expected base points (B, D), got %s' % (base.shape,))
    n_base, n_lat = base.shape
    panels = [(int(d), lo, hi) for d, lo, hi in panels]
    n_frames, n_buffer_frames, n_cols, chunk_size = int(n_frames), int(n_buffer_frames), int(n_cols), int(chunk_size)
    if not panels or n_cols < 1 or n_frames < 1 or n_buffer_frames < 0 or chunk_size < 1:
        raise ValueError('point_path_movie: %d panels in %d columns, n_frames %d, n_buffer_frames %d, chunk_size %d'
                         % (len(panels), n_cols, n_frames, n_buffer_frames, chunk_size))
    for d, _, _ in panels:
        if not 0 <= d < n_lat:
            raise ValueError('point_path_movie: dimension %d of a base point with %d' % (d, n_lat))
    if order_idxs is not None:
        order_idxs = [int(k) for k in order_idxs]
        if not order_idxs or min(order_idxs) < 0 or max(order_idxs) >= len(panels):
            raise ValueError('point_path_movie: order_idxs %s of %d panels' % (order_idxs, len(panels)))
    n_steps = 2 * (n_frames + 1)
    legs = []
    for row in base:
        for d, lo, hi in panels:
            points = np.array([row] * 3)
            points[0, d], points[1, d], points[2, d] = lo, hi, lo
            legs.append(path_points(points, n_frames))
    table = np.ascontiguousarray(np.concatenate(legs, axis=0).astype(np.float32))
    crop = _checked_crop(model, table.shape[0], ch, crop_kwargs)
    labels = _point_labels(model, labels_0, n_base)
    if labels is not None:
        labels = labels.repeat_interleave(len(panels) * n_steps, dim=0)
    frames = decode_points_device(model, table, labels, apply_inverse_transform, chunk_size)
    n_t = n_base * (n_steps + (n_buffer_frames if n_base > 1 else 0))
    return _mosaic_in_chunks(
        frames, lambda beg, end: path_movie_src(n_base, len(panels), n_steps, n_buffer_frames, n_cols, order_idxs,
                                                beg, end), n_t, ch, crop, chunk_size)


def point_path_movie(model, base_latents, panels, n_frames=10, n_buffer_frames=5, n_cols=3, order_idxs=None,
                     labels_0=None, apply_inverse_transform=True, crop_kwargs=None, ch=0, chunk_size=200):
    """``point_path_movie_device`` as a numpy array ``(T, n_rows * Hc, n_cols * n_ch * Wc)`` of uint8."""
    return point_path_movie_device(model, base_latents, panels, n_frames, n_buffer_frames, n_cols, order_idxs,
                                   labels_0, apply_inverse_transform, crop_kwargs, ch, chunk_size).cpu().numpy()


# ------------------------------------------------------------------------------------------ session swaps
def swap_points(latents, background_idxs, medians):
    """The latents ``(T, D)`` of a trial once per session, ``(S * T, D)``: block ``s`` is the trial with the columns
    ``background_idxs`` set to row ``s`` of ``medians`` (S, n_background) -- the reference's ``latents_np[:,
    background_idxs] = background_medians[s]`` (plotting/cond_ae_utils.py:3111), all sessions in one table."""
    latents = np.asarray(latents)
    idxs = np.asarray(background_idxs, dtype=np.int64).reshape(-1)
    medians = np.asarray(medians)
    if latents.ndim != 2:
        raise ValueError('swap_points: expected latents (T, D), got %s' % (latents.shape,))
    if medians.ndim != 2 or medians.shape[1] != len(idxs):
        raise ValueError('swap_points: expected medians (S, %d), got %s' % (len(idxs), medians.shape))
    if len(idxs) and (idxs.min() < 0 or idxs.max() >= latents.shape[1]):
        raise ValueError('swap_points: background columns %s of latents with %d' % (idxs.tolist(), latents.shape[1]))
    out = np.tile(latents[None], (medians.shape[0], 1, 1))
    out[:, :, idxs] = medians[:, None, :]
    return out.reshape(medians.shape[0] * latents.shape[0], latents.shape[1])


def swap_layout(n_sessions, sess_idx=0, layout_pattern=None):
    """Where the panels of a session-swap movie go: an int array ``(n_rows, n_cols)`` naming the session every
    position shows, -1 for a blank one (plotting/cond_ae_utils.py:3130-3152).  Session ``sess_idx``, the trial's own,
    swaps places with session 0 and so comes first.  Without a pattern fewer than four sessions stand in one row,
    four in 2 x 2, five or six in 2 x 3; a boolean ``layout_pattern`` (n_rows, n_cols) whose sum is the number of
    sessions places them at its true positions, row by row.  More than six sessions without a pattern, a pattern of
    another sum and a session outside [0, n_sessions) are ValueErrors."""
    n_sessions, sess_idx = int(n_sessions), int(sess_idx)
    if n_sessions < 1 or not 0 <= sess_idx < n_sessions:
        raise ValueError('session_swap_movie: session %d of %d' % (sess_idx, n_sessions))
    order = list(range(n_sessions))
    order[0], order[sess_idx] = order[sess_idx], order[0]
    if layout_pattern is None:
        if n_sessions > 6:
            raise ValueError('session_swap_movie: %d sessions need a layout_pattern (at most six are laid out '
                             'without one)' % n_sessions)
        n_rows, n_cols = (1, n_sessions) if n_sessions < 4 else (2, 2) if n_sessions == 4 else (2, 3)
        pattern = np.arange(n_rows * n_cols).reshape(n_rows, n_cols) < n_sessions
    else:
        pattern = np.asarray(layout_pattern).astype(bool)
        if pattern.ndim != 2 or int(pattern.sum()) != n_sessions:
            raise ValueError('session_swap_movie: layout_pattern must be a 2-d boolean array with %d true entries, '
                             'got %s with %d' % (n_sessions, pattern.shape, int(pattern.sum())))
    grid = np.full(pattern.shape, -1, dtype=np.int64)
    grid[pattern] = order
    return grid


def session_swap_movie_device(model, trials_latents, background_idxs, medians, sess_idx=0, n_buffer_frames=5,
                              layout_pattern=None, apply_inverse_transform=False, chunk_size=200):
    """The frames of the reference's ``make_session_swap_movie`` (plotting/cond_ae_utils.py:3030-3156), the MSPS-VAE's
    own picture, as a uint8 DEVICE tensor ``(sum T_i + (n_trials - 1) * n_buffer_frames, n_rows * H, n_cols * C *
    W)``: every trial of ``trials_latents`` (a list of (T_i, D) tables) re-rendered once per session with that session's
    median background latents (row ``s`` of ``medians`` (S, n_background) in the columns ``background_idxs``:
    ``swap_points``), one panel per session laid out by ``swap_layout``, every panel showing all channels of its
    frame side by side; ``n_buffer_frames`` all-zero frames separate the trials.

    A trial's ``S * T_i`` points are decoded by ``decode_points_device`` and tiled by one mosaic launch
    (``bn_frame_mosaic_ch_u8``) per ``chunk_size`` movie frames; only the movie crosses to the host.

    ``apply_inverse_transform=False`` is the reference's call: it hands the output of ``get_transformed_latents``,
    whose supervised block lies in label space, to the decoder without mapping it back.  ``True`` maps it back first,
    which is the consistent alternative."""
    medians = np.asarray(medians)
    if medians.ndim != 2:
        raise ValueError('session_swap_movie: expected medians (S, n_background), got %s' % (medians.shape,))
    grid = swap_layout(medians.shape[0], sess_idx, layout_pattern)
    n_buffer_frames, chunk_size = int(n_buffer_frames), int(chunk_size)
    if n_buffer_frames < 0 or chunk_size < 1 or len(trials_latents) < 1:
        raise ValueError('session_swap_movie: %d trials, n_buffer_frames %d, chunk_size %d'
                         % (len(trials_latents), n_buffer_frames, chunk_size))
    tables = [swap_points(z, background_idxs, medians) for z in trials_latents]
    lengths = [len(z) for z in trials_latents]
    if min(lengths) < 1:
        raise ValueError('session_swap_movie: a trial without frames (lengths %s)' % (lengths,))
    _checked_crop(model, sum(len(t) for t in tables), None, None)
    parts = []
    for i, (table, n) in enumerate(zip(tables, lengths)):
        frames = decode_points_device(model, np.ascontiguousarray(table, dtype=np.float32), None,
                                      apply_inverse_transform, chunk_size)
        n_t = n + (n_buffer_frames if i + 1 < len(tables) else 0)

        def src_of(beg, end, n=n):
            tau = np.arange(beg, end)[:, None, None]
            return np.where((grid[None] >= 0) & (tau < n), grid[None] * n + tau, -1).astype(np.int32)
        parts.append(_mosaic_in_chunks(frames, src_of, n_t, None, None, chunk_size))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def session_swap_movie(model, trials_latents, background_idxs, medians, sess_idx=0, n_buffer_frames=5,
                       layout_pattern=None, apply_inverse_transform=False, chunk_size=200):
    """``session_swap_movie_device`` as a numpy array of uint8."""
    return session_swap_movie_device(model, trials_latents, background_idxs, medians, sess_idx, n_buffer_frames,
                                     layout_pattern, apply_inverse_transform, chunk_size).cpu().numpy()


def background_medians(data_generator, model, background_idxs, min_p=15, max_p=85):
    """The median background latents of every session of ``data_generator``, ``(S, n_background)`` float32: per
    session ``latent_ranges(..., sess_idx=s, min_p, max_p)['med']`` at the columns ``background_idxs`` -- the first
    user of ``'med'``, with the reference's percentiles (plotting/cond_ae_utils.py:3079-3084).  None off rank 0."""
    idxs = np.asarray(background_idxs, dtype=np.int64).reshape(-1)
    rows = []
    for s in range(len(data_generator.datasets)):
        got = latent_ranges(data_generator, model, sess_idx=s, min_p=min_p, max_p=max_p)
        if got is None:
            return None
        rows.append(got['med'][idxs])
    return np.stack(rows)


# ------------------------------------------------------------------------------------------ reconstruction movies
def reconstruction_movie_device(model, y, sess=None, masks=None, labels=None, labels_2d=None, max_frames=400,
                                chunk_size=200, extra_models=()):
    """The frames of the reference's reconstruction movie (``make_ae_reconstruction_movie_wrapper``,
    plotting/ae_utils.py) as a uint8 DEVICE tensor ``(T, R * H, 3 * C * W)``, ``T = min(len(y), max_frames)``: per
    frame the original, the reconstruction and the residual ``0.5 + (original - reconstruction)`` next to each
    other, each panel with its channels side by side (the reference's ``concat``), clipped to [0, 1] as its
    ``imshow(vmin=0, vmax=1)`` clips and quantised by ``unit_float_to_u8``'s rule.  ``imshow(movie[t], cmap='gray',
    vmin=0, vmax=255)`` shows frame t.

    ``y``: fp32 frames or stored uint8 frames (value / 255; they go into a conv encoder as they are).  ``masks``: one
    (C, H, W) mask or per-frame masks; as in the reference they multiply the ORIGINAL alone -- the model sees the
    frames unmasked -- in its panel and inside the residual.  Every model of ``extra_models`` (the reference's
    ``include_linear``: the linear AE with the same latents) adds a row below with a black first panel, so R = 1 +
    ``len(extra_models)``.  Eval mode, ``no_grad``, the posterior mean for every variational class.

    Each chunk of ``chunk_size`` frames is one forward pass and ONE launch of ``bn_recon_panels_u8``, which reads the
    frames, the masks and the reconstruction and writes the chunk's strips into the movie; only the movie crosses to
    the host.  ``hparams['hip_encode_dtype']`` and ``['hip_decode_dtype']`` of each model are honoured: under
    ``'bf16'`` a served decoder's last layer writes uint8 grey levels (``quantising_frames``), which are the
    reconstruction panel as they are and enter the residual as value / 255.  The fp32 decoder's last bits can depend
    on the batch it is given (traversals), so ``chunk_size`` may turn a grey level there."""
    models = [model] + list(extra_models)
    for m in models:
        if m.hparams['model_class'] not in _LATENTS_AT:
            raise ValueError('Invalid model class %s' % m.hparams['model_class'])
        decode_dtype_of(m), encode_dtype_of(m)          # (an invalid key is an error before anything runs)
    who = 'reconstruction_movie'
    _check_frames(who, y)
    max_frames = int(max_frames)
    if max_frames < 0 or int(chunk_size) < 1:
        raise ValueError('%s: max_frames %d, chunk_size %d' % (who, max_frames, chunk_size))
    y = y[:max_frames].contiguous()
    n, c, h, w = (int(v) for v in y.shape)
    if masks is not None:
        # one (C, H, W) mask per trial, or per-frame masks (models.aes.frame_masks) for at least the movie's frames
        if tuple(masks.shape[-3:]) != (c, h, w) or masks.dim() not in (3, 4) or \
                (masks.dim() == 4 and masks.shape[0] != 1 and masks.shape[0] < n):
            raise ValueError('%s: expected masks %s or (T, %d, %d, %d), got %s'
                             % (who, (c, h, w), c, h, w, tuple(masks.shape)))
        masks = masks[:n] if masks.dim() == 4 and masks.shape[0] > n else masks
    masks, per_frame = _trial_masks(masks, y)
    labels = None if labels is None else labels[:max_frames]
    labels_2d = None if labels_2d is None else labels_2d[:max_frames]
    out = torch.empty((n, len(models) * h, 3 * c * w), dtype=torch.uint8, device=y.device)
    floats = None          # (the fp32 copy of stored frames, made once for the models that need it)
    for row, m in enumerate(models):
        def panels(beg, end, x_hat, req):
            recon = req.frames if req.frames is not None else x_hat
            recon = recon.contiguous().view(y[beg:end].shape)
            _hip.recon_panels_u8(y[beg:end], recon, masks[beg:end] if per_frame else masks, show_orig=row == 0,
                                 out=out[beg:end], row=row, n_rows=len(models))

        x = _model_frames(m, y, labels_2d, floats)
        floats = floats if x is y else x
        with encode_precision(encode_dtype_of(m)), decode_precision(decode_dtype_of(m)):
            _forward_chunks(who, m, y, sess, labels, labels_2d, chunk_size, panels,
                            lambda beg, end: quantising_frames(), x)
    return out


def reconstruction_movie(model, y, sess=None, masks=None, labels=None, labels_2d=None, max_frames=400, chunk_size=200,
                         extra_models=()):
    """``reconstruction_movie_device`` as a numpy array ``(T, R * H, 3 * C * W)`` of uint8."""
    return reconstruction_movie_device(model, y, sess, masks, labels, labels_2d, max_frames, chunk_size,
                                       extra_models).cpu().numpy()


# ------------------------------------------------------------------------------------------ ranges
def percentile_plan(n_valid, ps, dtype=np.float32):
    """Where ``np.nanpercentile(values, p, axis=0)`` of ``dtype`` values reads a column of ``n_valid[j]`` non-NaN
    values, for every ``p`` of ``ps``: ``(ranks, gammas)`` with ``ranks`` int64 ``(2 len(ps), D)`` -- rows 2 i and
    2 i + 1 are the zero-based ranks ``lo`` and ``hi`` of ``ps[i]`` among the column's sorted valid values -- and
    ``gammas`` of ``dtype``, ``(len(ps), D)``, the weight between them.  numpy's own float arithmetic (2.2: the
    'linear' method on float32 data with a Python-scalar percentile), restated:

        q = p / dtype(100);  vi = dtype(m - 1) * q;  lo = floor(vi), hi = lo + 1, both m - 1 where vi >= m - 1;
        gamma = vi - floor(vi)

    An empty column (``m == 0``) gets rank -1, which the selection answers with NaN as ``nanpercentile`` does."""
    m = np.asarray(n_valid, dtype=np.int64).reshape(-1)
    ps = [ps] if np.isscalar(ps) else list(ps)
    ranks = np.empty((2 * len(ps), m.size), dtype=np.int64)
    gammas = np.empty((len(ps), m.size), dtype=dtype)
    top = np.maximum(m - 1, 0)
    top_f = top.astype(dtype)
    for i, p in enumerate(ps):
        q = np.true_divide(p, dtype(100))
        vi = top_f * q
        fl = np.floor(vi)
        lo = np.minimum(fl.astype(np.int64), top)
        hi = np.minimum(lo + 1, top)
        above = vi >= top_f
        lo[above] = top[above]
        hi[above] = top[above]
        ranks[2 * i] = np.where(m > 0, lo, -1)
        ranks[2 * i + 1] = np.where(m > 0, hi, -1)
        gammas[i] = vi - fl
    return ranks, gammas


def percentile_lerp(lo, hi, gammas):
    """numpy's interpolation between the two selected neighbours, in their dtype: with ``diff = hi - lo``,
    ``lo + diff * g`` where ``g < 0.5`` and ``hi - diff * (1 - g)`` elsewhere (``np.lib._function_base_impl._lerp``).
    Two equal infinities give NaN, as they do there."""
    lo, hi, g = np.asarray(lo), np.asarray(hi), np.asarray(gammas)
    with np.errstate(invalid='ignore', over='ignore'):
        diff = hi - lo
        out = lo + diff * g
        upper = hi - diff * (1 - g)
    return np.where(g >= 0.5, upper, out).astype(lo.dtype, copy=False)


def column_percentiles(table, ps):
    """``np.nanpercentile(table, p, axis=0)`` for every ``p`` of ``ps`` (at most four) on a float32 DEVICE table
    ``(n, D)``, as a float32 numpy array ``(len(ps), D)`` with numpy's bits: ONE ``bn_column_count`` for the columns'
    valid counts (D integers to the host), the ranks named on the host (``percentile_plan``), ONE ``bn_column_select``
    for both neighbours of every percentile, and numpy's float32 interpolation of the ``2 len(ps) D`` selected values
    (``percentile_lerp``).  The table stays on the device and is not changed."""
    ps = list(ps)
    n_valid = _hip.column_count(table).cpu().numpy()
    ranks, gammas = percentile_plan(n_valid, ps)
    sel = _hip.column_select(table, torch.from_numpy(ranks).to(table.device)).cpu().numpy()
    return percentile_lerp(sel[0::2], sel[1::2], gammas)


def _table_ranges(table, min_p, max_p):
    got = column_percentiles(table, (min_p, max_p, 50))
    return {'min': got[0], 'max': got[1], 'med': got[2]}


def _ranges_device():
    return torch.device('cuda', torch.cuda.current_device())


def stack_for_ranges(values_list, device=None):
    """The entries of ``values_list`` -- numpy arrays or tensors ``(n_i, D)``, entries of length 0 skipped as the
    reference's ``compute_range`` skips the gap trials of a latents pickle -- as ONE float32 device table: numpy
    entries are stacked on the host and uploaded once, device entries concatenated where they are."""
    kept = [v for v in values_list if len(v) != 0]
    if not kept:
        raise ValueError('compute_range: no values (every entry of values_list is empty)')
    for v in kept:
        if np.ndim(v) != 2 or v.shape[1] != kept[0].shape[1]:
            raise ValueError('compute_range: expected entries (n_i, %d), got %s'
                             % (kept[0].shape[1] if np.ndim(kept[0]) == 2 else -1, tuple(np.shape(v))))
    tensors = [v for v in kept if torch.is_tensor(v)]
    if device is None:
        on_device = [t.device for t in tensors if t.is_cuda]
        device = on_device[0] if on_device else _ranges_device()
    parts = []
    host = [np.asarray(v, dtype=np.float32) for v in kept if not torch.is_tensor(v)]
    if host:
        parts.append(torch.from_numpy(np.ascontiguousarray(np.vstack(host))).to(device))
    parts.extend(t.detach().to(device=device, dtype=torch.float32) for t in tensors)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def compute_range(values_list, min_p=5, max_p=95):
    """``plotting.cond_ae_utils.compute_range``: see there."""
    return _table_ranges(stack_for_ranges(values_list), min_p, max_p)


def _wanted_sessions(who, data_generator, sess_idx):
    """The sessions ``sess_idx`` names -- one index, a list, or None for all -- as a set."""
    n_sess = len(data_generator.datasets)
    if sess_idx is None:
        wanted = set(range(n_sess))
    elif isinstance(sess_idx, (list, tuple, np.ndarray)):
        wanted = set(int(s) for s in sess_idx)
    else:
        wanted = {int(sess_idx)}
    if not wanted or min(wanted) < 0 or max(wanted) >= n_sess:
        raise ValueError('%s: sessions %s of a generator with %d' % (who, sorted(wanted), n_sess))
    return wanted


def _latent_trials(who, data_generator, model, dtypes, wanted, per_trial=None, keep_empty=False, upload=True):
    """``{(session, int(trial)): fp32 device tensor (T, D)}`` of the trials of the splits ``dtypes`` of the sessions
    ``wanted``, in walk order: the latents, walked and encoded as ``export_latents`` walks and encodes them (the same
    per-trial encoder and batch fields; trials served on the host go through ``encode_trial`` and are uploaded to the
    model's device one by one -- or, with ``upload=False``, stay the numpy arrays they are for a caller that uploads
    them at once).  The one-process sink form of the trial walk: the caller runs it on ONE rank.  A trial without
    rows is left out unless ``keep_empty``.  ``per_trial(sess, trial, z, data)`` sees every kept trial with its batch
    as soon as it is encoded; what it raises ends the walk there."""
    device = next(model.parameters()).device
    encode = _GraphedTrialEncoder(model)
    parts = {}

    def on_device(images, sess, data, trial):
        if sess not in wanted:
            return None
        return encode(images, sess, _batch_fields(model, data)[2]).to(torch.float32), data

    def on_host(images, sess, data, trial):
        if sess not in wanted:
            return None
        z = encode_trial(model, images, sess, _batch_fields(model, data)[2])
        return (torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(device) if upload else z), data

    def sink(sess, trial, result):
        if result is not None and (keep_empty or len(result[0])):
            if per_trial is not None:
                per_trial(sess, int(trial), *result)
            parts[(sess, int(trial))] = result[0]
    _export_per_trial(who, data_generator, model, on_device, on_host, sink=sink, dtypes=dtypes)
    return parts


def _parts_table(parts, data_generator, dtypes, wanted, cols):
    """``(keys, table)``: the trials of ``parts`` (``_latent_trials``) that lie in the splits ``dtypes`` of the sessions
    ``wanted``, in ``_corr_trial_order`` -- the generator serves the trials in its own order, the table is put together
    in the reference's -- and their columns ``cols`` (``_corr_columns``: a range is read in place, an index array is
    gathered once on the device) as one table; None without trials."""
    keys = [k for k in _corr_trial_order([ds.batch_idxs for ds in data_generator.datasets], dtypes, wanted)
            if k in parts]
    if not keys:
        return keys, None
    table = torch.cat([parts[k] for k in keys], dim=0)
    if isinstance(cols, tuple):
        return keys, table[:, cols[0]:cols[1]]
    return keys, table[:, torch.from_numpy(cols).to(table.device)]


def _latent_table(data_generator, model, sess_idx):
    """The latents of every train / val / test trial of the sessions ``sess_idx`` as ONE device table, encoded as
    ``export_latents`` encodes them; None on the ranks other than 0."""
    _export_setup(model)
    if bdist.world_size() > 1 and bdist.rank() != 0:
        return None
    wanted = _wanted_sessions('latent_ranges', data_generator, sess_idx)
    # (trials encoded on the host stay there: ``stack_for_ranges`` uploads them once, not one by one)
    parts = _latent_trials('latent_ranges', data_generator, model, ('train', 'val', 'test'), wanted, upload=False)
    if not parts:
        raise ValueError('latent_ranges: the sessions %s have no train, val or test trial' % sorted(wanted))
    return stack_for_ranges(list(parts.values()), device=next(model.parameters()).device)


def latent_ranges(data_generator, model, sess_idx=None, min_p=5, max_p=95):
    """The ranges of a model's latents, ``{'min', 'max', 'med'}`` as ``(D,)`` float32 arrays: the ``min_p``-th,
    ``max_p``-th and 50th percentile per latent over every frame of every train / val / test trial of the sessions
    ``sess_idx`` (one index, a list, or None for all) -- what the reference's ``get_input_range('latents', ...)``
    computes from a latents pickle (``compute_range``, plotting/cond_ae_utils.py:148-178) and hands to its traversals
    as ``mins`` and ``maxes``.

    The trials are walked and encoded as ``export_latents`` walks and encodes them (the same per-trial encoder and
    batch fields, so the latents have its bits; ``hparams['hip_encode_dtype']`` is honoured), but they stay in one
    device table and the percentiles are selected there (``column_percentiles``): the counts and the selected
    neighbours are all that crosses to the host.

    Under ``torch.distributed`` order statistics do not combine across ranks the way sums do: rank 0 alone walks
    every trial (the one-process sink form of the trial walk, no collective is entered) and the other ranks return
    None at once."""
    table = _latent_table(data_generator, model, sess_idx)
    return None if table is None else _table_ranges(table, min_p, max_p)


def latent_ranges_device(data_generator, model, sess_idx=None, min_p=5, max_p=95):
    """``latent_ranges`` as a float32 DEVICE tensor ``(3, D)``: the rows min, max, med (None off rank 0)."""
    table = _latent_table(data_generator, model, sess_idx)
    if table is None:
        return None
    return torch.from_numpy(column_percentiles(table, (min_p, max_p, 50))).to(table.device)


# ------------------------------------------------------------------------------------------ label scores
LABEL_R2_CLASSES = ('ps-vae', 'msps-vae', 'cond-ae-msp')          # the classes with a supervised block of latents
LABEL_R2_MODEL = 'MSPS-VAE'          # the 'Model' column of r2_supervised.csv: the reference's literal, for every class


def _check_label_r2_class(who, model_class):
    if model_class not in LABEL_R2_CLASSES:
        raise ValueError('%s: model class %r has no supervised latents (label scores are served for %s)'
                         % (who, model_class, ', '.join(LABEL_R2_CLASSES)))


def _scores_from_sums(n, sy, syy, sd):
    """``(r2, mse, ss_tot)`` from the four sums, elementwise in float64: ``mse = sd / n``, ``ss_tot = syy - sy^2 / n``,
    ``r2 = 1 - sd / ss_tot``; where ``ss_tot`` is zero sklearn's rule for a constant ``y_true`` holds (1.0 for a
    perfect prediction, else 0.0).  ``ss_tot`` is a difference of two sums that each carry a rounding error of up to
    ``n 2^-53`` of their size, so a value within ``8 n 2^-53 syy`` of zero IS zero as far as the sums can tell (a
    column that is constant over its valid entries lands there, exactly zero only when its sums happen to be exact)
    and is set to it.  Entries without a valid value are NaN."""
    with np.errstate(divide='ignore', invalid='ignore'):
        mse = sd / n
        ss_tot = syy - sy * sy / n
        ss_tot = np.where(np.abs(ss_tot) <= 8.0 * n * 2.0 ** -53 * np.abs(syy), 0.0, ss_tot)
        r2 = 1.0 - sd / ss_tot
    r2 = np.where(ss_tot == 0, np.where(sd == 0, 1.0, 0.0), r2)
    # (a NaN among the valid entries stays one: ss_tot == 0 and sd == 0 are both False for it)
    r2 = np.where(np.isnan(ss_tot) | np.isnan(sd), np.nan, r2)
    empty = n == 0
    return np.where(empty, np.nan, r2), np.where(empty, np.nan, mse), np.where(empty, np.nan, ss_tot)


def summarise_label_sums(sums, min_valid=10):
    """Label scores from the sums ``bn_segment_label_sums`` returns, ``(S, L, 4)`` = per segment and label the count,
    ``sum y``, ``sum y^2`` and ``sum (y - y_hat)^2`` of the valid entries, in numpy float64 on the host:

    ``{'n', 'r2', 'mse'}``, each ``(S, L)`` -- what the reference's ``get_label_r2`` computes per trial and label with
    ``sklearn.metrics.r2_score`` and ``np.mean(np.square(...))`` (cond_ae_utils.py:1257-1265), ``r2`` and ``mse`` NaN
    where ``n <= min_valid`` as there (``len(y_true) > 10``) -- and ``'pooled'``, from the sums added over the segments
    and regardless of ``min_valid``: ``{'n', 'r2', 'mse'}`` per label ``(L,)`` and the scalar
    ``'r2_variance_weighted'``, sklearn's variance-weighted R^2 over the labels, ``1 - sum_j sd_j / sum_j ss_tot_j``
    (labels with ``ss_tot == 0`` weigh nothing; all of them so: the plain mean) -- the quantity the training step logs
    as ``label_r2`` (``models.vaes._r2_variance_weighted``)."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[2] != 4:
        raise ValueError('summarise_label_sums: expected sums (S, L, 4), got %s' % (tuple(sums.shape),))
    n = sums[..., 0]
    r2, mse, _ = _scores_from_sums(n, sums[..., 1], sums[..., 2], sums[..., 3])
    few = n <= min_valid
    out = {'n': n.astype(np.int64), 'r2': np.where(few, np.nan, r2), 'mse': np.where(few, np.nan, mse)}
    tot = sums.sum(axis=0)
    p_r2, p_mse, p_ss = _scores_from_sums(tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 3])
    scored = tot[:, 0] > 0
    if not scored.any():
        weighted = np.nan
    elif np.any(p_ss[scored] != 0):
        weighted = float(np.average(p_r2[scored], weights=p_ss[scored]))
    else:
        weighted = float(np.mean(p_r2[scored]))
    out['pooled'] = {'n': tot[:, 0].astype(np.int64), 'r2': p_r2, 'mse': p_mse, 'r2_variance_weighted': weighted}
    return out


def _splits(who, dtype):
    dtypes = [dtype] if isinstance(dtype, str) else list(dtype)
    if not dtypes or any(d not in ('train', 'val', 'test') for d in dtypes) or len(set(dtypes)) != len(dtypes):
        raise ValueError("%s: dtype must be 'train', 'val' or 'test' or a list of them, got %r" % (who, dtype))
    return dtypes


def label_r2(data_generator, model, dtype='val', sess_idx=None):
    """How well a model's supervised latents reconstruct each label, per trial and label: the numbers of the
    reference's ``get_label_r2`` (plotting/cond_ae_utils.py:1234-1279) for a ``ps-vae``, ``msps-vae`` or
    ``cond-ae-msp`` model (any other class: ValueError) over the trials of the split ``dtype`` -- or a list of splits;
    the trials of other splits are not read -- of the sessions ``sess_idx`` (one index, a list, or None for all).

    The trials are walked and encoded as ``export_latents`` walks and encodes them (the same per-trial encoder and
    batch fields; ``hparams['hip_encode_dtype']`` is honoured; host-resident generators go through ``encode_trial``).
    A trial's prediction is the first ``n_labels`` columns of its latents in the transformed space -- what the
    reference's ``get_transformed_latents(images)`` returns: for ``ps-vae`` / ``msps-vae``
    ``model.get_transformed_latents(latents, as_numpy=False)`` (the label map ``D`` on the supervised block), for
    ``cond-ae-msp`` the encoded latents as they are, since the trial encoder has applied ``U`` already (as
    ``export_latents`` does for that class) and a second ``U`` would score other numbers.  Predictions,
    ``labels`` and ``labels_masks`` (where the batches have them) stay on the device in three tables with one offsets
    vector, ONE ``bn_segment_label_sums`` launch reduces all trials, and ``(S, L, 4)`` doubles cross to the host.

    -> ``summarise_label_sums``'s dict (``'n'``, ``'r2'``, ``'mse'`` as ``(S, L)``, ``'pooled'``) plus ``'session'`` and
    ``'trial'``, int arrays ``(S,)`` in walk order, and ``'sums'`` ``(S, L, 4)``.  Under ``torch.distributed`` rank 0
    walks every trial and the other ranks return None, as ``latent_ranges`` does."""
    _check_label_r2_class('label_r2', model.hparams['model_class'])
    dtypes = _splits('label_r2', dtype)
    _export_setup(model)
    if bdist.world_size() > 1 and bdist.rank() != 0:
        return None
    wanted = _wanted_sessions('label_r2', data_generator, sess_idx)
    n_labels = int(model.hparams['n_labels'])
    device = next(model.parameters()).device
    # (the trial encoder returns U z for an AE-MSP, ``_encode_trial_device``: the transformed space already)
    transformed = model.hparams['model_class'] == 'cond-ae-msp'
    preds, truths, masks, sessions, trials = [], [], [], [], []

    def table(value):
        value = value[0]
        return (value if torch.is_tensor(value) else torch.from_numpy(np.asarray(value))).to(device, torch.float32)

    def per_trial(sess, trial, z, data):
        if 'labels' not in data:
            raise ValueError('label_r2: the generator serves no labels (session %d, trial %d)' % (sess, trial))
        if transformed:
            pred = z
        else:
            with torch.no_grad():
                pred = model.get_transformed_latents(z, as_numpy=False)
        truth = table(data['labels'])
        if truth.dim() != 2 or truth.shape != (pred.shape[0], n_labels):
            raise ValueError('label_r2: labels %s for %d frames and %d labels (session %d, trial %d)'
                             % (tuple(truth.shape), pred.shape[0], n_labels, sess, trial))
        preds.append(pred)
        truths.append(truth)
        masks.append(table(data['labels_masks']) if 'labels_masks' in data else None)
        sessions.append(sess)
        trials.append(trial)
    _latent_trials('label_r2', data_generator, model, dtypes, wanted, per_trial=per_trial, keep_empty=True)
    if not preds:
        raise ValueError('label_r2: the sessions %s have no %s trial' % (sorted(wanted), ' or '.join(dtypes)))
    offsets = np.concatenate(([0], np.cumsum([p.shape[0] for p in preds]))).astype(np.int64)
    pred = torch.cat(preds, dim=0)
    mask = None
    if any(m is not None for m in masks):
        mask = torch.cat([torch.ones_like(t) if m is None else m for m, t in zip(masks, truths)], dim=0)
    sums = _hip.segment_label_sums(pred[:, :n_labels], torch.cat(truths, dim=0), mask, offsets).cpu().numpy()
    out = summarise_label_sums(sums)
    out.update({'session': np.asarray(sessions, dtype=np.int64), 'trial': np.asarray(trials, dtype=np.int64),
                'sums': sums})
    return out


def export_label_r2(data_generator, model, label_names=None, dtype='val', filename=None):
    """``label_r2`` as the table the reference's ``get_label_r2`` saves and its hyperparameter searches read:
    ``r2_supervised.csv`` in the model's version directory (or ``filename``), one row per (trial, label) in walk order
    with the reference's columns in its order -- ``Trial, Label, R2, MSE, Model``, the last one its literal string --
    and one trailing column ``Session``, the session's index (the reference's table cannot tell two sessions' trials
    apart).  ``label_names`` defaults to ``label_0, label_1, ...``; a NaN is an empty field, as pandas writes it.
    Written with the ``csv`` module.  -> the path (None on the ranks other than 0)."""
    scores = label_r2(data_generator, model, dtype=dtype)
    if scores is None:
        return None
    n_labels = scores['r2'].shape[1]
    if label_names is None:
        label_names = ['label_%i' % i for i in range(n_labels)]
    if len(label_names) != n_labels:
        raise ValueError('export_label_r2: %d label names for %d labels' % (len(label_names), n_labels))
    if filename is None:
        filename = _version_path(model, 'r2_supervised.csv')
    return _write_csv(filename, ['Trial', 'Label', 'R2', 'MSE', 'Model', 'Session'],
                      ([int(trial), name, scores['r2'][k, i], scores['mse'][k, i], LABEL_R2_MODEL, int(sess)]
                       for k, (sess, trial) in enumerate(zip(scores['session'], scores['trial']))
                       for i, name in enumerate(label_names)))


# ------------------------------------------------------------------------------------------ latent correlations
LATENT_CORR_MAX_COLUMNS = 64


def _moments_from_gram(A, shift):
    """``{'n', 'mean', 'cov', 'corr', 'mean_abs_offdiag'}`` from augmented moment matrices ``(..., D + 1, D + 1)``."""
    n = A[..., 0, 0]
    s = A[..., 0, 1:]
    G = A[..., 1:, 1:]
    D = s.shape[-1]
    nn = n[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = s / nn + (0.0 if shift is None else shift)
        ss = G - s[..., :, None] * s[..., None, :] / nn[..., None]          # the centred sums of products
        cov = ss / (nn[..., None] - 1.0)
        gd = np.diagonal(G, axis1=-2, axis2=-1)
        sd = np.diagonal(ss, axis1=-2, axis2=-1)
        # a centred sum of squares within the rounding noise of the two sums it is the difference of: the column is
        # constant as far as the sums can tell (the rule of _scores_from_sums)
        flat = np.abs(sd) <= 8.0 * nn * 2.0 ** -53 * np.abs(gd)
        var = np.where(flat | (nn < 2), np.nan, sd)
        corr = ss / np.sqrt(var[..., :, None] * var[..., None, :])
    few = np.broadcast_to((nn < 2)[..., None], cov.shape)
    cov = np.where(few, np.nan, cov)
    mean = np.where(np.broadcast_to(nn < 1, mean.shape), np.nan, mean)
    corr = np.clip(corr, -1.0, 1.0)
    if D > 1:
        iu = np.triu_indices(D, 1)
        offdiag = np.abs(corr[..., iu[0], iu[1]]).mean(axis=-1)
    else:
        offdiag = np.full(n.shape, np.nan)
    return {'n': n.astype(np.int64), 'mean': mean, 'cov': cov, 'corr': corr, 'mean_abs_offdiag': offdiag}


def summarise_gram(A, shift=None):
    """Means, covariances and correlations from the matrices ``bn_segment_gram`` returns, ``(S, D + 1, D + 1)`` = per
    segment the sum of ``a^T a`` with ``a = (1, z - shift)``, in numpy float64 on the host:

    ``'n' (S,)``; ``'mean' (S, D)`` = ``shift + s / n``; ``'cov' (S, D, D)`` = ``(G - s s^T / n) / (n - 1)``, ``ddof = 1``
    as ``np.cov``; ``'corr' (S, D, D)``, ``cov`` normalised by its diagonal and clipped to [-1, 1] as ``np.corrcoef``
    does; ``'mean_abs_offdiag' (S,)``, the mean of ``|corr|`` over the pairs ``i < j`` (NaN for D = 1) -- the "average
    over all pairs" the reference's docstring promises; and ``'pooled'``, the same keys without the segment axis from
    the matrices added over the segments (all segments share the one shift, so their matrices add).

    With ``n < 2``, or for a column whose centred sum of squares is within ``8 n 2^-53`` of its raw one -- rounding
    noise of the sums: a column that is constant as far as they can tell --, the entries of ``corr`` that involve the
    column are NaN (``np.corrcoef`` divides zero by zero there)."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 3 or A.shape[1] != A.shape[2] or A.shape[1] < 2:
        raise ValueError('summarise_gram: expected matrices (S, D + 1, D + 1), got %s' % (tuple(A.shape),))
    if shift is not None:
        shift = np.asarray(shift, dtype=np.float64)
        if shift.shape != (A.shape[1] - 1,):
            raise ValueError('summarise_gram: %d columns, shift %s' % (A.shape[1] - 1, tuple(shift.shape)))
    out = _moments_from_gram(A, shift)
    out['pooled'] = _moments_from_gram(A.sum(axis=0), shift)
    return out


def _corr_columns(who, hparams, n_latents, columns):
    """The columns ``latent_correlations`` reads -> ``(start, stop)`` for a contiguous ascending range (served without
    a copy) or an int64 index array.  None: the unsupervised block of the model class."""
    if columns is None:
        model_class = hparams['model_class']
        first = 0
        if model_class in ('ps-vae', 'msps-vae'):
            first = int(hparams['n_labels'])
        if model_class == 'msps-vae':
            first += int(hparams['n_background'])
        columns = slice(first, n_latents)
    if isinstance(columns, slice):
        if columns.step not in (None, 1):
            columns = np.arange(n_latents)[columns]
        else:
            start, stop, _ = columns.indices(n_latents)
            columns = np.arange(start, stop)
    idx = np.asarray(columns)
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in 'iu':
        raise ValueError('%s: columns must name at least one latent of %d by index, got %r' % (who, n_latents, columns))
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx.max() >= n_latents:
        raise ValueError('%s: columns %s of a model with %d latents' % (who, idx.tolist(), n_latents))
    if idx.size > LATENT_CORR_MAX_COLUMNS:
        raise ValueError('%s: %d columns (1 to %d are served)' % (who, idx.size, LATENT_CORR_MAX_COLUMNS))
    if np.array_equal(idx, np.arange(idx[0], idx[0] + idx.size)):
        return int(idx[0]), int(idx[0]) + int(idx.size)
    return idx


def _corr_trial_order(batch_idxs, dtypes, wanted):
    """``[(session, trial)]`` in the order the reference's ``np.vstack`` of ``load_latents(..., dtype)`` stacks the
    rows: sessions ascending, and within a session the trials of each split in turn, in ``batch_idxs[dtype]`` order.
    ``batch_idxs``: one dict a session."""
    return [(s, int(t)) for s, idxs in enumerate(batch_idxs) if s in wanted for dt in dtypes for t in idxs[dt]]


def _corr_segments(who, keys, lengths, segments):
    """Offsets of the segments over the pooled table whose trials ``keys`` = ``[(session, trial)]`` hold ``lengths``
    rows each -> ``(offsets int64 (S + 1,), session, trial)``; the last two are int64 ``(S,)`` arrays for ``'trial'``
    (both) and ``'session'`` (the first) and None otherwise.  None: one segment over everything; an int ``b``:
    consecutive batches of ``b`` rows, across trial and session boundaries, the last one ragged."""
    ends = np.cumsum(np.asarray(lengths, dtype=np.int64))
    total = int(ends[-1]) if len(ends) else 0
    sessions = np.asarray([k[0] for k in keys], dtype=np.int64)
    if segments is None:
        return np.asarray([0, total], dtype=np.int64), None, None
    if isinstance(segments, (int, np.integer)) and not isinstance(segments, bool):
        if segments < 1:
            raise ValueError('%s: batches of %d rows' % (who, segments))
        b = int(segments)
        return np.minimum(np.arange(-(-total // b) + 1, dtype=np.int64) * b, total), None, None
    if isinstance(segments, str) and segments == 'trial':
        return np.concatenate(([0], ends)).astype(np.int64), sessions, np.asarray([k[1] for k in keys], dtype=np.int64)
    if isinstance(segments, str) and segments == 'session':
        present = np.unique(sessions)
        last = np.asarray([ends[np.nonzero(sessions == s)[0][-1]] for s in present], dtype=np.int64)
        return np.concatenate(([0], last)).astype(np.int64), present.astype(np.int64), None
    raise ValueError("%s: segments must be None, a batch size, 'trial' or 'session', got %r" % (who, segments))


def latent_correlations(data_generator, model, dtype='train', sess_idx=None, segments=None, columns=None):
    """Mean, covariance and correlation matrix of a model's latents per batch, trial or session or over all time
    points: the third number the reference's PS-VAE and MSPS-VAE hyperparameter searches read next to pixel MSE and
    label R^2 (plotting/cond_ae_utils.py:1679-1700, 2802-2835: the latents pickles of every session stacked on the
    host and ``np.corrcoef`` once per ``batch_size`` rows).

    The trials of the split ``dtype`` (or a list of splits) of the sessions ``sess_idx`` (one index, a list, or None
    for all) are walked and encoded as ``export_latents`` walks and encodes them (``hparams['hip_encode_dtype']`` is
    honoured; host-resident generators go through ``encode_trial``) and put into ONE device table in the order of the
    reference's stack: sessions ascending, within a session the trials in ``batch_idxs[dtype]`` order, split after
    split.  ``segments``: None (one segment over everything, the reference's ``batch_size=None``), an int ``b``
    (consecutive batches of ``b`` rows of that table, across trial and session boundaries as the reference's, the last
    one ragged), ``'trial'`` or ``'session'``.  ``columns``: a slice or a list of latent indices, 64 at most; by
    default the unsupervised block (from ``n_labels`` on for ``ps-vae``, from ``n_labels + n_background`` on for
    ``msps-vae``, every latent otherwise).  A contiguous range is read in place, any other list is gathered once on the
    device.  The shift is the first row of the selected table, taken on the device.  ONE ``bn_segment_gram`` launch
    reduces all segments; ``(S, D + 1, D + 1)`` doubles and the D shift values cross to the host.

    -> ``summarise_gram``'s dict plus ``'gram'``, ``'shift'``, ``'rows' (S, 2)`` (begin and end row of each segment),
    ``'abs_corr_01' (S,)`` = ``|corr[0, 1]|``, the number the reference plots (NaN for fewer than two columns), and for
    ``'trial'`` / ``'session'`` segments the int arrays ``'session'`` (and ``'trial'``).  Under ``torch.distributed``
    rank 0 walks every trial and the other ranks return None, as ``label_r2`` does."""
    who = 'latent_correlations'
    dtypes = _splits(who, dtype)
    cols = _corr_columns(who, model.hparams, int(model.hparams['n_ae_latents']), columns)
    _corr_segments(who, [], [], segments)          # (a bad value: an error before the walk)
    _export_setup(model)
    if bdist.world_size() > 1 and bdist.rank() != 0:
        return None
    wanted = _wanted_sessions(who, data_generator, sess_idx)
    parts = _latent_trials(who, data_generator, model, dtypes, wanted)
    keys, selected = _parts_table(parts, data_generator, dtypes, wanted, cols)
    if not keys:
        raise ValueError('%s: the sessions %s have no %s trial' % (who, sorted(wanted), ' or '.join(dtypes)))
    offsets, sessions, trials = _corr_segments(who, keys, [parts[k].shape[0] for k in keys], segments)
    shift = selected[0].contiguous()
    gram = _hip.segment_gram(selected, offsets, shift)
    host = torch.cat([gram.reshape(-1), shift.to(torch.float64)]).cpu().numpy()          # one transfer
    D = selected.shape[1]
    gram, shift = host[:host.size - D].reshape(len(offsets) - 1, D + 1, D + 1), host[host.size - D:]
    out = summarise_gram(gram, shift)
    out.update({'gram': gram, 'shift': shift, 'rows': np.stack([offsets[:-1], offsets[1:]], axis=1),
                'abs_corr_01': np.abs(out['corr'][:, 0, 1]) if D > 1 else np.full(len(offsets) - 1, np.nan)})
    if sessions is not None:
        out['session'] = sessions
    if trials is not None:
        out['trial'] = trials
    return out


def _write_latent_corr_csv(filename, scores):
    return _write_csv(filename, ['Segment', 'RowBegin', 'RowEnd', 'N', 'AbsCorr01', 'MeanAbsCorr'],
                      ([k, int(begin), int(end), int(scores['n'][k]), scores['abs_corr_01'][k],
                        scores['mean_abs_offdiag'][k]] for k, (begin, end) in enumerate(scores['rows'])))


def export_latent_correlations(data_generator, model, dtype='train', segments=None, columns=None, filename=None):
    """``latent_correlations`` as a table: ``corr_unsupervised.csv`` in the model's version directory (or
    ``filename``), one row per segment with the columns ``Segment, RowBegin, RowEnd, N, AbsCorr01, MeanAbsCorr`` --
    ``AbsCorr01`` the reference's ``|corr[0, 1]|`` of the first two selected columns, ``MeanAbsCorr`` the mean of
    ``|corr|`` over all pairs.  Written with the ``csv`` module, ``repr(float)`` fields, a NaN an empty field.
    -> the path (None on the ranks other than 0)."""
    scores = latent_correlations(data_generator, model, dtype=dtype, segments=segments, columns=columns)
    if scores is None:
        return None
    if filename is None:
        filename = _version_path(model, 'corr_unsupervised.csv')
    return _write_latent_corr_csv(filename, scores)


# ------------------------------------------------------------------------------------------ session classifier
SESSION_CLASSIFIER_FILE = 'fc_session_classification.npy'


def _check_session_classifier(who, data_generator, sess_idx=None):
    """The sessions to tell apart, ascending; fewer than two, or more than the kernel's eight: ValueError."""
    wanted = sorted(_wanted_sessions(who, data_generator, sess_idx))
    if len(wanted) < 2:
        raise ValueError('%s: %d session (a session classifier needs at least two)' % (who, len(wanted)))
    if len(wanted) > _hip.SOFTMAX_CV_MAX_S:
        raise ValueError('%s: %d sessions (2 to %d are served)' % (who, len(wanted), _hip.SOFTMAX_CV_MAX_S))
    return wanted


def session_classifier(data_generator, model, dtype='val', columns=None, Cs=_clf.DEFAULT_CS, n_splits=5, tol=1e-4,
                       max_iter=100, sess_idx=None):
    """``fc``, the fraction of the ``dtype`` frames whose session a linear classifier recovers from the latents, and
    the classifier: the fourth number the reference's MSPS-VAE hyperparameter search reads (``fit_classifier``,
    plotting/cond_ae_utils.py:1282-1369: ``LogisticRegressionCV(Cs=<8 values>, cv=5, penalty='l2',
    multi_class='multinomial')`` on the host copy of every training frame, then ``accuracy_score`` on ``dtype``).

    The ``'train'`` trials and the ``dtype`` trials of the sessions ``sess_idx`` (a list, or None for all; at least two)
    are walked and encoded as ``latent_correlations`` walks and encodes them and put into two device tables in its
    order; ``columns`` are its columns (default: the unsupervised block of ``ps-vae`` / ``msps-vae``, every latent
    otherwise).  The class of a row is the index of its session among the selected ones; the folds are sklearn's
    unshuffled ``StratifiedKFold(n_splits)`` of that order (``fitting.classifier.stratified_folds``).  The
    ``n_splits x len(Cs)`` models are fitted in lockstep (``fitting.classifier.cross_validate``): an iteration is
    one ``bn_softmax_cv_lossgrad`` launch over the training table for all models and one transfer of
    ``M (S (D + 1) + 2)`` doubles; ``bn_softmax_cv_score`` scores them on their held-out folds and the refitted model
    on the ``dtype`` table.  ``tol`` bounds ``||dF||_inf`` of sklearn's objective; ``max_iter`` the accepted steps.

    -> ``(fc, SessionClassifier)``; under ``torch.distributed`` rank 0 walks every trial and the other ranks return
    None, as ``label_r2`` does."""
    who = 'session_classifier'
    splits = _splits(who, dtype)
    if len(splits) != 1:
        raise ValueError("%s: dtype must be 'train', 'val' or 'test', got %r" % (who, dtype))
    cols = _corr_columns(who, model.hparams, int(model.hparams['n_ae_latents']), columns)
    wanted = _check_session_classifier(who, data_generator, sess_idx)
    if n_splits < 2 or n_splits * len(Cs) > _hip.SOFTMAX_CV_MAX_M:
        raise ValueError('%s: %d folds x %d values of C (2 folds at least, %d models a launch at most)'
                         % (who, n_splits, len(Cs), _hip.SOFTMAX_CV_MAX_M))
    _export_setup(model)
    if bdist.world_size() > 1 and bdist.rank() != 0:
        return None
    dtypes = ['train'] + [d for d in splits if d != 'train']
    parts = _latent_trials(who, data_generator, model, dtypes, set(wanted))

    def table(split):
        keys, z = _parts_table(parts, data_generator, [split], set(wanted), cols)
        if not keys:
            raise ValueError('%s: the sessions %s have no %s trial' % (who, wanted, split))
        y = np.concatenate([np.full(parts[k].shape[0], wanted.index(k[0]), dtype=np.int32) for k in keys])
        return z, y
    z_train, y_train = table('train')
    z_eval, y_eval = (z_train, y_train) if splits[0] == 'train' else table(splits[0])
    result = classify_table(z_train, y_train, len(wanted), Cs, n_splits, tol, max_iter, classes=np.asarray(wanted),
                            columns=cols)
    hits, rows = score_table(z_eval, y_eval, result.weights_)
    return hits / rows, result


def classify_table(z, y, n_classes, Cs=_clf.DEFAULT_CS, n_splits=5, tol=1e-4, max_iter=100, classes=None, columns=None):
    """``fitting.classifier.cross_validate`` on a DEVICE table: ``z`` fp32 ``(n, D)``, D <= 64 (a column slice of a
    wider table is read in place), ``y`` the class of every row, 0 .. ``n_classes`` - 1, as a host array.  Classes and
    fold ids (``stratified_folds``) are uploaded once; an iteration of the fit is one ``bn_softmax_cv_lossgrad``
    launch for all ``n_splits x len(Cs)`` models and one transfer of ``M (S (D + 1) + 2)`` doubles; the held-out
    scores are one ``bn_softmax_cv_score`` launch.  -> ``SessionClassifier``."""
    clf = _clf
    y = np.ascontiguousarray(y, dtype=np.int32)
    S, D = int(n_classes), int(z.shape[1])
    folds = clf.stratified_folds(y, n_splits)
    y_d, fold_d = torch.from_numpy(y).to(z.device), torch.from_numpy(folds).to(z.device)
    leaves = {}

    def on(W, leave):
        key = leave.tobytes()
        if key not in leaves:
            leaves[key] = torch.from_numpy(np.ascontiguousarray(leave, dtype=np.int32)).to(z.device)
        return torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(z.device), leaves[key]

    def lossgrad(W, leave):
        M = len(leave)
        # (losses, counts and gradients in the one buffer the launch wrote them to: one transfer, no kernel between)
        host = _hip.softmax_cv_lossgrad(z, y_d, fold_d, *on(W, leave), packed=True).cpu().numpy()
        return host[:M], host[2 * M:].reshape(M, S, D + 1), host[M:2 * M]

    def score(W, leave):
        return _hip.softmax_cv_score(z, y_d, fold_d, *on(W, leave)).cpu().numpy()
    return clf.cross_validate(lossgrad, score, np.bincount(folds, minlength=n_splits), S, D, Cs, tol, max_iter,
                              classes=classes, columns=columns)


def score_table(z, y, weights):
    """``(hits, rows)`` of ONE model ``weights (S, D + 1)`` on the device table ``z`` with the host classes ``y``: the
    rows whose argmax logit is their class, and the rows with a class in [0, S) (``bn_softmax_cv_score``)."""
    W_d = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)[None]).to(z.device)
    y_d = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(z.device)
    none = torch.full((1,), -1, dtype=torch.int32, device=z.device)
    held = _hip.softmax_cv_score(z, y_d, None, W_d, none).cpu().numpy()
    return float(held[0, 0]), float(held[0, 1])


def export_session_classifier(data_generator, model, dtype='val', columns=None, filename=None, **kwargs):
    """``session_classifier``'s ``fc`` as the file the reference's ``fit_classifier`` saves and its hyperparameter
    search reads: ``fc_session_classification.npy`` in the model's version directory (or ``filename``), written with
    ``np.save(np.array([fc]))``.  -> ``(path, fc, SessionClassifier)`` (None on the ranks other than 0)."""
    out = session_classifier(data_generator, model, dtype=dtype, columns=columns, **kwargs)
    if out is None:
        return None
    if filename is None:
        filename = _version_path(model, SESSION_CLASSIFIER_FILE)
    np.save(filename, np.array([out[0]]))
    return filename, out[0], out[1]


# ------------------------------------------------------------------------------------------ ARHMM (second stage)
ARHMM_MODEL_FILE = 'arhmm_best_val_model.pt'
_ARHMM_NOISE = {'gaussian': 'ar'}            # noise_type -> the model's observations ('gaussian' at zero lags)


def _arhmm_trials(who, data_generator, model, data_key, dtypes, wanted):
    """``{(session, trial): fp32 device tensor (T, D)}`` of the trials of the splits ``dtypes`` of the sessions
    ``wanted``: the latents, walked and encoded as ``latent_correlations`` walks and encodes them, or, for
    ``data_key='labels'``, the labels the generator serves (no model is needed for those)."""
    parts = {}
    if data_key == 'labels':
        device = torch.device('cuda', torch.cuda.current_device()) if model is None \
            else next(model.parameters()).device
        for dtype in dtypes:
            data_generator.reset_iterators(dtype)
            for _ in range(sum(len(ds.batch_idxs[dtype]) for ds in data_generator.datasets)):
                single = {'return_multiple': False} if getattr(data_generator, 'n_sessions_per_batch', 1) > 1 else {}
                data, sess = data_generator.next_batch(dtype, **single)
                if 'labels' not in data:
                    raise ValueError('%s: the generator serves no labels (session %d)' % (who, sess))
                if sess not in wanted:
                    continue
                idx = data['batch_idx']
                y = data['labels'][0]
                y = y if torch.is_tensor(y) else torch.from_numpy(np.asarray(y))
                parts[(sess, idx.item() if hasattr(idx, 'item') else int(idx))] = y.to(device, torch.float32)
        return parts
    if data_key != 'ae_latents':
        raise ValueError("%s: data_key must be 'ae_latents' or 'labels', got %r" % (who, data_key))
    if model is None:
        raise ValueError('%s: latents need the model that encodes them' % who)
    return _latent_trials(who, data_generator, model, dtypes, wanted)


def _arhmm_split(parts, keys):
    """``(table, offsets, sessions, trials)`` of the trials ``keys`` in that order; the table is None without rows."""
    keys = [k for k in keys if k in parts]
    offsets = np.concatenate(([0], np.cumsum([parts[k].shape[0] for k in keys]))).astype(np.int64)
    table = torch.cat([parts[k] for k in keys], dim=0).contiguous() if keys and offsets[-1] else None
    return (table, offsets, np.asarray([k[0] for k in keys], dtype=np.int64),
            np.asarray([k[1] for k in keys], dtype=np.int64))


def _arhmm_data_key(hparams):
    """What an ARHMM of ``hparams['model_class']`` was fitted on: the labels for a class with ``label`` in its name
    (``arhmm-labels``), the latents otherwise."""
    return 'labels' if str(hparams.get('model_class', 'arhmm')).find('label') > -1 else 'ae_latents'


def _arhmm_stage(who, data_generator, model, data_key, dtypes, sess_idx, per_split, gate=True, every=False,
                 parts=None):
    """How the entry points of the ARHMM stage open: an invalid dtype key of the model that encodes the latents is an
    error before any trial is read; the ranks other than 0 stop here (``gate``; ``sample_arhmm`` has none); the
    sessions ``sess_idx`` are checked; their trials of the splits ``dtypes`` are gathered ONCE (``_arhmm_trials``;
    ``parts``: gathered already) and put into device tables (``_arhmm_split``) in ``_corr_trial_order``: one per
    split (``per_split``: a dict by split) or one over all of them.  ``every`` is the states exporters' form: every
    session whatever ``sess_idx`` says, a model that may be None even for latents (``_arhmm_trials`` refuses it), and
    ONE table with the trials in ``sorted`` order -- the states files are indexed by it.
    -> ``(wanted, parts, tables)``, or None on a rank that stops."""
    if data_key == 'ae_latents' and not (every and model is None):
        _export_setup(model)
    if gate and bdist.world_size() > 1 and bdist.rank() != 0:
        return None
    wanted = set(range(len(data_generator.datasets))) if every else _wanted_sessions(who, data_generator, sess_idx)
    if parts is None:
        parts = _arhmm_trials(who, data_generator, model, data_key, dtypes, wanted)
    if every:
        return wanted, parts, _arhmm_split(parts, sorted(parts))
    idxs = [ds.batch_idxs for ds in data_generator.datasets]
    if per_split:
        return wanted, parts, {dt: _arhmm_split(parts, _corr_trial_order(idxs, [dt], wanted)) for dt in dtypes}
    return wanted, parts, _arhmm_split(parts, _corr_trial_order(idxs, dtypes, wanted))


def _arhmm_loss(lls, offsets, sel, D):
    """``-loglik / (frames D)`` over the trials ``sel`` (a mask); NaN without frames."""
    frames = float(np.sum(np.diff(offsets)[sel]))
    return float(-np.sum(lls[sel]) / (frames * D)) if frames else float('nan')


def _new_arhmm(D, n_states, n_lags, transitions, kappa, noise_type):
    """The model of one configuration, or the error that names what is not served."""
    from behavenet_amd.models.arhmm import ARHMM
    if noise_type not in _ARHMM_NOISE:
        raise NotImplementedError('fit_arhmm: noise_type %r is not served (gaussian is)' % (noise_type,))
    return ARHMM(n_states, D, lags=n_lags, transitions='stationary' if transitions == 'standard' else transitions,
                 kappa=kappa)


def _arhmm_epoch_rows(rows, epoch, tr_lls, val_lls, splits, n_datasets, D, val_prev, tol):
    """The rows of one epoch -- pooled, then one a session -- appended to ``rows``.  -> ``(stop, val_ll)``: whether
    the fit stops after this epoch, and the ``val_loss`` the next epoch compares with."""
    _, t_off, t_sess, _ = splits['train']
    _, v_off, v_sess, _ = splits['val']
    every_t, every_v = np.ones(len(t_sess), dtype=bool), np.ones(len(v_sess), dtype=bool)
    val_ll = _arhmm_loss(val_lls, v_off, every_v, D)
    rows.append({'epoch': epoch, 'dataset': -1, 'tr_loss': _arhmm_loss(tr_lls, t_off, every_t, D),
                 'val_loss': val_ll, 'trial': -1})
    for d in n_datasets:
        val_ll = _arhmm_loss(val_lls, v_off, v_sess == d, D)
        rows.append({'epoch': epoch, 'dataset': d, 'tr_loss': _arhmm_loss(tr_lls, t_off, t_sess == d, D),
                     'val_loss': val_ll, 'trial': -1})
    # (the reference compares the val_loss it computed last: the last session's)
    if epoch > 10 and np.abs((val_ll - val_prev) / val_ll) < tol:
        print('relative change less than tolerance=%1.2f; training terminating!' % tol)
        return True, val_ll
    return False, val_ll


def _arhmm_test_rows(rows, epoch, test_lls, splits, D):
    _, s_off, s_sess, s_trial = splits['test']
    for i in np.argsort(s_sess, kind='stable'):
        frames = int(s_off[i + 1] - s_off[i])
        rows.append({'epoch': epoch, 'dataset': int(s_sess[i]),
                     'test_loss': float(-test_lls[i] / (frames * D)) if frames else float('nan'),
                     'trial': int(s_trial[i])})


def _arhmm_relabel(arhmm, train, t_off):
    """States relabelled by usage on the training trials."""
    usage = np.bincount(arhmm.table_states(train, t_off), minlength=arhmm.K)
    arhmm.permute(np.argsort(usage)[::-1])


def _fit_arhmm_splits(splits, n_datasets, n_states, n_lags, transitions, kappa, n_iters, tol, rng_seed_model,
                      noise_type):
    if noise_type not in _ARHMM_NOISE:
        raise NotImplementedError('fit_arhmm: noise_type %r is not served (gaussian is)' % (noise_type,))
    train, t_off, _, _ = splits['train']
    if train is None:
        raise ValueError('fit_arhmm: no train frames')
    val, v_off, _, _ = splits['val']
    D = int(train.shape[1])
    arhmm = _new_arhmm(D, n_states, n_lags, transitions, kappa, noise_type)
    arhmm.initialize(train, t_off, seed=rng_seed_model)
    rows, stats, val_prev, epoch = [], None, np.inf, 0
    for epoch in range(int(n_iters) + 1):
        # the 0th epoch has no training: the initialised model is evaluated.  The E-step that scores the training
        # trials of an epoch is the one the next epoch's M-step needs
        if epoch > 0:
            arhmm.m_step(*stats)
        mom, _, xi_sum, g0, tr_lls = arhmm.e_step(train, t_off)
        stats = (mom, xi_sum, g0)
        val_lls = arhmm.trial_logliks(val, v_off) if val is not None else np.zeros((0,))
        stop, val_prev = _arhmm_epoch_rows(rows, epoch, tr_lls, val_lls, splits, n_datasets, D, val_prev, tol)
        if stop:
            break
    test, s_off, _, _ = splits['test']
    if test is not None:
        _arhmm_test_rows(rows, epoch, arhmm.trial_logliks(test, s_off), splits, D)
    _arhmm_relabel(arhmm, train, t_off)
    return arhmm, rows


# ------------------------------------------------------------------------------------------ a grid of ARHMMs
ARHMM_GRID_TABLE_BYTES = 8 << 30        # ll plus gamma of one group of a grid, float64 (rows, states): 8 GiB


def arhmm_grid(n_states, n_lags=(1,), transitions=('stationary',), kappa=(0,), rng_seed_model=(0,)):
    """The configurations of a grid search: the cartesian product of the arguments (a scalar counts as one value) as
    a list of dicts of ``fit_arhmm``'s keyword arguments, in ``itertools.product``'s order over the arguments as
    listed, without the combinations the reference's driver refuses to fit (fitting/arhmm_grid_search.py:25-30):
    ``sticky`` with ``kappa == 0`` and anything else with ``kappa > 0``.  Pure host code."""
    import itertools
    names = ('n_states', 'n_lags', 'transitions', 'kappa', 'rng_seed_model')
    axes = [list(v) if isinstance(v, (list, tuple, np.ndarray, range)) else [v]
            for v in (n_states, n_lags, transitions, kappa, rng_seed_model)]
    grid = []
    for combo in itertools.product(*axes):
        cfg = dict(zip(names, combo))
        if cfg['transitions'] == 'sticky' and cfg['kappa'] == 0:
            continue
        if cfg['transitions'] != 'sticky' and cfg['kappa'] > 0:
            continue
        grid.append(cfg)
    return grid


_ARHMM_GRID_KEYS = ('n_states', 'n_lags', 'transitions', 'kappa', 'rng_seed_model', 'noise_type')


def _arhmm_grid_config(cfg):
    """``cfg`` with ``fit_arhmm``'s defaults filled in."""
    if not isinstance(cfg, dict) or 'n_states' not in cfg or set(cfg) - set(_ARHMM_GRID_KEYS):
        raise ValueError('fit_arhmm_grid: a configuration is a dict with n_states and any of %s, got %r'
                         % (', '.join(_ARHMM_GRID_KEYS[1:]), cfg))
    full = {'n_lags': 1, 'transitions': 'stationary', 'kappa': 0, 'rng_seed_model': 0, 'noise_type': 'gaussian'}
    full.update(cfg)
    return full


def arhmm_grid_groups(grid, n_rows, max_states=None, max_bytes=ARHMM_GRID_TABLE_BYTES):
    """The configurations of ``grid`` cut into groups that advance in one set of launches: lists of positions in
    ``grid``, every position once.  A group has ONE ``n_lags``, at
    most ``max_states`` (512) states and 512 models together, and its ``ll`` and ``gamma`` tables on ``n_rows`` rows
    -- ``2 * 8 * n_rows * states`` bytes -- within ``max_bytes`` (a configuration that is beyond that alone is a
    group of its own).  The configurations of a group keep the grid's order; a group is closed when the next
    configuration of its ``n_lags`` does not fit.  Pure host code."""
    from behavenet_amd import _hip
    max_states = _hip.ARHMM_GRID_MAX_STATES if max_states is None else int(max_states)
    groups, open_group = [], {}
    for i, cfg in enumerate(grid):
        cfg = _arhmm_grid_config(cfg)
        K, lags = int(cfg['n_states']), int(cfg['n_lags'])
        g = open_group.get(lags)
        if g is not None:
            states = sum(int(grid[j]['n_states']) for j in g) + K
            if states > max_states or len(g) >= _hip.ARHMM_GRID_MAX_MODELS or 16 * int(n_rows) * states > max_bytes:
                g = None
        if g is None:
            g = []
            groups.append(g)
            open_group[lags] = g
        g.append(i)
    return groups


def _fit_arhmm_grid_splits(splits, n_datasets, grid, n_iters, tol):
    from behavenet_amd.models.arhmm import ARHMMGroup
    train, t_off, _, _ = splits['train']
    if train is None:
        raise ValueError('fit_arhmm: no train frames')
    val, v_off, _, _ = splits['val']
    test, s_off, _, _ = splits['test']
    D = int(train.shape[1])
    grid = [_arhmm_grid_config(cfg) for cfg in grid]
    # every configuration is built -- and refused, if it is not served -- before the first epoch of any
    models = [_new_arhmm(D, c['n_states'], c['n_lags'], c['transitions'], c['kappa'], c['noise_type']) for c in grid]
    out = [None] * len(grid)
    for members in arhmm_grid_groups(grid, int(train.shape[0])):
        for i in members:
            models[i].initialize(train, t_off, seed=grid[i]['rng_seed_model'])
        rows = {i: [] for i in members}
        val_prev, last = {i: np.inf for i in members}, {i: 0 for i in members}
        active, grouped, group, stats = list(members), None, None, {}
        for epoch in range(int(n_iters) + 1):
            if not active:
                break
            if grouped != active:
                # a model that has stopped leaves the launches; its parameters are those of its last epoch
                group, grouped = ARHMMGroup([models[i] for i in active]), list(active)
            if epoch > 0:
                group.m_step([stats[i] for i in active])
            stats = dict(zip(active, group.e_step(train, t_off)))
            val_lls = group.trial_logliks(val, v_off) if val is not None else np.zeros((len(active), 0))
            going = []
            for k, i in enumerate(active):
                stop, val_prev[i] = _arhmm_epoch_rows(rows[i], epoch, stats[i][4], val_lls[k], splits, n_datasets, D,
                                                      val_prev[i], tol)
                last[i] = epoch
                if not stop:
                    going.append(i)
            active = going
        if test is not None:
            test_lls = ARHMMGroup([models[i] for i in members]).trial_logliks(test, s_off)
            for k, i in enumerate(members):
                _arhmm_test_rows(rows[i], last[i], test_lls[k], splits, D)
        # every member, stopped early or not
        _arhmm_grid_relabel([models[i] for i in members], train, t_off)
        for i in members:
            out[i] = (models[i], rows[i])
    return out


def _arhmm_grid_relabel(models, train, t_off):
    """``_arhmm_relabel`` for the models of one group from ONE decoding of the group: every row of the train table
    lies in a trial, so ``frames`` is ``_arhmm_relabel``'s bincount, and the paths are its paths integer for integer
    (``bn_hmm_grid_viterbi``)."""
    from behavenet_amd.models.arhmm import ARHMMGroup
    for m, (_, frames, _) in zip(models, ARHMMGroup(models).table_runs(train, t_off)):
        m.permute(np.argsort(frames)[::-1])


def fit_arhmm_grid(data_generator, model, grid, n_iters=150, tol=0, sess_idx=None, data_key='ae_latents'):
    """``fit_arhmm`` for every configuration of ``grid`` (``arhmm_grid``; dicts of ``n_states``, ``n_lags``,
    ``transitions``, ``kappa``, ``rng_seed_model``) at once: the trials are walked and encoded ONCE, one device table
    per split, and the configurations advance in groups (``arhmm_grid_groups``: one ``n_lags``, 512 states,
    ``ARHMM_GRID_TABLE_BYTES``), every model of a group one EM iteration in one set of launches
    (``models.arhmm.ARHMMGroup``).  -> a list, in grid order, of the ``(arhmm, rows)`` ``fit_arhmm`` returns for the
    configuration: the same epochs, rows, stop rule per model (a stopped model is frozen and its rows end at its
    epoch), test rows and usage permutation.  A configuration that is not served is refused before the first epoch
    with ``fit_arhmm``'s error.  Under ``torch.distributed`` rank 0 fits and the other ranks return None."""
    who = 'fit_arhmm_grid'
    grid = [_arhmm_grid_config(cfg) for cfg in grid]
    for c in grid:                                          # (types and limits that need no table)
        _new_arhmm(1, c['n_states'], 0, c['transitions'], c['kappa'], c['noise_type'])
    stage = _arhmm_stage(who, data_generator, model, data_key, ('train', 'val', 'test'), sess_idx, True)
    if stage is None:
        return None
    wanted, _, splits = stage
    return _fit_arhmm_grid_splits(splits, sorted(wanted), grid, n_iters, tol)


def fit_arhmm_grid_tables(train, val=None, test=None, grid=(), n_iters=150, tol=0):
    """``fit_arhmm_grid`` for lists of (T, D) arrays or device tensors, with no generator and no model
    (``fit_arhmm_tables`` for a grid)."""
    grid = [_arhmm_grid_config(cfg) for cfg in grid]
    train = list(train) if train is not None else []
    if train:
        D = int(train[0].shape[1])
        for c in grid:                                      # refused before a table is built
            _new_arhmm(D, c['n_states'], c['n_lags'], c['transitions'], c['kappa'], c['noise_type'])
    return _fit_arhmm_grid_splits(_arhmm_table_splits(train, val, test), [0], grid, n_iters, tol)


def fit_arhmm(data_generator, model, n_states, n_lags=1, transitions='stationary', kappa=0, n_iters=150, tol=0,
              rng_seed_model=0, sess_idx=None, data_key='ae_latents', noise_type='gaussian'):
    """Fit an ARHMM on a model's latents by EM with the E-step on the device: the second stage of the BehaveNet
    pipeline, with the bookkeeping of the reference's driver (fitting/arhmm_grid_search.py:132-209).

    The train / val / test trials of the sessions ``sess_idx`` are walked and encoded as ``latent_correlations`` walks
    and encodes them (``hparams['hip_encode_dtype']`` is honoured) and kept as one device table per split, in the
    reference's order.  ``data_key='labels'`` takes the generator's labels in place of latents (``arhmm-labels``;
    ``model`` may be None).  Epochs ``0 .. n_iters``: epoch 0 is evaluated and not trained; ``tr_loss`` and
    ``val_loss`` are ``-loglik / (frames D)``, pooled (``dataset = -1``) and per session; the fit stops after epoch 10
    on a relative ``val_loss`` change below ``tol``; a ``test_loss`` per test trial follows; then the states are
    relabelled by their usage in the Viterbi paths of the training trials.
    -> ``(arhmm, rows)``: the ``models.arhmm.ARHMM`` and the list of dicts the reference hands to ``exp.log``.
    Under ``torch.distributed`` rank 0 fits and the other ranks return None."""
    stage = _arhmm_stage('fit_arhmm', data_generator, model, data_key, ('train', 'val', 'test'), sess_idx, True)
    if stage is None:
        return None
    wanted, _, splits = stage
    return _fit_arhmm_splits(splits, sorted(wanted), n_states, n_lags, transitions, kappa, n_iters, tol,
                             rng_seed_model, noise_type)


def fit_arhmm_tables(train, val=None, test=None, n_states=2, n_lags=1, transitions='stationary', kappa=0, n_iters=150,
                     tol=0, rng_seed_model=0, noise_type='gaussian'):
    """``fit_arhmm`` for lists of (T, D) arrays or device tensors, with no generator and no model: one session
    (``dataset = 0``), the trials numbered by their position in their list."""
    return _fit_arhmm_splits(_arhmm_table_splits(train, val, test), [0], n_states, n_lags, transitions, kappa,
                             n_iters, tol, rng_seed_model, noise_type)


def _arhmm_table_splits(train, val, test):
    from behavenet_amd.models.arhmm import ARHMM
    splits = {}
    for name, datas in (('train', train), ('val', val), ('test', test)):
        datas = list(datas) if datas is not None else []
        if datas:
            table, offsets = ARHMM.as_table(datas)
            table = table if offsets[-1] else None
        else:
            table, offsets = None, np.zeros((1,), dtype=np.int64)
        splits[name] = (table, offsets, np.zeros(len(datas), dtype=np.int64), np.arange(len(datas), dtype=np.int64))
    return splits


def export_states(hparams, data_generator, arhmm, model=None, filename=None):
    """The most likely states of every train / val / test trial, per session
    ``{'states': [per-trial int arrays, empty for gap trials], 'trials': batch_idxs}`` in
    ``<lab>_<expt>_<animal>_<session>_states.pkl`` under ``hparams['expt_dir']/version_<hparams['version']>`` (or
    ``filename``): the reference's ``export_states`` (fitting/eval.py:121-188).  The trials' latents (encoded by
    ``model``) or, for a ``model_class`` with ``label`` in it, their labels go into ONE device table and ONE Viterbi
    launch.  -> the file names (an empty list on the ranks other than 0)."""
    stage = _arhmm_stage('export_states', data_generator, model, _arhmm_data_key(hparams), ('train', 'val', 'test'),
                         None, False, every=True)
    if stage is None:
        return []
    table, offsets, sessions, trials = stage[2]
    states = [[np.array([]) for _ in range(ds.n_trials)] for ds in data_generator.datasets]
    if table is not None:
        path = arhmm.table_states(table, offsets)
        for i, (sess, trial) in enumerate(zip(sessions, trials)):
            states[sess][trial] = path[offsets[i]:offsets[i + 1]].copy()
    return _write_per_session(data_generator, hparams, filename, 'states', 'states', states, 'states')


def check_export_arhmm(who, kwargs):
    """``hparams['export_arhmm']``: a dict of ``fit_arhmm``'s keyword arguments with ``n_states`` among them."""
    known = set(inspect.signature(fit_arhmm).parameters) - {'data_generator', 'model'}
    if not isinstance(kwargs, dict) or 'n_states' not in kwargs or not set(kwargs) <= known:
        raise ValueError('%s: expected a dict with n_states and any of %s, got %r' % (who, sorted(known), kwargs))
    from behavenet_amd.models.arhmm import ARHMM
    ARHMM(kwargs['n_states'], 1, lags=kwargs.get('n_lags', 1),                         # (limits and served types)
          transitions={'standard': 'stationary'}.get(kwargs.get('transitions'), kwargs.get('transitions', 'stationary')))


def export_arhmm(data_generator, model, **kwargs):
    """``fit_arhmm`` + ``export_states`` for a trained model: the ARHMM pickled as ``arhmm_best_val_model.pt`` and the
    states files next to the model's latents.  -> ``(arhmm, rows, model file, states files)``, None on the ranks
    other than 0."""
    out = fit_arhmm(data_generator, model, **kwargs)
    if out is None:
        return None
    arhmm, rows = out
    labels = kwargs.get('data_key', 'ae_latents') == 'labels'
    hparams = {'expt_dir': model.hparams['expt_dir'], 'version': model.version,
               'model_class': ('arhmm' if kwargs.get('n_lags', 1) > 0 else 'hmm') + ('-labels' if labels else '')}
    path = _version_path(hparams, ARHMM_MODEL_FILE)
    with open(path, 'wb') as f:
        pickle.dump(arhmm, f)
    return arhmm, rows, path, export_states(hparams, data_generator, arhmm, model=model)


# ------------------------------------------------------------------------------------------ states of a grid of ARHMMs
ARHMM_GRID_DIR = 'arhmm_grid'
ARHMM_GRID_SELECTION_FILE = 'selection.pkl'


def _grid_models(who, fits):
    """The models of ``fits``: the ``(arhmm, rows)`` pairs ``fit_arhmm_grid`` returns, or bare models."""
    from behavenet_amd.models.arhmm import ARHMM
    models = [f[0] if isinstance(f, (tuple, list)) else f for f in fits]
    for m in models:
        if not isinstance(m, ARHMM):
            raise ValueError('%s: expected fitted ARHMMs or (arhmm, rows) pairs, got %s' % (who, type(m).__name__))
    return models


def _grid_groups_of(models, n_rows):
    """``(positions, ARHMMGroup)`` for the fitted ``models`` cut by ``arhmm_grid_groups``' limits."""
    from behavenet_amd.models.arhmm import ARHMMGroup
    grid = [{'n_states': m.K, 'n_lags': m.lags} for m in models]
    return [(members, ARHMMGroup([models[i] for i in members])) for members in arhmm_grid_groups(grid, n_rows)]


def arhmm_grid_runs(fits, tables, offsets=None):
    """Per fitted model of ``fits`` (``fit_arhmm_grid``'s list, or bare models) the ``(runs, frames, trans)`` of
    ``ARHMM.table_runs`` on one table, host arrays, in the order of ``fits``.  ``tables``: an fp32 device table (n, D)
    with its ``offsets`` (int64 (S + 1)), or a list of (T, D) arrays or device tensors without.  The models are
    decoded in groups with the limits of ``arhmm_grid_groups`` (one ``n_lags``, 512 states, 512 models): a group is one
    log-likelihood launch, one Viterbi launch a class, the run searches and two transfers
    (``ARHMMGroup.table_runs``)."""
    from behavenet_amd.models.arhmm import ARHMM
    who = 'arhmm_grid_runs'
    models = _grid_models(who, fits)
    if offsets is None:
        tables, offsets = ARHMM.as_table(list(tables))
    out = [None] * len(models)
    for members, group in _grid_groups_of(models, int(tables.shape[0])):
        for i, triple in zip(members, group.table_runs(tables, offsets)):
            out[i] = triple
    return out


def arhmm_grid_states(data_generator, model, fits, dtype='test', sess_idx=None, data_key='ae_latents'):
    """``arhmm_grid_runs`` on the trials of the split ``dtype`` of the sessions ``sess_idx``: the trials are walked
    and encoded ONCE for all models (``fit_arhmm``'s walk and order), then every group is decoded on that one table.
    -> the per-model triples, or ``None`` per model when the split has no frames.  Under ``torch.distributed`` rank
    0 works and the other ranks return None."""
    who = 'arhmm_grid_states'
    dtypes = _splits(who, dtype)
    models = _grid_models(who, fits)
    stage = _arhmm_stage(who, data_generator, model, data_key, dtypes, sess_idx, False)
    if stage is None:
        return None
    table, offsets, _, _ = stage[2]
    if table is None:
        return [None] * len(models)
    return arhmm_grid_runs(models, table, offsets)


def arhmm_grid_selection(grid, fits, stats, test_frames=None):
    """The table a choice over a grid is made from: one dict per configuration of ``grid``, in grid order.  Pure host
    code.  ``fits``: ``fit_arhmm_grid``'s ``(arhmm, rows)`` pairs; ``stats``: the per-model ``(runs, frames, trans)``
    of ``arhmm_grid_runs`` / ``arhmm_grid_states``, None (or None for a model) where there are none.  A dict holds

    * the configuration's own keys;
    * ``epochs``: the number of the last epoch the model was scored at (0 is the initialised model);
    * ``tr_loss`` and ``val_loss``: those of the last row with ``dataset == -1`` (pooled over the sessions);
    * ``test_loss``: the mean of the rows' ``test_loss`` weighted by the trials' frames -- ``test_frames``, a dict
      ``{(dataset, trial): frames}``; without it every test trial weighs the same, which is the same number where the
      trials are equally long -- NaN rows (empty trials) left out, NaN without test rows;
    * ``usage``: ``frames / sum(frames)``, a float64 array (K) (zeros when no frame was decoded);
    * ``n_states_used``: the states with ``frames > 0``;
    * ``n_states_99``: the fewest states whose frames, taken from the most used down, cover 99 % of all frames
      (``cumulative >= 0.99 * total`` in integers: ``100 * cumulative >= 99 * total``), 0 without frames;
    * ``n_runs``; ``median_duration`` and ``mean_duration`` over ``end - beg`` of ALL runs, those that touch the
      ends of their trials included (NaN without runs).

    The run fields are None for a model without ``stats``."""
    who = 'arhmm_grid_selection'
    grid = list(grid)
    fits = list(fits)
    stats = [None] * len(grid) if stats is None else list(stats)
    if len(fits) != len(grid) or len(stats) != len(grid):
        raise ValueError('%s: %d configurations, %d fits and %d stats' % (who, len(grid), len(fits), len(stats)))
    table = []
    for cfg, fit, st in zip(grid, fits, stats):
        if not isinstance(cfg, dict):
            raise ValueError('%s: a configuration is a dict, got %r' % (who, cfg))
        rows = fit[1]
        out = dict(cfg)
        pooled = [r for r in rows if r.get('dataset') == -1 and 'val_loss' in r]
        out['epochs'] = int(pooled[-1]['epoch']) if pooled else 0
        out['tr_loss'] = float(pooled[-1]['tr_loss']) if pooled else float('nan')
        out['val_loss'] = float(pooled[-1]['val_loss']) if pooled else float('nan')
        num = den = 0.0
        for r in rows:
            if 'test_loss' not in r or np.isnan(r['test_loss']):
                continue
            w = 1.0 if test_frames is None else float(test_frames[(int(r['dataset']), int(r['trial']))])
            num += w * float(r['test_loss'])
            den += w
        out['test_loss'] = num / den if den else float('nan')
        if st is None:
            for key in ('usage', 'n_states_used', 'n_states_99', 'n_runs', 'median_duration', 'mean_duration'):
                out[key] = None
        else:
            runs, frames, _ = st
            runs = np.asarray(runs).reshape(-1, 4).astype(np.int64)
            frames = np.asarray(frames, dtype=np.int64).reshape(-1)
            total = int(frames.sum())
            out['usage'] = frames / float(total) if total else np.zeros(len(frames))
            out['n_states_used'] = int(np.sum(frames > 0))
            covered = np.cumsum(np.sort(frames)[::-1])
            out['n_states_99'] = int(np.argmax(100 * covered >= 99 * total)) + 1 if total else 0
            durations = runs[:, 2] - runs[:, 1]
            out['n_runs'] = int(len(runs))
            out['median_duration'] = float(np.median(durations)) if len(runs) else float('nan')
            out['mean_duration'] = float(np.mean(durations)) if len(runs) else float('nan')
        table.append(out)
    return table


def _grid_model_dir(hparams, i):
    return _version_path(hparams, ARHMM_GRID_DIR, 'model_%03i' % i)


def export_states_grid(hparams, data_generator, fits, model=None, _parts=None):
    """``export_states`` for every fitted model of ``fits`` at once: the trials of all sessions go into ONE device
    table -- walked and encoded once -- and every group of models (``arhmm_grid_groups``' limits) is decoded by one
    group Viterbi (``ARHMMGroup.table_states``).  Model ``i`` gets ``export_states``' files,
    ``<lab>_<expt>_<animal>_<session>_states.pkl``, under ``version_<v>/arhmm_grid/model_%03i/``.  -> per model the
    list of its file names (an empty list on the ranks other than 0)."""
    who = 'export_states_grid'
    models = _grid_models(who, fits)
    stage = _arhmm_stage(who, data_generator, model, _arhmm_data_key(hparams), ('train', 'val', 'test'), None, False,
                         every=True, parts=_parts)
    if stage is None:
        return []
    table, offsets, sessions, trials = stage[2]
    paths = [None] * len(models)
    if table is not None:
        for members, group in _grid_groups_of(models, int(table.shape[0])):
            for i, path in zip(members, group.table_states(table, offsets)):
                paths[i] = path
    filenames = []
    for i in range(len(models)):
        states = [[np.array([]) for _ in range(ds.n_trials)] for ds in data_generator.datasets]
        if paths[i] is not None:
            for t, (sess, trial) in enumerate(zip(sessions, trials)):
                states[sess][trial] = paths[i][offsets[t]:offsets[t + 1]].copy()
        os.makedirs(_grid_model_dir(hparams, i), exist_ok=True)
        names = []
        for sess, dataset in enumerate(data_generator.datasets):
            out = _session_filename(hparams, dataset, None, 'states.pkl', ARHMM_GRID_DIR, 'model_%03i' % i)
            with open(out, 'wb') as f:
                pickle.dump({'states': states[sess], 'trials': dataset.batch_idxs}, f)
            names.append(out)
        filenames.append(names)
    print('saved the states of %i models under %s' % (len(models), os.path.dirname(_grid_model_dir(hparams, 0))))
    return filenames


def check_export_arhmm_grid(who, kwargs):
    """``hparams['export_arhmm_grid']``: a dict of ``export_arhmm_grid``'s keyword arguments with ``grid``, a
    non-empty list of configurations, among them.  Every configuration is built -- a type or a limit that is not
    served is ``fit_arhmm``'s error -- and ``dtype`` is checked, before any epoch."""
    known = set(inspect.signature(export_arhmm_grid).parameters) - {'data_generator', 'model'}
    if not isinstance(kwargs, dict) or 'grid' not in kwargs or not set(kwargs) <= known:
        raise ValueError('%s: expected a dict with grid and any of %s, got %r' % (who, sorted(known), kwargs))
    grid = kwargs['grid']
    if not isinstance(grid, (list, tuple)) or not len(grid):
        raise ValueError('%s: grid is a non-empty list of configurations (arhmm_grid), got %r' % (who, grid))
    dtype = kwargs.get('dtype', 'val')
    if not isinstance(dtype, str):
        raise ValueError("%s: dtype must be 'train', 'val' or 'test', got %r" % (who, dtype))
    _splits(who, dtype)
    if kwargs.get('data_key', 'ae_latents') not in ('ae_latents', 'labels'):
        raise ValueError("%s: data_key must be 'ae_latents' or 'labels', got %r" % (who, kwargs['data_key']))
    for cfg in grid:
        c = _arhmm_grid_config(cfg)
        _new_arhmm(1, c['n_states'], c['n_lags'], c['transitions'], c['kappa'], c['noise_type'])


def export_arhmm_grid(data_generator, model, grid, n_iters=150, tol=0, sess_idx=None, data_key='ae_latents',
                      dtype='val'):
    """``fit_arhmm_grid`` + ``arhmm_grid_selection`` on the split ``dtype`` + ``export_states_grid`` for a trained
    model.  The train / val / test trials are walked and encoded ONCE for the fit, the selection table and -- when
    ``sess_idx`` names every session -- the states.  Under ``version_<v>/arhmm_grid/``: ``selection.pkl``, a dict of
    ``grid``, ``rows`` (per configuration the rows of its fit) and ``selection`` (the table), and per configuration
    ``model_%03i/arhmm_best_val_model.pt`` with its states files.
    -> ``(fits, selection, selection file, states files)``, None on the ranks other than 0."""
    who = 'export_arhmm_grid'
    check_export_arhmm_grid(who, {'grid': grid, 'dtype': dtype, 'data_key': data_key})
    full = [_arhmm_grid_config(cfg) for cfg in grid]
    stage = _arhmm_stage(who, data_generator, model, data_key, ('train', 'val', 'test'), sess_idx, True)
    if stage is None:
        return None
    wanted, parts, splits = stage
    fits = _fit_arhmm_grid_splits(splits, sorted(wanted), full, n_iters, tol)
    table, offsets, _, _ = splits[dtype]
    stats = arhmm_grid_runs(fits, table, offsets) if table is not None else None
    _, s_off, s_sess, s_trial = splits['test']
    test_frames = {(int(s), int(t)): int(f) for s, t, f in zip(s_sess, s_trial, np.diff(s_off))}
    selection = arhmm_grid_selection(list(grid), fits, stats, test_frames=test_frames)
    labels = data_key == 'labels'
    hparams = {'expt_dir': model.hparams['expt_dir'], 'version': model.version,
               'model_class': 'arhmm' + ('-labels' if labels else '')}
    for i, (arhmm, _) in enumerate(fits):
        os.makedirs(_grid_model_dir(hparams, i), exist_ok=True)
        with open(os.path.join(_grid_model_dir(hparams, i), ARHMM_MODEL_FILE), 'wb') as f:
            pickle.dump(arhmm, f)
    path = os.path.join(os.path.dirname(_grid_model_dir(hparams, 0)), ARHMM_GRID_SELECTION_FILE)
    with open(path, 'wb') as f:
        pickle.dump({'grid': list(grid), 'rows': [rows for _, rows in fits], 'selection': selection}, f)
    every = wanted == set(range(len(data_generator.datasets)))
    files = export_states_grid(hparams, data_generator, fits, model=model, _parts=parts if every else None)
    return fits, selection, path, files


# ------------------------------------------------------------------------------------------ ARHMM predictions
ARHMM_PREDICTIONS_FILE = 'arhmm_predictions.csv'
_PREDICTION_MEASURES = ('mse', 'r2', 'mse_persistence', 'r2_persistence')


def _arhmm_scored_table(who, data_generator, model, data_key, dtype, sess_idx):
    """``_arhmm_stage``'s ONE table over the splits ``dtype`` for the scores of a fitted ARHMM, which need frames:
    a table without any is a ValueError.  -> ``_arhmm_split``'s tuple, or None on the ranks other than 0."""
    dtypes = _splits(who, dtype)
    stage = _arhmm_stage(who, data_generator, model, data_key, dtypes, sess_idx, False)
    if stage is None:
        return None
    if stage[2][0] is None:
        raise ValueError('%s: the sessions %s have no %s frames' % (who, sorted(stage[0]), ' or '.join(dtypes)))
    return stage[2]


def summarise_prediction_sums(sums, min_valid=10):
    """Prediction scores from the sums ``ARHMM.prediction_sums`` returns, ``(2, S, D, 4)`` -- the model's and the
    persistence baseline's, per trial and dimension -- in numpy float64 on the host, by ``summarise_label_sums``:
    ``'n'``, ``'mse'``, ``'r2'``, ``'mse_persistence'``, ``'r2_persistence'``, each ``(S, D)`` (scores NaN where
    ``n <= min_valid``), and ``'pooled'``, the same five per dimension ``(D,)`` from the sums added over the trials
    plus, over all dimensions, ``'mse_all'`` / ``'mse_persistence_all'`` (``sum_d sd / sum_d n``) and ``'r2_all'`` /
    ``'r2_persistence_all'`` (the variance-weighted R^2, ``1 - sum_d sd / sum_d ss_tot``)."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 4 or sums.shape[0] != 2 or sums.shape[3] != 4:
        raise ValueError('summarise_prediction_sums: expected sums (2, S, D, 4), got %s' % (tuple(sums.shape),))
    model, base = summarise_label_sums(sums[0], min_valid), summarise_label_sums(sums[1], min_valid)
    out = {'n': model['n'], 'mse': model['mse'], 'r2': model['r2'], 'mse_persistence': base['mse'],
           'r2_persistence': base['r2']}
    pooled = {'n': model['pooled']['n']}
    for scored, tot, tag in ((model, sums[0].sum(axis=0), ''), (base, sums[1].sum(axis=0), '_persistence')):
        pooled['mse' + tag], pooled['r2' + tag] = scored['pooled']['mse'], scored['pooled']['r2']
        rows = float(tot[:, 0].sum())
        pooled['mse%s_all' % tag] = float(tot[:, 3].sum() / rows) if rows else float('nan')
        pooled['r2%s_all' % tag] = scored['pooled']['r2_variance_weighted']
    out['pooled'] = pooled
    return out


def arhmm_predictions(data_generator, model, arhmm, dtype='test', weights='predictive', sess_idx=None,
                      data_key='ae_latents', return_latents=False):
    """How well a fitted ARHMM predicts the next latent, in the latents' own units: per trial and dimension the mean
    squared error and R^2 of the one-step-ahead prediction ``sum_k w_t[k] (b_k + sum_l A_k[l] x_{t-1-l})`` and of the
    persistence baseline ``x_{t-1}`` over the rows ``t >= max(lags, 1)`` of every trial of the split ``dtype`` (or a
    list of splits) of the sessions ``sess_idx``.  ``weights``: ``'predictive'``, the causal
    ``p(z_t | x_0 .. x_{t-1})``, or ``'smoothed'``, the posterior marginals (the ``ssm`` library's ``smooth``).

    The trials are walked and encoded ONCE as ``fit_arhmm`` walks and encodes them (``data_key='labels'``: the
    generator's labels, ``model`` may be None) into one device table; log-likelihoods, weights, predictions and the
    two ``bn_segment_label_sums`` reductions follow each other on the device (``ARHMM.prediction_sums``) and
    ``(2, S, D, 4)`` doubles cross to the host.
    -> ``summarise_prediction_sums``'s dict plus ``'session'`` and ``'trial'``, int arrays ``(S,)`` in the table's
    order, and ``'sums'``; with ``return_latents`` also ``'latents'`` and ``'latents_pred'``, lists of host (T, D)
    arrays per trial -- the operands of ``real_vs_sampled_movie(model, latents, latents_pred)`` for a
    real-versus-predicted movie.  Under ``torch.distributed`` rank 0 works and the other ranks return None."""
    stage = _arhmm_scored_table('arhmm_predictions', data_generator, model, data_key, dtype, sess_idx)
    if stage is None:
        return None
    table, offsets, sessions, trials = stage
    xhat, valid = arhmm.table_predictions(table, offsets, weights)
    sums = arhmm.sums_of_predictions(table, offsets, xhat, valid)
    out = summarise_prediction_sums(sums)
    out.update({'session': sessions, 'trial': trials, 'sums': sums})
    if return_latents:
        host, pred = table.cpu().numpy(), xhat.cpu().numpy()
        out['latents'] = [host[offsets[i]:offsets[i + 1]].copy() for i in range(len(sessions))]
        out['latents_pred'] = [pred[offsets[i]:offsets[i + 1]].copy() for i in range(len(sessions))]
    return out


def export_arhmm_predictions(hparams, data_generator, arhmm, model=None, dtype='test', weights='predictive',
                             filename=None):
    """``arhmm_predictions`` as a table next to the states files: ``arhmm_predictions.csv`` under
    ``hparams['expt_dir']/version_<hparams['version']>`` (or ``filename``), one row per (trial, dimension) in the
    table's order with the columns ``Session, Trial, Dim, N, MSE, R2, MSE_persistence, R2_persistence``; a NaN is an
    empty field, as in ``export_label_r2``'s table.  Latents or labels by ``hparams['model_class']`` as
    ``export_states`` chooses.  Written with the ``csv`` module.  -> the path (None on the ranks other than 0)."""
    scores = arhmm_predictions(data_generator, model, arhmm, dtype=dtype, weights=weights,
                               data_key=_arhmm_data_key(hparams))
    if scores is None:
        return None
    if filename is None:
        filename = _version_path(hparams, ARHMM_PREDICTIONS_FILE)
    return _write_csv(filename, ['Session', 'Trial', 'Dim', 'N', 'MSE', 'R2', 'MSE_persistence', 'R2_persistence'],
                      ([int(sess), int(trial), d, int(scores['n'][k, d])]
                       + [scores[name][k, d] for name in _PREDICTION_MEASURES]
                       for k, (sess, trial) in enumerate(zip(scores['session'], scores['trial']))
                       for d in range(scores['n'].shape[1])))


# ------------------------------------------------------------------------------------------ ARHMM forecasts
ARHMM_FORECASTS_FILE = 'arhmm_forecasts.csv'


def summarise_forecast_sums(sums, min_valid=10):
    """Forecast scores per horizon from the sums ``ARHMM.forecast_sums`` returns, ``(2, H, S, D, 4)``, in numpy float64
    on the host: ``summarise_prediction_sums`` a horizon, stacked -- ``'n'``, ``'mse'``, ``'r2'``,
    ``'mse_persistence'``, ``'r2_persistence'``, each ``(H, S, D)``; ``'pooled'`` with the same five ``(H, D)`` and
    ``'mse_all'``, ``'r2_all'``, ``'mse_persistence_all'``, ``'r2_persistence_all'`` ``(H,)`` -- and
    ``'horizon_of_no_gain'``: the first horizon (from 1) at which the pooled ``mse_all`` is not below the pooled
    ``mse_persistence_all`` (a NaN is not below), or None if the model wins at every horizon served."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 5 or sums.shape[0] != 2 or sums.shape[4] != 4:
        raise ValueError('summarise_forecast_sums: expected sums (2, H, S, D, 4), got %s' % (tuple(sums.shape),))
    per = [summarise_prediction_sums(sums[:, h], min_valid) for h in range(sums.shape[1])]
    out = {key: np.stack([p[key] for p in per]) for key in ('n',) + _PREDICTION_MEASURES}
    out['pooled'] = {key: np.stack([np.asarray(p['pooled'][key]) for p in per]) for key in per[0]['pooled']}
    out['horizon_of_no_gain'] = None
    for h, (mse, base) in enumerate(zip(out['pooled']['mse_all'], out['pooled']['mse_persistence_all'])):
        if not mse < base:
            out['horizon_of_no_gain'] = h + 1
            break
    return out


def arhmm_forecasts(data_generator, model, arhmm, horizons=10, dtype='test', sess_idx=None, data_key='ae_latents'):
    """How many frames ahead a fitted ARHMM still beats ``x_{t-1}``: per horizon ``h = 1 .. horizons``, trial and
    dimension the mean squared error and R^2 of the exact forecast ``E[x_{t+h-1} | x_0 .. x_{t-1}]`` and of the
    persistence baseline ``x_{t-1}`` over the origin rows ``t >= max(lags, 1)`` of every trial with ``t + h - 1``
    still in the trial.  The trials are walked and encoded ONCE as ``arhmm_predictions`` walks and encodes them;
    ``ARHMM.forecast_sums`` scores all horizons in one launch and ``(2, H, S, D, 4)`` doubles cross to the host.
    -> ``summarise_forecast_sums``'s dict plus ``'session'`` and ``'trial'``, int arrays ``(S,)`` in the table's
    order, and ``'sums'``.  Under ``torch.distributed`` rank 0 works and the other ranks return None."""
    stage = _arhmm_scored_table('arhmm_forecasts', data_generator, model, data_key, dtype, sess_idx)
    if stage is None:
        return None
    table, offsets, sessions, trials = stage
    sums = arhmm.forecast_sums(table, offsets, horizons)
    out = summarise_forecast_sums(sums)
    out.update({'session': sessions, 'trial': trials, 'sums': sums})
    return out


def export_arhmm_forecasts(hparams, data_generator, arhmm, model=None, horizons=10, dtype='test', filename=None):
    """``arhmm_forecasts`` as a table next to ``arhmm_predictions.csv``: ``arhmm_forecasts.csv`` under
    ``hparams['expt_dir']/version_<hparams['version']>`` (or ``filename``), one row per (horizon, trial, dimension)
    with the columns ``Horizon, Session, Trial, Dim, N, MSE, R2, MSE_persistence, R2_persistence``; a NaN is an empty
    field.  Latents or labels by ``hparams['model_class']`` as ``export_states`` chooses.  -> the path (None on the
    ranks other than 0)."""
    scores = arhmm_forecasts(data_generator, model, arhmm, horizons=horizons, dtype=dtype,
                             data_key=_arhmm_data_key(hparams))
    if scores is None:
        return None
    if filename is None:
        filename = _version_path(hparams, ARHMM_FORECASTS_FILE)
    write_forecasts_csv(filename, scores)
    return filename


def write_forecasts_csv(filename, scores):
    """The rows of ``export_arhmm_forecasts`` from ``arhmm_forecasts``'s dict."""
    _write_csv(filename, ['Horizon', 'Session', 'Trial', 'Dim', 'N', 'MSE', 'R2', 'MSE_persistence', 'R2_persistence'],
               ([h + 1, int(sess), int(trial), d, int(scores['n'][h, k, d])]
                + [scores[name][h, k, d] for name in _PREDICTION_MEASURES]
                for h in range(scores['n'].shape[0])
                for k, (sess, trial) in enumerate(zip(scores['session'], scores['trial']))
                for d in range(scores['n'].shape[2])))


def check_export_arhmm_forecasts(who, kwargs, export_arhmm=True):
    """``hparams['export_arhmm_forecasts']``: a dict with ``horizons`` (an int from 1 to 32) and, if wanted, ``dtype``;
    it scores the model that ``hparams['export_arhmm']`` fits, so that key has to be there (``export_arhmm``: its
    value)."""
    from behavenet_amd._hip import check_arhmm_horizons
    if not isinstance(kwargs, dict) or 'horizons' not in kwargs or not set(kwargs) <= {'horizons', 'dtype'}:
        raise ValueError("%s: expected a dict with horizons and, if wanted, dtype, got %r" % (who, kwargs))
    check_arhmm_horizons(who, kwargs['horizons'])
    _splits(who, kwargs.get('dtype', 'test'))
    if not export_arhmm:
        raise ValueError("%s scores the model that hparams['export_arhmm'] fits, and that key is not set" % who)


# ------------------------------------------------------------------------------------------ ARHMM samples
def sample_arhmm(data_generator, model, arhmm, n_samples=50, conditional=True, dtype='test', sess_idx=None,
                 data_key='ae_latents', seed=0):
    """Real and sampled latents of a fitted ARHMM: the dict of the reference's ``get_model_latents_states``
    (plotting/arhmm_utils.py:134-251) without its ``model`` entry.

    ``latents``, ``states`` and ``trial_idxs``: per split (train / val / test) the trials of the sessions ``sess_idx``
    in ``_corr_trial_order``'s order, as host arrays (fp32 latents, int32 Viterbi paths -- ONE ``table_states`` launch
    a split) and ``(session, trial)`` pairs -- the trial numbers alone when one session is asked for, as in the
    reference.  ``latents_gen``: with ``conditional`` one sampled trial per real trial of ``dtype``, drawn along its
    most likely states with the real trial's first ``lags`` rows (``ARHMM.sample_conditional``), and ``states_gen`` is
    ``[]``; else ``n_samples`` fully generated trials as long as the first trial of ``dtype``, 200 burn-in rows
    dropped (``ARHMM.sample``), with their states.  ``n_samples = 0`` returns two empty lists.  The draws are
    reproducible for a given ``seed``, device and torch build only (``ARHMM.sample_table``).

    Departures from the reference: the initial rows of a conditional sample are the real trial's (the reference
    seeds row 0 from the first real latent through ``sample_x``) and those of a generated trial N(0, I); parity with
    the ``ssm`` library is unchecked."""
    who = 'sample_arhmm'
    _splits(who, dtype)
    wanted, _, splits = _arhmm_stage(who, data_generator, model, data_key, ('train', 'val', 'test'), sess_idx, True,
                                     gate=False)
    out = {'latents': {}, 'states': {}, 'trial_idxs': {}, 'latents_gen': [], 'states_gen': []}
    for dt, (table, offsets, sess, trials) in splits.items():
        n = len(sess)
        if table is not None:
            path = arhmm.table_states(table, offsets)
            host = table.cpu().numpy()
        else:
            path, host = np.zeros((0,), dtype=np.int32), np.zeros((0, arhmm.D), dtype=np.float32)
        out['latents'][dt] = [host[offsets[i]:offsets[i + 1]].copy() for i in range(n)]
        out['states'][dt] = [path[offsets[i]:offsets[i + 1]].copy() for i in range(n)]
        out['trial_idxs'][dt] = trials.copy() if len(wanted) == 1 else list(zip(sess.tolist(), trials.tolist()))
    if int(n_samples) > 0:
        real = out['latents'][dtype]
        if not real:
            raise ValueError('%s: no %s trials to sample by' % (who, dtype))
        if conditional:
            _, out['latents_gen'] = arhmm.sample_conditional(real, seed=seed)
        else:
            out['states_gen'], out['latents_gen'] = arhmm.sample(real[0].shape[0], n_samples=int(n_samples),
                                                                 burn_in=200, seed=seed)
    return out


def real_vs_sampled_plan(lengths, max_frames, n_buffer):
    """Source rows of one column of the real-vs-sampled movie: trials of ``lengths`` frames are appended, each followed
    by ``n_buffer`` blank frames, until there are at least ``max_frames`` frames (the reference's
    ``while ims.shape[0] < max_frames`` loop, plotting/arhmm_utils.py:598-619).  -> ``(src, n_trials)``: per movie
    frame the row of the table of the first ``n_trials`` trials stacked, -1 for a blank frame.  Running out of trials is
    a ValueError (the reference's IndexError)."""
    src, used, rows = [], 0, 0
    while len(src) < max_frames:
        if used >= len(lengths):
            raise ValueError('real_vs_sampled_movie: %d trials give %d frames, max_frames is %d'
                             % (len(lengths), len(src), max_frames))
        src.extend(range(rows, rows + int(lengths[used])))
        src.extend([-1] * n_buffer)
        rows += int(lengths[used])
        used += 1
    return np.asarray(src, dtype=np.int64), used


def real_vs_sampled_movie_device(model, latents, latents_gen, max_frames=400, n_buffer=5, labels_0=None,
                                 apply_inverse_transform=True, chunk_size=200):
    """The frames of the reference's real-vs-sampled movie (``real_vs_sampled_wrapper`` /
    ``make_real_vs_sampled_movies``, plotting/arhmm_utils.py:513-700) as a uint8 DEVICE tensor ``(T, C * H, 2 * W)``:
    the left column plays the decoded real latents ``latents`` (a list of (T_i, D) trials), the right the decoded
    samples ``latents_gen``; the channels of a frame are stacked vertically, as the reference's
    ``np.concatenate(..., axis=1)`` stacks them.

    Per column trials are appended until there are at least ``max_frames`` frames, ``n_buffer`` all-zero frames after
    every trial, the last one included (``real_vs_sampled_plan``); ``T`` is the smaller of the two counts.  Running out
    of trials before ``max_frames`` is a ValueError that says how many frames there were.  The rows of the trials
    used are decoded in ONE batched pass (``decode_points_device``, which honours ``hparams['hip_decode_dtype']``)
    and tiled by one mosaic launch per ``chunk_size`` movie frames (``_hip.frame_mosaic_u8`` on the frames viewed as
    ``(P * C, 1, H, W)``); only the movie crosses to the host.  ``labels_0``: the labels of a cond-AE / cond-VAE, one
    row for all frames."""
    max_frames, n_buffer, chunk_size = int(max_frames), int(n_buffer), int(chunk_size)
    if max_frames < 1 or n_buffer < 0 or chunk_size < 1:
        raise ValueError('real_vs_sampled_movie: max_frames %d, n_buffer %d, chunk_size %d'
                         % (max_frames, n_buffer, chunk_size))
    sides, tables = [], []
    rows = 0
    for trials in (latents, latents_gen):
        trials = [t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in trials]
        for t in trials:
            if t.ndim != 2:
                raise ValueError('real_vs_sampled_movie: a trial must be (T, D), got %s' % (t.shape,))
        src, used = real_vs_sampled_plan([len(t) for t in trials], max_frames, n_buffer)
        sides.append(np.where(src >= 0, src + rows, -1))
        tables.extend(np.asarray(t, dtype=np.float32) for t in trials[:used])
        rows += sum(len(t) for t in trials[:used])
    n_t = min(len(sides[0]), len(sides[1]))
    table = np.ascontiguousarray(np.concatenate(tables, axis=0))
    if not len(table):
        raise ValueError('real_vs_sampled_movie: the trials have no frames')
    frames = decode_points_device(model, table, labels_0, apply_inverse_transform, chunk_size)
    P, C, H, W = frames.shape
    planes = frames.contiguous().view(P * C, 1, H, W)

    def src_of(beg, end):
        # mosaic row c of column q shows channel c of the column's frame: plane s * C + c
        s = np.stack([sides[0][beg:end], sides[1][beg:end]], axis=1)                  # (t, 2)
        src = np.where(s[:, None, :] >= 0, s[:, None, :] * C + np.arange(C)[None, :, None], -1)
        return src.astype(np.int32)                                                   # (t, C, 2)
    return _mosaic_in_chunks(planes, src_of, n_t, 0, None, chunk_size)


def real_vs_sampled_movie(model, latents, latents_gen, max_frames=400, n_buffer=5, labels_0=None,
                          apply_inverse_transform=True, chunk_size=200):
    """``real_vs_sampled_movie_device`` as a numpy array ``(T, C * H, 2 * W)`` of uint8."""
    return real_vs_sampled_movie_device(model, latents, latents_gen, max_frames, n_buffer, labels_0,
                                        apply_inverse_transform, chunk_size).cpu().numpy()


# ------------------------------------------------------------------------------------------ state runs, syllable movies
def _runs_array(runs, K, lengths):
    runs = runs.detach().cpu().numpy() if torch.is_tensor(runs) else np.asarray(runs)
    runs = runs.reshape(-1, 4).astype(np.int64)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if len(runs) and (runs[:, 0].min() < 0 or runs[:, 0].max() >= len(lengths)):
        raise ValueError('discrete_chunks: the runs name trial %d of %d' % (int(runs[:, 0].max()), len(lengths)))
    if len(runs) and (runs[:, 3].min() < 0 or runs[:, 3].max() >= int(K)):
        raise ValueError('discrete_chunks: the runs name state %d of %d' % (int(runs[:, 3].max()), int(K)))
    return runs, lengths


def discrete_chunks(runs, K, lengths, include_edges=True):
    """The structure of the reference's ``get_discrete_chunks`` (plotting/arhmm_utils.py:24-68) from the rows
    ``(trial, beg, end, state)`` of ``_hip.state_runs`` / ``ARHMM.table_runs``: a list of ``K`` int64 arrays
    ``(m, 3)`` of ``[chunk, beg, end]``, the occurrences of each state in order of appearance, ``(0, 3)`` for a state
    that never occurs.  ``lengths``: the frames of every trial.  ``include_edges=False`` drops the runs that touch
    either end of their trial (``beg == 0`` or ``end == lengths[chunk]``), which is what the reference's test on its
    padded indices amounts to.  Departure: the list has the model's ``K`` entries, not ``max(state) + 1``."""
    runs, lengths = _runs_array(runs, K, lengths)
    if not include_edges and len(runs):
        runs = runs[(runs[:, 1] != 0) & (runs[:, 2] != lengths[runs[:, 0]])]
    return [runs[runs[:, 3] == k][:, :3].copy() for k in range(int(K))]


def state_durations(runs, K, lengths, include_edges=True):
    """Per state the frame counts ``end - beg`` of its runs (the reference's ``get_state_durations``,
    plotting/arhmm_utils.py:71-99): a list of ``K`` int64 arrays, and ``[]`` for a single-state model."""
    if int(K) == 1:
        return []
    return [c[:, 2] - c[:, 1] for c in discrete_chunks(runs, K, lengths, include_edges)]


def syllable_instances(chunks, min_threshold=0, seed=0):
    """Per state the instances of ``chunks`` (``discrete_chunks``) with ``end - beg > min_threshold``, shuffled
    (``make_syllable_movies_wrapper``, plotting/arhmm_utils.py:338-345).  Departure: the reference shuffles with
    numpy's global generator; here ONE ``np.random.RandomState(seed)`` shuffles the states in order, so the
    selection is reproducible."""
    rng = np.random.RandomState(seed)
    out = []
    for c in chunks:
        c = np.asarray(c, dtype=np.int64).reshape(-1, 3)
        keep = c[(c[:, 2] - c[:, 1]) > min_threshold].copy()
        if len(c):
            rng.shuffle(keep)
        out.append(keep)
    return out


def syllable_movie_plan(state_list, max_frames=400, n_buffer=5, n_pre_frames=3, n_rows=None, single_syllable=None):
    """The panels of the reference's syllable movie (``make_syllable_movies``, plotting/arhmm_utils.py:391-492), host
    only: ``(src, mark, n_rows, n_cols)``.  ``src`` int64 ``(T, n_rows, n_cols, 2)`` names per movie frame and panel
    the ``(chunk, row)`` shown, -1 for a blank panel; ``mark`` uint8 ``(T, n_rows, n_cols)`` is 1 where the reference
    draws its red box.  Panel ``i`` shows state ``i`` at ``(i // n_cols, i % n_cols)``, ``n_rows`` defaults to
    ``floor(sqrt(K))`` and ``n_cols = ceil(K / n_rows)``; with ``single_syllable`` there is one panel, for that state.

    Per panel, while fewer than ``max_frames`` frames are planned: the next instance ``[chunk, beg, end]`` of the
    state gives the rows ``max(beg - n_pre_frames, 0) .. end - 1`` -- the clip frames ``i`` with ``min(n_pre_frames,
    beg) <= i < min(n_pre_frames, beg) + 2`` are marked -- and ``n_buffer`` blanks; without instances left, one
    blank.  A clip is never cut, so a panel may pass ``max_frames``; ``T`` is the longest panel, shorter ones and
    states without instances are blank.  ValueError where no state has an instance, and where ``single_syllable``
    names a state without any."""
    who = 'syllable_movie_plan'
    max_frames, n_buffer, n_pre_frames = int(max_frames), int(n_buffer), int(n_pre_frames)
    if max_frames < 1 or n_buffer < 0 or n_pre_frames < 0:
        raise ValueError('%s: max_frames %d, n_buffer %d, n_pre_frames %d' % (who, max_frames, n_buffer, n_pre_frames))
    lists = [np.asarray(c, dtype=np.int64).reshape(-1, 3) for c in state_list]
    if single_syllable is not None:
        k = int(single_syllable)
        if not 0 <= k < len(lists) or not len(lists[k]):
            raise ValueError('%s: state %d has no instances' % (who, k))
        shown, n_rows = [k], 1
    else:
        shown = list(range(len(lists)))
    if not any(len(lists[k]) for k in shown):
        raise ValueError('%s: no state has an instance' % who)
    n_rows = int(np.floor(np.sqrt(len(shown)))) if n_rows is None else int(n_rows)
    if n_rows < 1:
        raise ValueError('%s: n_rows is %d' % (who, n_rows))
    n_cols = int(np.ceil(len(shown) / n_rows))
    panels = []
    for k in shown:
        rows = []                                         # (chunk, row, mark) per frame of the panel
        used = 0
        while len(lists[k]) and len(rows) < max_frames:
            if used >= len(lists[k]):
                rows.append((-1, -1, 0))
                continue
            chunk, beg, end = (int(v) for v in lists[k][used])
            first = max(beg - n_pre_frames, 0)
            start = min(n_pre_frames, beg)
            rows.extend((chunk, r, 1 if start <= r - first < start + 2 else 0) for r in range(first, end))
            rows.extend([(-1, -1, 0)] * n_buffer)
            used += 1
        panels.append(rows)
    n_t = max(len(rows) for rows in panels)
    src = np.full((n_t, n_rows, n_cols, 2), -1, dtype=np.int64)
    mark = np.zeros((n_t, n_rows, n_cols), dtype=np.uint8)
    for i, rows in enumerate(panels):
        if rows:
            a = np.asarray(rows, dtype=np.int64)
            src[:len(a), i // n_cols, i % n_cols] = a[:, :2]
            mark[:len(a), i // n_cols, i % n_cols] = a[:, 2]
    return src, mark, n_rows, n_cols


SYLLABLE_BOX = (5, 5, 10, 10)            # the reference's Rectangle((5, 5), 10, 10): rows and columns 5 .. 14
SYLLABLE_BOX_VALUE = 255


def syllable_movie_device(trial_frames, state_list, max_frames=400, n_buffer=5, n_pre_frames=3, n_rows=None,
                          single_syllable=None, chunk_size=200, device=None):
    """The frames of the reference's syllable movie (``make_syllable_movies``, plotting/arhmm_utils.py:360-511):
    ``(movie, mark)``, the uint8 DEVICE movie ``(T, n_rows * C * H, n_cols * W)`` and the host plan's ``mark``
    ``(T, n_rows, n_cols)`` (``syllable_movie_plan``).  Panel ``i`` plays the instances ``state_list[i]`` of state
    ``i`` (``syllable_instances``) one after the other, ``n_pre_frames`` frames of lead-in before and ``n_buffer``
    blank frames after each; the channels of a frame are stacked vertically, as the reference's
    ``np.concatenate(..., axis=1)`` stacks them.

    ``trial_frames[chunk]`` -- or ``trial_frames(chunk)`` for a callable -- is the ``(T_chunk, C, H, W)`` uint8 or
    fp32 array or tensor of the trial ``chunk`` counts; only the chunks the plan names are asked for.  The rows the
    clips show, and only those, are stacked into one device table, viewed as planes ``(P * C, 1, H, W)`` and tiled by
    one mosaic launch per ``chunk_size`` movie frames.  ONE ``stamp_boxes_u8`` launch then sets rows and columns
    5 .. 14 of every marked panel to 255 -- the reference's red ``Rectangle((5, 5), 10, 10)`` in grey; ``mark`` is
    returned so a caller can draw it in colour instead."""
    who = 'syllable_movie'
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise ValueError('%s: chunk_size %d' % (who, chunk_size))
    src, mark, n_rows, n_cols = syllable_movie_plan(state_list, max_frames, n_buffer, n_pre_frames, n_rows,
                                                    single_syllable)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    n_t = src.shape[0]
    shown = src[..., 0] >= 0
    pairs = np.unique(src[shown], axis=0)                            # (chunk, row), sorted by chunk, then row
    index = np.full(src.shape[:3], -1, dtype=np.int64)
    # (np.unique's order is the lexicographic one searchsorted needs on chunk * big + row)
    big = int(pairs[:, 1].max()) + 1
    index[shown] = np.searchsorted(pairs[:, 0] * big + pairs[:, 1], src[shown][:, 0] * big + src[shown][:, 1])
    parts, dims, dtype = [], None, None
    for chunk in np.unique(pairs[:, 0]):
        frames = trial_frames(int(chunk)) if callable(trial_frames) else trial_frames[int(chunk)]
        rows = pairs[pairs[:, 0] == chunk, 1]
        if not torch.is_tensor(frames):
            frames = np.asarray(frames)
        if frames.ndim != 4:
            raise ValueError('%s: the frames of trial %d must be (T, C, H, W), got %s'
                             % (who, chunk, tuple(frames.shape)))
        if int(rows.max()) >= frames.shape[0]:
            raise ValueError('%s: an instance of trial %d ends at frame %d, the trial has %d'
                             % (who, chunk, int(rows.max()) + 1, frames.shape[0]))
        if torch.is_tensor(frames):
            picked = frames.index_select(0, torch.from_numpy(rows).to(frames.device)).to(device)
        else:
            picked = torch.from_numpy(np.ascontiguousarray(frames[rows])).to(device)
        if picked.dtype not in (torch.uint8, torch.float32):
            raise ValueError('%s: frames must be uint8 or float32, got %s' % (who, picked.dtype))
        if dims is None:
            dims, dtype = tuple(picked.shape[1:]), picked.dtype
        elif tuple(picked.shape[1:]) != dims or picked.dtype != dtype:
            raise ValueError('%s: trial %d has frames %s %s, the first trial shown %s %s'
                             % (who, chunk, picked.dtype, tuple(picked.shape[1:]), dtype, dims))
        parts.append(picked)
    table = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    P, C, H, W = table.shape
    planes = table.contiguous().view(P * C, 1, H, W)

    def src_of(beg, end):
        # mosaic row r * C + c of column q shows channel c of the frame of panel (r, q): plane s * C + c
        s = index[beg:end][:, :, None, :]                                             # (t, n_rows, 1, n_cols)
        out = np.where(s >= 0, s * C + np.arange(C)[None, None, :, None], -1)         # (t, n_rows, C, n_cols)
        return out.reshape(end - beg, n_rows * C, n_cols).astype(np.int32)
    movie = _mosaic_in_chunks(planes, src_of, n_t, 0, None, chunk_size)
    _hip.stamp_boxes_u8(movie, mark, (C * H, W), SYLLABLE_BOX, SYLLABLE_BOX_VALUE)
    return movie, mark


def syllable_movie(trial_frames, state_list, max_frames=400, n_buffer=5, n_pre_frames=3, n_rows=None,
                   single_syllable=None, chunk_size=200, device=None):
    """``syllable_movie_device`` with the movie as a numpy array ``(T, n_rows * C * H, n_cols * W)`` of uint8."""
    movie, mark = syllable_movie_device(trial_frames, state_list, max_frames, n_buffer, n_pre_frames, n_rows,
                                        single_syllable, chunk_size, device)
    return movie.cpu().numpy(), mark
