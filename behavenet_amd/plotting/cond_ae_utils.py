"""Latent and label traversals with the reference's signatures (``behavenet/plotting/cond_ae_utils.py``:
``interpolate_1d``, ``interpolate_2d``, ``interpolate_point_path``), decoded in ONE batch, the frames of the
session-swap movie (``make_session_swap_movie``), tiled on the device, the ranges they sweep (``get_input_range``,
``compute_range``), selected on the device, the per-trial label scores of the models with supervised latents
(``get_label_r2``) and the correlations of the unsupervised latents (``get_latent_corr``), reduced on the device, and
the session classifier on the latents (``fit_classifier``), fitted on the device.

The reference calls ``get_reconstruction`` once per point: P launch chains of one frame and P copies to the host.
Here the points are collected into one table (``fitting.eval.traversal_points``) and ``get_reconstruction`` is called
once on it; the lists that come back have the reference's nesting and dtypes.  For an image instead of lists --
cropped, quantised and tiled on the device, with only the uint8 result crossing to the host -- see
``fitting.eval.traverse_latents``, ``traversal_movie`` and ``point_path_movie``.  Nothing here imports
matplotlib."""

import os
import pickle

import numpy as np
import torch

from behavenet_amd.fitting import distributed as _bdist
from behavenet_amd.fitting import eval as _eval
from behavenet_amd.fitting.eval import get_reconstruction, path_points, traversal_points
from behavenet_amd.plotting import get_crop

__all__ = ['interpolate_1d', 'interpolate_2d', 'interpolate_point_path', 'make_session_swap_movie', 'get_input_range',
           'compute_range', 'get_label_r2', 'get_latent_corr', 'fit_classifier']

_PLAIN = ('ae', 'vae', 'beta-tcvae', 'ps-vae', 'msps-vae')
_COND = ('cond-ae', 'cond-vae')
_MSP = ('cond-ae-msp', 'ps-vae', 'msps-vae')


def _get_updated_scaled_labels(labels_og, idxs=None, vals=None):
    """A copy ``(1, n)`` of the scaled labels with ``labels_sc[0, idx] = val`` for every pair of ``idxs`` / ``vals``
    (one int and one float, or two sequences of equal length); None stays None.  4-d one-hot maps ``(1, L, H, W)``
    are read back as coordinates first: the x of every hot pixel, then the y (ref cond_ae_utils.py:847-874)."""
    if labels_og is None:
        return None
    labels_og = np.asarray(labels_og)
    if labels_og.ndim == 4:
        _, y, x = np.where(labels_og[0] == 1)
        labels_sc = np.hstack([x, y])[None, :]
    else:
        labels_sc = np.copy(labels_og)
    if idxs is not None:
        if isinstance(idxs, (int, np.integer)):
            assert isinstance(vals, (float, np.floating))
            idxs, vals = [idxs], [vals]
        assert len(idxs) == len(vals)
        for idx, val in zip(idxs, vals):
            labels_sc[0, idx] = val
    return labels_sc


def _device_of(model):
    return next(model.parameters()).device


def _interpolate(mode, interp_type, model, ims_0, latents_0, labels_0, labels_sc_0, mins, maxes, input_idxs, n_frames,
                 crop_type, mins_sc, maxes_sc, crop_kwargs, marker_idxs, ch):
    cls = model.hparams['model_class']
    if interp_type not in ('latents', 'labels'):
        raise NotImplementedError('interp_type must be "latents" or "labels", got %r' % (interp_type,))
    if mode == '2d':
        assert len(input_idxs) == 2
    inputs_sc = None
    if mins_sc is not None and maxes_sc is not None:
        inputs_sc = [np.linspace(mins_sc[d], maxes_sc[d], n_frames) for d in input_idxs]
    elif interp_type == 'labels':
        raise NotImplementedError('interpolating labels needs mins_sc and maxes_sc')
    if interp_type == 'latents' and cls not in _PLAIN + _COND + ('cond-ae-msp',):
        raise NotImplementedError('model class %s' % cls)
    if interp_type == 'labels' and cls not in _MSP and np.ndim(labels_sc_0) == 4:
        raise NotImplementedError(
            'interpolating the labels of a %s with 4-d labels_sc_0 (a conditional encoder) is not served: the maps '
            'of every point would have to be built and sent through the encoder; pass 1-d scaled labels' % cls)

    # every point of the traversal in one table, one batched decode
    if interp_type == 'latents' or cls in _MSP:
        table, (rows, cols) = traversal_points(latents_0, mins, maxes, input_idxs, n_frames, mode)
        labels = None
        if cls in _COND:
            labels = torch.from_numpy(np.asarray(labels_0)).float().to(_device_of(model)).expand(table.shape[0], -1)
        ims = get_reconstruction(model, table, labels=labels, apply_inverse_transform=True)
    else:
        table, (rows, cols) = traversal_points(labels_0, mins, maxes, input_idxs, n_frames, mode)
        ims_rep = ims_0.to(_device_of(model)).expand(table.shape[0], -1, -1, -1).contiguous()
        ims = get_reconstruction(model, ims_rep, labels=torch.from_numpy(table).to(_device_of(model)), labels_2d=None)

    y_min = crop_kwargs['y_0'] - crop_kwargs['y_ext'] if crop_type else 0
    x_min = crop_kwargs['x_0'] - crop_kwargs['x_ext'] if crop_type else 0
    ims_list, labels_list, ims_crop_list = [], [], []
    for i0 in range(rows):
        ims_tmp, labels_tmp, ims_crop_tmp = [], [], []
        for i1 in range(cols):
            im = ims[i0 * cols + i1]
            ims_tmp.append(np.copy(im[ch]))
            if interp_type == 'labels':
                if mode == '1d':
                    labels_sc = _get_updated_scaled_labels(labels_sc_0, input_idxs[i0], inputs_sc[i0][i1])
                else:
                    labels_sc = _get_updated_scaled_labels(
                        labels_sc_0, input_idxs, [inputs_sc[0][i0], inputs_sc[1][i1]])
                labels_tmp.append([np.copy(labels_sc[0, input_idxs[0]]) - y_min,
                                   np.copy(labels_sc[0, input_idxs[1]]) - x_min])
            elif labels_sc_0 is not None:
                labels_sc = _get_updated_scaled_labels(labels_sc_0)
                labels_tmp.append([np.copy(labels_sc[0, marker_idxs[0]]) - y_min,
                                   np.copy(labels_sc[0, marker_idxs[1]]) - x_min])
            else:
                labels_tmp.append([np.nan, np.nan])
            if crop_type:
                # (the reference crops channel 0 whatever ``ch`` says; kept)
                ims_crop_tmp.append(get_crop(
                    im[0], crop_kwargs['y_0'], crop_kwargs['y_ext'], crop_kwargs['x_0'], crop_kwargs['x_ext']))
            else:
                ims_crop_tmp.append([])
        ims_list.append(ims_tmp)
        labels_list.append(labels_tmp)
        ims_crop_list.append(ims_crop_tmp)
    return ims_list, labels_list, ims_crop_list


def interpolate_2d(
        interp_type, model, ims_0, latents_0, labels_0, labels_sc_0, mins, maxes, input_idxs,
        n_frames, crop_type=None, mins_sc=None, maxes_sc=None, crop_kwargs=None,
        marker_idxs=None, ch=0):
    """Reconstructions on the ``n_frames x n_frames`` grid spanned by two latents (``interp_type='latents'``) or two
    labels (``'labels'``) between ``mins`` and ``maxes``, the reference's ``interpolate_2d`` (cond_ae_utils.py:346-540)
    with its parameters in its order.  Returns ``(ims_list, labels_list, ims_crop_list)``, each a list over the first
    swept dimension of lists over the second: float32 frames ``(y_pix, x_pix)`` of channel ``ch``; marker pairs
    ``[y, x]`` shifted by the crop's origin (``[nan, nan]`` without scaled labels); float64 zero-filled crops
    (``get_crop``; ``[]`` without ``crop_type``).  ``input_idxs`` for labels: y first, then x.

    Labels of a cond-ae-msp / ps-vae / msps-vae are changed in the latents and mapped back through the inverse
    transform; labels of a cond-ae / cond-vae go with ``ims_0``, repeated, through the whole model.  A cond-ae /
    cond-vae with 4-d ``labels_sc_0`` (a conditional encoder) is a NotImplementedError for ``'labels'``; so is
    ``'labels'`` without ``mins_sc`` / ``maxes_sc``, as in the reference."""
    return _interpolate('2d', interp_type, model, ims_0, latents_0, labels_0, labels_sc_0, mins, maxes, input_idxs,
                        n_frames, crop_type, mins_sc, maxes_sc, crop_kwargs, marker_idxs, ch)


def interpolate_1d(
        interp_type, model, ims_0, latents_0, labels_0, labels_sc_0, mins, maxes, input_idxs,
        n_frames, crop_type=None, mins_sc=None, maxes_sc=None, crop_kwargs=None,
        marker_idxs=None, ch=0):
    """One row of ``n_frames`` reconstructions per entry of ``input_idxs``, that latent (or label) alone swept between
    its ``mins`` and ``maxes``: the reference's ``interpolate_1d`` (cond_ae_utils.py:543-730) with its parameters in
    its order.  Returns and refusals as ``interpolate_2d``; the marker pair of a label traversal is read at
    ``input_idxs[0]`` and ``input_idxs[1]``, as there."""
    return _interpolate('1d', interp_type, model, ims_0, latents_0, labels_0, labels_sc_0, mins, maxes, input_idxs,
                        n_frames, crop_type, mins_sc, maxes_sc, crop_kwargs, marker_idxs, ch)


def interpolate_point_path(
        interp_type, model, ims_0, labels_0, points, n_frames=10, ch=0, crop_kwargs=None,
        apply_inverse_transform=True):
    """Reconstructions along the path through ``points`` (n_points, D): the reference's ``interpolate_point_path``
    (cond_ae_utils.py:733-844), what its traversal movies play, with its parameters in its order.  Every leg has
    ``n_frames + 1`` steps, both ends included (``n_frames``: an int, or one per leg; another length is its
    AssertionError; ``fitting.eval.path_points``).  Returns ``(ims_list, inputs_list)``: per step a float32 frame
    ``(y_pix, x_pix)`` of channel ``ch`` -- with a non-int ``ch`` all channels next to each other, ``(y_pix, C *
    x_pix)``; with ``crop_kwargs`` the float64 zero-filled ``get_crop`` of channel ``ch``, where a non-int ``ch`` is
    the reference's ValueError -- and the step's point ``(1, D)`` in the dtype of ``points``.

    ``'latents'``: the points are latents (``labels_0`` (1, L) goes with them for a cond-ae / cond-vae;
    ``apply_inverse_transform`` as in ``get_reconstruction``).  ``'labels'``: the points are the transformed latents of
    a cond-ae-msp / ps-vae / msps-vae, mapped back, or the labels of a cond-ae / cond-vae, which go with ``ims_0``,
    repeated, through the whole model.  Where the reference calls ``get_reconstruction`` once per step, this makes ONE
    batched call on the table.  ``hparams['conditional_encoder']`` is a NotImplementedError, as there."""
    if model.hparams.get('conditional_encoder', False):
        raise NotImplementedError
    if interp_type not in ('latents', 'labels'):
        raise NotImplementedError
    if crop_kwargs is not None and not isinstance(ch, int):
        raise ValueError('"ch" must be an integer to use crop_kwargs')
    cls = model.hparams['model_class']
    table = path_points(points, n_frames)
    ims_list, inputs_list = [], []
    if len(table) == 0:
        return ims_list, inputs_list
    if interp_type == 'latents':
        labels = None
        if cls in _COND:
            labels = torch.from_numpy(np.asarray(labels_0)).float().to(_device_of(model)).expand(table.shape[0], -1)
        ims = get_reconstruction(model, table, labels=labels, apply_inverse_transform=apply_inverse_transform)
    elif cls in _MSP:
        ims = get_reconstruction(model, table, apply_inverse_transform=True)
    else:
        ims_0 = ims_0 if torch.is_tensor(ims_0) else torch.from_numpy(np.asarray(ims_0))
        ims_rep = ims_0.float().to(_device_of(model)).expand(table.shape[0], -1, -1, -1).contiguous()
        ims = get_reconstruction(model, ims_rep, labels=torch.from_numpy(table).float().to(_device_of(model)))
    for im, vec in zip(ims, table):
        if crop_kwargs is not None:
            ims_list.append(get_crop(
                im[ch], crop_kwargs['y_0'], crop_kwargs['y_ext'], crop_kwargs['x_0'], crop_kwargs['x_ext']))
        elif isinstance(ch, int):
            ims_list.append(np.copy(im[ch]))
        else:
            ims_list.append(np.concatenate(list(im), axis=1))
        inputs_list.append(np.copy(vec[None]))
    return ims_list, inputs_list


def make_session_swap_movie(
        model, data_generator, n_labels, n_background, sess_idx, trials, trial_idxs=None, n_buffer_frames=5,
        layout_pattern=None, save_file=None, max_frames=400):
    """The frames of the reference's ``make_session_swap_movie`` (cond_ae_utils.py:3030-3156): trials of session
    ``sess_idx`` re-rendered with every session's median background latents, one panel per session (the trial's own
    session first), all channels side by side, ``n_buffer_frames`` black frames between trials -- a uint8 array
    ``(T, n_rows * H, n_cols * C * W)`` (``fitting.eval.session_swap_movie``: decoded and tiled on the device).

    The model and the generator are taken as they are (as ``fit_classifier`` and ``get_label_r2`` take them) instead
    of being rebuilt from ``hparams`` and ``version``; the figure, titles and ffmpeg are not served.  The background
    columns are ``n_labels .. n_labels + n_background - 1`` and every session's median comes from
    ``fitting.eval.latent_ranges(..., sess_idx=s, min_p=15, max_p=85)['med']``, the reference's percentiles.
    ``trials`` are trial numbers of the session; an entry of ``trial_idxs`` indexes its test trials
    (``batch_idxs['test'][trial_idx]``) and is used where the entry of ``trials`` is None; one of the two lists may be
    None.  Of every trial the first ``max_frames`` frames are taken; their latents come from
    ``get_transformed_latents`` for a cond-ae-msp / ps-vae / msps-vae and from ``get_reconstruction(...,
    return_latents=True)`` otherwise, and are decoded without the inverse transform, as the reference decodes them.
    ``save_file``: the array is also written there with ``np.save``.  Under ``torch.distributed`` rank 0 alone
    works; the other ranks return None."""
    if _bdist.world_size() > 1 and _bdist.rank() != 0:
        return None
    if trial_idxs is None:
        trial_idxs = [None] * len(trials)
    if trials is None:
        trials = [None] * len(trial_idxs)
    if len(trials) != len(trial_idxs) or not len(trials):
        raise ValueError('make_session_swap_movie: %d trials and %d trial_idxs' % (len(trials), len(trial_idxs)))
    for trial, trial_idx in zip(trials, trial_idxs):
        if (trial is None) == (trial_idx is None):
            raise ValueError('make_session_swap_movie: exactly one of a trial and its trial_idx must be given, '
                             'got %r and %r' % (trial, trial_idx))
    n_sessions = len(data_generator.datasets)
    _eval.swap_layout(n_sessions, sess_idx, layout_pattern)          # (a layout error before anything is encoded)
    dataset = data_generator.datasets[sess_idx]
    numbers = [int(dataset.batch_idxs['test'][trial_idx]) if trial is None else int(trial)
               for trial, trial_idx in zip(trials, trial_idxs)]
    background_idxs = np.arange(n_labels, n_labels + n_background)
    medians = _eval.background_medians(data_generator, model, background_idxs, min_p=15, max_p=85)
    cls = model.hparams['model_class']
    latents = []
    model.eval()
    for trial in numbers:
        batch = data_generator._sample(sess_idx, trial, 'test')          # (the trial as the generator serves it)
        ims = batch['images'][0][:max_frames]
        ims = ims if torch.is_tensor(ims) else torch.from_numpy(np.asarray(ims))
        ims = (ims.float() / 255 if ims.dtype == torch.uint8 else ims).to(_device_of(model))
        if cls in _MSP:
            with torch.no_grad():
                latents.append(model.get_transformed_latents(ims, dataset=sess_idx, as_numpy=True))
        else:
            labels = batch['labels'][0][:max_frames] if cls in _COND else None
            latents.append(get_reconstruction(model, ims, dataset=sess_idx, labels=labels, return_latents=True)[1])
    movie = _eval.session_swap_movie(model, latents, background_idxs, medians, sess_idx=sess_idx,
                                     n_buffer_frames=n_buffer_frames, layout_pattern=layout_pattern,
                                     apply_inverse_transform=False)
    if save_file is not None:
        np.save(save_file, movie)
    return movie


# ------------------------------------------------------------------------------------------ ranges
def compute_range(values_list, min_p=5, max_p=95):
    """The ``min_p``-th, ``max_p``-th and 50th percentile of every column of the vertically stacked ``values_list``,
    NaNs ignored: ``{'min', 'max', 'med'}``, each a ``(D,)`` float32 array -- the reference's ``compute_range``
    (cond_ae_utils.py:148-178) with its parameters, and ``np.nanpercentile``'s float32 numbers bit for bit.

    The entries are numpy arrays or device tensors ``(n_i, D)``; entries of length 0 (the gap trials of a latents
    pickle) are skipped; numpy entries are stacked and uploaded once and anything else is made float32.  The three
    percentiles come from ONE count and ONE select call on the device table (``fitting.eval.column_percentiles``:
    exact order statistics by a radix select, csrc/column_select.hip); the valid counts and the six selected
    neighbours of every column are all that comes back.  There is no CPU fallback."""
    return _eval.compute_range(values_list, min_p=min_p, max_p=max_p)


def _session_list(sess_idx):
    return [int(s) for s in sess_idx] if isinstance(sess_idx, (list, tuple, np.ndarray)) else [sess_idx]


def _latents_file(hparams, sess_ids, s_idx, version):
    ids = sess_ids[s_idx] if (sess_ids is not None and s_idx is not None) else hparams
    name = '%s_%s_%s_%s_latents.pkl' % (ids['lab'], ids['expt'], ids['animal'], ids['session'])
    return os.path.join(hparams['expt_dir'], 'version_%i' % version, name)


def _trial_signal(dataset, signal, trial):
    """One trial's ``signal`` (T, L) as a float32 numpy array from a session of a data generator: read from a
    file-backed session's store with its transform applied, or taken from a synthetic session's list."""
    if hasattr(dataset, 'read') and signal in getattr(dataset, 'signals', ()):
        arr = np.asarray(dataset.read(signal, trial)).astype(np.float32)
        transform = dataset.transforms.get(signal)
        return transform(arr) if transform else arr
    trials = getattr(dataset, signal, None)
    if trials is None:
        raise KeyError(signal)
    arr = trials[trial]
    return (arr.detach().cpu().numpy() if torch.is_tensor(arr) else np.asarray(arr)).astype(np.float32)


def _session_signal(data_gen, signal, sessions):
    out = []
    for s_idx in sessions:
        dataset = data_gen.datasets[0 if s_idx is None else s_idx]
        for dtype in ('train', 'val', 'test'):
            out.extend(_trial_signal(dataset, signal, int(t)) for t in dataset.batch_idxs[dtype])
    return out


def get_input_range(input_type, hparams, sess_ids=None, sess_idx=0, model=None, data_gen=None, version=0, min_p=5,
                    max_p=95, apply_label_masks=False):
    """The range of one kind of input, ``{'min', 'max', 'med'}`` (``compute_range``), with the reference's signature
    (cond_ae_utils.py:43-145).

    ``'latents'``: from the latents pickle(s) of session ``sess_idx`` (one index or a list) in
    ``hparams['expt_dir']/version_<version>`` where they exist -- named by ``sess_ids[sess_idx]``, or by ``hparams``
    without ``sess_ids`` -- and otherwise from ``fitting.eval.latent_ranges(data_gen, model, sess_idx)``, which
    encodes the trials as ``export_latents`` would and gives the same numbers without writing and re-reading a file.
    ``'labels'`` / ``'labels_sc'``: that signal of every train, val and test trial of the session(s), taken from
    ``data_gen`` -- the reference rebuilds a generator from ``hparams``; here ``data_gen`` is required (ValueError
    without it).  ``apply_label_masks`` sets the labels whose ``labels_masks`` entry is 0 to NaN first, and NaNs take
    no part in a percentile.  Any other ``input_type`` is a NotImplementedError."""
    sessions = _session_list(sess_idx)
    if input_type == 'latents':
        files = [_latents_file(hparams, sess_ids, s_idx, version) for s_idx in sessions]
        if all(os.path.exists(f) for f in files):
            inputs = []
            for f in files:
                with open(f, 'rb') as fh:
                    inputs += list(pickle.load(fh)['latents'])
            return compute_range(inputs, min_p=min_p, max_p=max_p)
        if model is None or data_gen is None:
            raise ValueError('get_input_range: no latents file at %s; pass model and data_gen to compute the latents'
                             % [f for f in files if not os.path.exists(f)][0])
        return _eval.latent_ranges(data_gen, model, sess_idx, min_p=min_p, max_p=max_p)
    if input_type not in ('labels', 'labels_sc'):
        raise NotImplementedError(input_type)
    if data_gen is None:
        raise ValueError('get_input_range: %r needs data_gen, the generator that serves the session\'s %s'
                         % (input_type, input_type))
    try:
        inputs = _session_signal(data_gen, input_type, sessions)
    except KeyError:
        raise ValueError('get_input_range: data_gen does not serve %r' % input_type)
    if apply_label_masks and input_type == 'labels':
        try:
            masks = _session_signal(data_gen, 'labels_masks', sessions)
        except KeyError:
            print('no label masks!')
            masks = []
        inputs = [np.where(m == 0, np.float32(np.nan), i) for i, m in zip(inputs, masks)] if masks else inputs
    return compute_range(inputs, min_p=min_p, max_p=max_p)


# ------------------------------------------------------------------------------------------ label scores
def get_label_r2(hparams, model, data_generator, version, label_names, dtype='val', overwrite=False):
    """R^2 and MSE of every label under the model's supervised latents, per trial of the split ``dtype``: the
    reference's ``get_label_r2`` (cond_ae_utils.py:1234-1279) with its signature, its messages and its file,
    ``r2_supervised.csv`` in ``hparams['expt_dir']/version_<version>`` -- read where it exists and ``overwrite`` is
    false (neither the model nor the generator is touched then), computed and written otherwise
    (``fitting.eval.export_label_r2``: the trials' predictions and labels stay on the device, one launch reduces them,
    no sklearn call).  -> a pandas DataFrame with the columns ``Trial, Label, R2, MSE, Model`` and, after them,
    ``Session``, one row per (trial, label).  pandas is imported here, not with the package."""
    import pandas as pd
    save_file = os.path.join(hparams['expt_dir'], 'version_%i' % version, 'r2_supervised.csv')
    if not os.path.exists(save_file) or overwrite:
        if not os.path.exists(save_file):
            print('R^2 metrics do not exist; computing from scratch')
        else:
            print('overwriting metrics at %s' % save_file)
        print('saving results to %s' % save_file)
        if _eval.export_label_r2(data_generator, model, label_names=list(label_names), dtype=dtype,
                                 filename=save_file) is None:
            return None          # (torch.distributed: rank 0 alone computes and writes)
    else:
        print('loading results from %s' % save_file)
    # (round_trip: the file holds the shortest decimals that name the float64 scores, and they are read back as those)
    return pd.read_csv(save_file, float_precision='round_trip')


# ------------------------------------------------------------------------------------------ latent correlations
def get_latent_corr(hparams, model, data_generator, version, batch_size=None, dtype='train', overwrite=False):
    """The correlation of the model's unsupervised latents per batch of ``batch_size`` rows, or across all time
    points (``batch_size=None``), over the trials of the split ``dtype``: the third number of the reference's PS-VAE
    and MSPS-VAE hyperparameter searches (cond_ae_utils.py:1679-1700, 2802-2835), saved and loaded as ``get_label_r2``
    saves and loads its table.  ``corr_unsupervised.csv`` in ``hparams['expt_dir']/version_<version>`` is read where
    it exists and ``overwrite`` is false (neither the model nor the generator is touched then), computed and written
    otherwise (``fitting.eval.export_latent_correlations``: the latents stay on the device, one launch reduces them).
    -> a pandas DataFrame with the columns ``Segment, RowBegin, RowEnd, N, AbsCorr01, MeanAbsCorr``, one row per
    batch.  pandas is imported here, not with the package."""
    import pandas as pd
    save_file = os.path.join(hparams['expt_dir'], 'version_%i' % version, 'corr_unsupervised.csv')
    if not os.path.exists(save_file) or overwrite:
        if not os.path.exists(save_file):
            print('latent correlations do not exist; computing from scratch')
        else:
            print('overwriting metrics at %s' % save_file)
        print('saving results to %s' % save_file)
        if _eval.export_latent_correlations(data_generator, model, dtype=dtype, segments=batch_size,
                                            filename=save_file) is None:
            return None          # (torch.distributed: rank 0 alone computes and writes)
    else:
        print('loading results from %s' % save_file)
    # (round_trip: the file holds the shortest decimals that name the float64 values, and they are read back as those)
    return pd.read_csv(save_file, float_precision='round_trip')


# ------------------------------------------------------------------------------------------ session classifier
# the classes the reference's collect_data serves (cond_ae_utils.py:1294-1307); any other: NotImplementedError
_CLASSIFIER_CLASSES = ('ae', 'vae', 'cond-vae', 'sss-vae', 'ps-vae', 'msps-vae')


def fit_classifier(model, data_generator, dtype='val', fit_full=False, overwrite=False):
    """Fit a classifier from the latent space to the session id -- the reference's ``fit_classifier``
    (cond_ae_utils.py:1323-1369), its signature, its messages and its file: ``fc_session_classification.npy`` in
    ``model.hparams['expt_dir']/version_<model.version>`` holds ``np.array([fc])``, the fraction of the ``dtype``
    frames whose session the classifier fitted on the ``'train'`` frames recovers.  The file is read where it exists
    and ``overwrite`` is false (neither the model nor the generator is touched then, and the classifier returned is
    None); otherwise ``fitting.eval.session_classifier`` fits and scores on the device.  ``fit_full=True`` takes every
    latent of a ``ps-vae`` instead of its unsupervised block; for ``msps-vae`` the reference ignores the flag
    (``collect_data``: 1304-1305), and so does this.  -> ``(fc, lr)``, ``lr`` a
    ``fitting.classifier.SessionClassifier`` with sklearn's attribute names."""
    model_class = model.hparams['model_class']
    if model_class not in _CLASSIFIER_CLASSES:
        raise NotImplementedError('fit_classifier: model class %r (served: %s)'
                                  % (model_class, ', '.join(_CLASSIFIER_CLASSES)))
    save_file = os.path.join(model.hparams['expt_dir'], 'version_%i' % model.version, _eval.SESSION_CLASSIFIER_FILE)
    if not os.path.exists(save_file) or overwrite:
        if not os.path.exists(save_file):
            print('FC metrics do not exist; computing from scratch')
        else:
            print('overwriting metrics at %s' % save_file)
        columns = None          # (the unsupervised block of ps-vae / msps-vae, every latent otherwise)
        if model_class in ('sss-vae', 'ps-vae') and fit_full:
            columns = slice(None)
        elif model_class == 'sss-vae':          # (the ps-vae's earlier name: the same block)
            columns = slice(int(model.hparams['n_labels']), None)
        # (the reference's messages; its four stages are one call here, so one 'done' closes them all)
        print('collecting training labels and latents')
        print('collecting %s labels and latents' % dtype)
        print('fitting linear classifier model with training data')
        print('computing fraction correct on %s data' % dtype)
        out = _eval.session_classifier(data_generator, model, dtype=dtype, columns=columns)
        if out is None:
            return None          # (torch.distributed: rank 0 alone computes and writes)
        fc, lr = out
        print('done')
        print('saving results to %s' % save_file)
        np.save(save_file, np.array([fc]))
    else:
        print('loading results from %s' % save_file)
        fc = np.load(save_file)[0]
        lr = None
    return fc, lr
