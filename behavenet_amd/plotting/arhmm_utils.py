"""Syllable movies and state-run statistics of a fitted ARHMM (``behavenet/plotting/arhmm_utils.py``:
``get_discrete_chunks``, ``get_state_durations``, ``make_syllable_movies_wrapper`` / ``make_syllable_movies``).

The reference pads and differences every trial's state path on the host and then calls ``imshow`` once per panel and
movie frame.  Here the Viterbi table stays on the device: one launch set turns it into runs
(``_hip.state_runs``), the panels are planned on the host from those few rows (``fitting.eval.syllable_movie_plan``),
the clips' frames are tiled by the uint8 mosaic and the marker boxes are stamped by one launch; only the movie
crosses to the host.  Figures, titles and movie files are the caller's: ``imshow(movie[t], cmap='gray', vmin=0,
vmax=255)``.  Nothing here imports matplotlib."""

import numpy as np
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting import eval as _eval
from behavenet_amd.fitting.eval import discrete_chunks, syllable_instances, syllable_movie

__all__ = ['get_discrete_chunks', 'get_state_durations', 'make_syllable_movies']


def get_discrete_chunks(states, include_edges=True, device=None):
    """The occurrences of every discrete state in ``states``, a list of per-trial host arrays of states: a list of
    ``max(state) + 1`` int64 arrays ``(m, 3)`` of ``[chunk number, starting index, ending index]`` (exclusive), as the
    reference returns them; a state that never occurs has shape ``(0, 3)`` (the reference: ``(0,)``).  The trials are
    uploaded as one int32 table and ``_hip.state_runs`` finds the runs; ``include_edges=False`` drops the runs at
    either end of a trial.  A negative state, or one beyond the ``_hip.ARHMM_MAX_K`` the kernels serve, is a
    ValueError."""
    trials = [np.asarray(x).reshape(-1) for x in states]
    lengths = np.asarray([len(x) for x in trials], dtype=np.int64)
    if not lengths.sum():
        raise ValueError('get_discrete_chunks: the trials have no frames')
    table = np.concatenate(trials)
    if not np.issubdtype(table.dtype, np.integer):
        if np.any(table != np.rint(table)):
            raise ValueError('get_discrete_chunks: states must be integers')
    K = int(table.max()) + 1
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    runs, _, _ = _hip.state_runs(torch.from_numpy(table.astype(np.int32)).to(device), offsets, max(K, 1))
    return discrete_chunks(runs, K, lengths, include_edges)


def get_state_durations(latents, arhmm, include_edges=True):
    """The frame count of every state run of the trials ``latents`` (a list of (T, D) arrays; empty ones are left
    out) under ``arhmm``: per state an int64 array, ``[]`` for a single-state model.  As in the reference the list
    has ``max(state) + 1`` entries.  One ``ARHMM.table_runs`` call: the states never reach the host."""
    if arhmm.K == 1:
        return []
    trials = [x for x in latents if len(x) > 0]
    table, offsets = arhmm.as_table(trials)
    runs, _, _ = arhmm.table_runs(table, offsets)
    K = int(runs[:, 3].max()) + 1 if len(runs) else 0
    # (state_durations is this line for the model's K entries)
    return [c[:, 2] - c[:, 1] for c in discrete_chunks(runs, K, np.diff(offsets), include_edges)]


def make_syllable_movies(model, data_generator, arhmm, sess_idx=0, dtype='test', max_frames=400, min_threshold=0,
                         n_buffer=5, n_pre_frames=3, n_rows=None, single_syllable=None, data_key='ae_latents', seed=0,
                         save_file=None):
    """The syllable movie of the ``dtype`` trials of session ``sess_idx`` as a uint8 array
    ``(T, n_rows * C * H, n_cols * W)``: one panel per state of ``arhmm`` (or the one of ``single_syllable``) playing
    the video clips of the state's runs longer than ``min_threshold`` frames, in an order shuffled by ``seed``,
    ``n_pre_frames`` frames of lead-in before each and ``n_buffer`` blank frames after; a grey box (rows and columns
    5 .. 14 at 255) marks the first two frames of every instance.  Where the reference loads the models and the
    data from ``hparams``, this takes them as they are.

    The trials' latents (encoded by ``model``) or, for ``data_key='labels'``, their labels go into ONE device table;
    log-likelihoods, Viterbi and the run search stay on the device (``ARHMM.table_runs``).  The frames of the trials
    the plan names are taken from ``data_generator`` as stored (uint8 where it stores uint8).  ``save_file``: written
    with ``np.save``."""
    who = 'make_syllable_movies'
    if not isinstance(dtype, str):
        raise ValueError("%s: dtype must be 'train', 'val' or 'test', got %r" % (who, dtype))
    _eval._splits(who, dtype)
    if data_key == 'ae_latents' and model is not None:
        _eval._export_setup(model)
    wanted = _eval._wanted_sessions(who, data_generator, int(sess_idx))
    sess_idx = int(sess_idx)
    parts = _eval._arhmm_trials(who, data_generator, model, data_key, (dtype,), wanted)
    idxs = [ds.batch_idxs for ds in data_generator.datasets]
    table, offsets, _, trials = _eval._arhmm_split(parts, _eval._corr_trial_order(idxs, [dtype], wanted))
    if table is None:
        raise ValueError('%s: no latents for dtype=%s' % (who, dtype))
    runs, _, _ = arhmm.table_runs(table, offsets)
    chunks = discrete_chunks(runs, arhmm.K, np.diff(offsets), include_edges=True)
    instances = syllable_instances(chunks, min_threshold=min_threshold, seed=seed)

    def frames_of(chunk):
        # (stored uint8 frames are handed out as they are: the mosaic takes grey levels)
        serve_prev = getattr(data_generator, 'serve_uint8', None)
        if serve_prev is not None:
            data_generator.serve_uint8 = True
        try:
            batch = data_generator._sample(sess_idx, int(trials[chunk]), dtype)
        finally:
            if serve_prev is not None:
                data_generator.serve_uint8 = serve_prev
        return batch['images'][0]
    movie, _ = syllable_movie(frames_of, instances, max_frames=max_frames, n_buffer=n_buffer,
                              n_pre_frames=n_pre_frames, n_rows=n_rows, single_syllable=single_syllable,
                              device=table.device)
    if save_file is not None:
        np.save(save_file, movie)
    return movie
