"""The reconstruction movie of an autoencoder (``behavenet/plotting/ae_utils.py``:
``make_ae_reconstruction_movie_wrapper``) as a uint8 array.

The reference copies the fp32 reconstruction to the host, builds the three fp32 arrays original, reconstruction and
``0.5 + (original - reconstruction)`` and lets matplotlib clip and colour them frame by frame.  Here the forward pass
feeds one launch per chunk that writes the three panels as grey levels (``fitting.eval.reconstruction_movie``), and
only the movie crosses to the host.  Figures, titles and movie files are the caller's: ``imshow(movie[t], cmap='gray',
vmin=0, vmax=255)``.  Nothing here imports matplotlib."""

import numpy as np
import torch

from behavenet_amd.fitting.eval import reconstruction_movie

__all__ = ['make_ae_reconstruction_movie']


def make_ae_reconstruction_movie(model, data_generator, trial=None, sess_idx=0, linear_model=None, max_frames=400,
                                 save_file=None):
    """The movie of one trial as a uint8 array ``(T, R * H, 3 * C * W)``: original, reconstruction and residual next
    to each other, ``T = min(frames of the trial, max_frames)``; with ``linear_model`` (the reference's
    ``include_linear``: the matching linear AE) a second row with a black first panel, its reconstruction and its
    residual.  Where the reference loads the models and the data from ``hparams``, this takes them as they are.

    ``trial``: None picks the first test trial of session ``sess_idx``, as the reference does.  The batch's ``masks``
    multiply the original when ``hparams['use_output_mask']`` is set; a ``cond-ae`` gets the batch's ``labels``, and
    its ``labels_sc`` when it has a conditional encoder.  ``save_file``: written with ``np.save`` (``.npy`` is
    appended to a name without it)."""
    hparams = model.hparams
    cls = hparams['model_class']
    dataset = data_generator.datasets[sess_idx]
    if trial is None:
        trial = dataset.batch_idxs['test'][0]
    trial = int(trial)
    cond_enc = cls == 'cond-ae' and hparams.get('conditional_encoder', False)
    # (stored uint8 frames are handed out as they are: reconstruction_movie converts for the models that need it)
    serve_prev = getattr(data_generator, 'serve_uint8', None)
    if serve_prev is not None:
        data_generator.serve_uint8 = True
    try:
        batch = data_generator._sample(sess_idx, trial, 'test')
    finally:
        if serve_prev is not None:
            data_generator.serve_uint8 = serve_prev
    images = batch['images'][0]
    if not torch.is_tensor(images):
        images = torch.from_numpy(np.asarray(images))
    dev = next(model.parameters()).device

    def signal(name):
        value = batch[name][0]
        value = value if torch.is_tensor(value) else torch.from_numpy(np.asarray(value))
        return value.to(dev)
    masks = signal('masks') if hparams.get('use_output_mask', False) else None
    labels = signal('labels') if cls in ('cond-ae', 'cond-vae') else None
    labels_2d = signal('labels_sc') if cond_enc else None
    movie = reconstruction_movie(model, images.to(dev), sess_idx, masks=masks, labels=labels, labels_2d=labels_2d,
                                 max_frames=max_frames,
                                 extra_models=() if linear_model is None else (linear_model,))
    if save_file is not None:
        np.save(save_file, movie)
    return movie
