"""The yardstick of the traversal tests: the semantics of the reference's ``interpolate_1d`` / ``interpolate_2d``,
``get_crop``, ``plot_2d_frame_array`` and ``make_latent_traversal_movie`` restated in plain numpy (no tests here).

Each thing is written twice, independently, and tests/test_traversals_cpu.py holds the two against each other:

* the point table as the reference's nested loop over panels (``points_loop``) and in closed form (``points_closed``);
* the panel image as a crop of every quantised frame put together with ``np.block`` (``mosaic_blocks``) and as the
  index rule of the kernel's header, one output pixel at a time (``mosaic_index_rule``).

Quantisation is ``tests.recon_u8_refs.quantise_u8``."""

import numpy as np
import torch

from tests.recon_u8_refs import quantise_u8


# ------------------------------------------------------------------------------------------ the point table
def sweep_values(mins, maxes, input_idxs, n_frames):
    return [np.linspace(mins[d], maxes[d], n_frames) for d in input_idxs]


def grid_shape(input_idxs, n_frames, mode):
    return (len(input_idxs), n_frames) if mode == '1d' else (n_frames, n_frames)


def points_loop(base, mins, maxes, input_idxs, n_frames, mode):
    """Panel by panel, as the reference walks them: copy the base (1, D), overwrite, cast as torch does."""
    base = np.asarray(base).reshape(1, -1)
    vals = sweep_values(mins, maxes, input_idxs, n_frames)
    rows, cols = grid_shape(input_idxs, n_frames, mode)
    out = []
    for i0 in range(rows):
        for i1 in range(cols):
            point = np.copy(base)
            if mode == '1d':
                point[0, input_idxs[i0]] = vals[i0][i1]
            else:
                point[0, input_idxs[0]] = vals[0][i0]
                point[0, input_idxs[1]] = vals[1][i1]
            out.append(torch.from_numpy(point).float().numpy()[0])
    return np.stack(out), (rows, cols)


def points_closed(base, mins, maxes, input_idxs, n_frames, mode):
    """Row p is panel divmod(p, cols); the swept columns are written by fancy indexing, nothing loops over panels."""
    base = np.asarray(base).reshape(-1)
    vals = np.stack(sweep_values(mins, maxes, input_idxs, n_frames)).astype(base.dtype)
    rows, cols = grid_shape(input_idxs, n_frames, mode)
    p = np.arange(rows * cols)
    i0, i1 = p // cols, p % cols
    table = np.tile(base, (rows * cols, 1))
    idx = np.asarray(input_idxs)
    if mode == '1d':
        table[p, idx[i0]] = vals[i0, i1]
    else:
        table[p, idx[0]] = vals[0, i0]
        table[p, idx[1]] = vals[1, i1]
    return table.astype(np.float32), (rows, cols)


# ------------------------------------------------------------------------------------------ crops and mosaics
def get_crop_ref(im, y_0, y_ext, x_0, x_ext):
    """The reference's ``get_crop`` for a window that starts inside the image: float64, zero past the edges."""
    y_min, x_min = y_0 - y_ext, x_0 - x_ext
    assert y_min >= 0 and x_min >= 0
    out = np.zeros((2 * y_ext, 2 * x_ext))
    part = np.copy(im[y_min:y_0 + y_ext, x_min:x_0 + x_ext])
    out[:part.shape[0], :part.shape[1]] = part
    return out


def crop_window(im, y_min, x_min, hc, wc):
    """Any window (odd sizes too) of a 2-d array, by padding with zeros below and to the right and slicing."""
    padded = np.pad(im, ((0, y_min + hc), (0, x_min + wc)))
    return padded[y_min:y_min + hc, x_min:x_min + wc]


def _grey(frames):
    frames = np.asarray(frames)
    return frames if frames.dtype == np.uint8 else quantise_u8(frames)


def _window(frames, crop):
    return (0, 0, frames.shape[2], frames.shape[3]) if crop is None else tuple(int(v) for v in crop)


def mosaic_blocks(frames, src, ch=0, crop=None):
    """(T, R Hc, Cc Wc) uint8: every panel the crop of its quantised frame (zeros for a blank one), ``np.block``."""
    grey = _grey(frames)
    y_min, x_min, hc, wc = _window(grey, crop)
    src = np.asarray(src)
    blank = np.zeros((hc, wc), dtype=np.uint8)
    out = [np.block([[blank if s < 0 else crop_window(grey[s, ch], y_min, x_min, hc, wc) for s in row] for row in t])
           for t in src]
    return np.stack(out).astype(np.uint8) if len(out) else np.zeros((0, src.shape[1] * hc, src.shape[2] * wc), np.uint8)


def mosaic_index_rule(frames, src, ch=0, crop=None):
    """The rule of include/behavenet_hip.h, per output pixel: out[t, r Hc + y, c Wc + x] is zero for src < 0,
    y_min + y >= H or x_min + x >= W, else the quantised frames[src, ch, y_min + y, x_min + x]."""
    frames = np.asarray(frames)
    y_min, x_min, hc, wc = _window(frames, crop)
    src = np.asarray(src)
    t_n, r_n, c_n = src.shape
    h, w = frames.shape[2:]
    t, oy, ox = np.indices((t_n, r_n * hc, c_n * wc))
    s = src[t, oy // hc, ox // wc]
    ys, xs = y_min + oy % hc, x_min + ox % wc
    shown = (s >= 0) & (ys < h) & (xs < w)
    if frames.shape[0] == 0:
        return np.zeros(s.shape, dtype=np.uint8)
    picked = frames[np.where(shown, s, 0), ch, np.where(shown, ys, 0), np.where(shown, xs, 0)]
    return np.where(shown, _grey(picked), 0).astype(np.uint8)


def grid_src(rows, cols):
    return np.arange(rows * cols, dtype=np.int32).reshape(1, rows, cols)


def movie_src_ref(n_base, n_dims, n_frames, n_cols):
    """Time b n_frames + i, panel k at (k // n_cols, k % n_cols): point (b n_dims + k) n_frames + i; else -1."""
    n_rows = int(np.ceil(n_dims / n_cols))
    src = -np.ones((n_base * n_frames, n_rows, n_cols), dtype=np.int32)
    for b in range(n_base):
        for i in range(n_frames):
            for k in range(n_dims):
                src[b * n_frames + i, k // n_cols, k % n_cols] = (b * n_dims + k) * n_frames + i
    return src


# ------------------------------------------------------------------------------------------ markers
def scaled_labels(labels_og, idxs=None, vals=None):
    """The scaled labels (1, n) of one panel: 4-d one-hot maps read back as [all x, all y], then the updates."""
    if labels_og is None:
        return None
    if np.ndim(labels_og) == 4:
        _, y, x = np.nonzero(np.asarray(labels_og)[0] == 1)
        out = np.concatenate([x, y])[None, :]
    else:
        out = np.array(labels_og, copy=True)
    if idxs is not None:
        for idx, val in zip(np.atleast_1d(idxs), np.atleast_1d(vals)):
            out[0, idx] = val
    return out


def marker_lists(interp_type, mode, labels_sc_0, input_idxs, n_frames, mins_sc=None, maxes_sc=None, marker_idxs=None,
                 origin=(0, 0)):
    """[[ [y, x] per panel ] per row]: a label traversal reads the updated labels at input_idxs[0] / [1], a latent
    traversal the unchanged ones at marker_idxs, both shifted by the crop's origin; [nan, nan] without labels."""
    rows, cols = grid_shape(input_idxs, n_frames, mode)
    vals_sc = None if mins_sc is None else sweep_values(mins_sc, maxes_sc, input_idxs, n_frames)
    out = []
    for i0 in range(rows):
        row = []
        for i1 in range(cols):
            if interp_type == 'labels':
                if mode == '1d':
                    lab = scaled_labels(labels_sc_0, [input_idxs[i0]], [vals_sc[i0][i1]])
                else:
                    lab = scaled_labels(labels_sc_0, input_idxs, [vals_sc[0][i0], vals_sc[1][i1]])
                row.append([lab[0, input_idxs[0]] - origin[0], lab[0, input_idxs[1]] - origin[1]])
            elif labels_sc_0 is not None:
                lab = scaled_labels(labels_sc_0)
                row.append([lab[0, marker_idxs[0]] - origin[0], lab[0, marker_idxs[1]] - origin[1]])
            else:
                row.append([np.nan, np.nan])
        out.append(row)
    return out


def one_hot_maps(xs, ys, h, w):
    """(1, L, h, w) float maps with one 1 per label at (ys[l], xs[l]): the 4-d ``labels_sc_0`` of the reference."""
    maps = np.zeros((1, len(xs), h, w))
    for l, (x, y) in enumerate(zip(xs, ys)):
        maps[0, l, y, x] = 1
    return maps


# ------------------------------------------------------------------------------------------ the per-point loop
def frames_loop(get_reconstruction, interp_type, mode, model, ims_0, latents_0, labels_0, mins, maxes, input_idxs,
                n_frames, device):
    """The reference's way: ONE ``get_reconstruction`` call per panel -> [[(C, H, W) float32 per panel] per row]."""
    cls = model.hparams['model_class']
    vals = sweep_values(mins, maxes, input_idxs, n_frames)
    rows, cols = grid_shape(input_idxs, n_frames, mode)

    def changed(base, i0, i1):
        point = np.copy(base)
        if mode == '1d':
            point[0, input_idxs[i0]] = vals[i0][i1]
        else:
            point[0, input_idxs[0]], point[0, input_idxs[1]] = vals[0][i0], vals[1][i1]
        return point
    out = []
    for i0 in range(rows):
        row = []
        for i1 in range(cols):
            if interp_type == 'latents' or cls in ('cond-ae-msp', 'ps-vae', 'msps-vae'):
                labels = None
                if cls in ('cond-ae', 'cond-vae'):
                    labels = torch.from_numpy(labels_0).float().to(device)
                im = get_reconstruction(model, torch.from_numpy(changed(latents_0, i0, i1)).float().to(device),
                                        labels=labels, apply_inverse_transform=True)
            else:
                im = get_reconstruction(model, ims_0.to(device),
                                        labels=torch.from_numpy(changed(labels_0, i0, i1)).float().to(device),
                                        labels_2d=None)
            row.append(np.copy(im[0]))
        out.append(row)
    return out
