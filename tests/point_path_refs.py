"""The yardstick of the point-path and session-swap tests: what the reference's ``interpolate_point_path``,
``make_latent_traversal_movie`` and ``make_session_swap_movie`` do, restated in plain numpy loops (no tests here),
and the rule of ``bn_frame_mosaic_ch_u8`` as include/behavenet_hip.h states it, one sub-panel at a time.

Quantisation is ``tests.recon_u8_refs.quantise_u8``."""

import numpy as np

from tests.recon_u8_refs import quantise_u8


# ------------------------------------------------------------------------------------------ paths
def path_loop(points, n_frames):
    """Step by step: a leg of n frames has n + 1 steps start + k * ((stop - start) / n), k a Python int, each a
    (1, D) row in the dtype numpy gives; a list of per-leg counts of another length is an AssertionError."""
    n_legs = len(points) - 1
    counts = [n_frames] * n_legs if isinstance(n_frames, int) else list(n_frames)
    assert len(counts) == n_legs
    steps = []
    for leg, n in enumerate(counts):
        start, stop = points[leg:leg + 1], points[leg + 1:leg + 2]
        step = (stop - start) / n
        for k in range(n + 1):
            steps.append(start + k * step)
    return steps


def three_point_path(base_row, dim, lo, hi):
    """min -> max -> min: the base row three times with one column overwritten."""
    points = np.array([base_row] * 3)
    points[0, dim] = lo
    points[1, dim] = hi
    points[2, dim] = lo
    return points


def movie_table(base, panels, n_frames):
    """(B K 2 (n_frames + 1), D) float32: base by base, panel by panel, step by step."""
    rows = []
    for b in range(len(base)):
        for dim, lo, hi in panels:
            rows += [s[0] for s in path_loop(three_point_path(base[b], dim, lo, hi), n_frames)]
    return np.stack(rows).astype(np.float32)


def path_movie_src_loop(n_base, n_panels, n_steps, n_buffer_frames, n_cols, order_idxs=None):
    """Frame by frame: the panels in ``order_idxs`` order fill the grid row by row, then the buffer frames of the
    base point (only where there are several), all blank."""
    order = list(range(n_panels)) if order_idxs is None else list(order_idxs)
    n_rows = int(np.ceil(len(order) / n_cols))
    frames = []
    for b in range(n_base):
        for i in range(n_steps):
            grid = -np.ones((n_rows, n_cols), dtype=np.int32)
            for j, k in enumerate(order):
                grid[j // n_cols, j % n_cols] = (b * n_panels + k) * n_steps + i
            frames.append(grid)
        if n_base > 1:
            for _ in range(n_buffer_frames):
                frames.append(-np.ones((n_rows, n_cols), dtype=np.int32))
    return np.stack(frames)


# ------------------------------------------------------------------------------------------ session swaps
def swap_loop(latents, background_idxs, medians):
    """Session by session: a copy of the trial's latents with the background columns overwritten."""
    blocks = []
    for s in range(len(medians)):
        z = np.copy(latents)
        z[:, background_idxs] = medians[s]
        blocks.append(z)
    return np.concatenate(blocks, axis=0)


def swap_grid_loop(n_sessions, sess_idx, layout_pattern=None):
    """The grid of panels: the sessions in order with ``sess_idx`` and 0 exchanged, dealt row by row onto the true
    positions of the pattern (without one: 1 x S below four sessions, 2 x 2 for four, 2 x 3 for five and six, filled
    from the top left).  -1: empty."""
    queue = list(range(n_sessions))
    queue[0], queue[sess_idx] = queue[sess_idx], queue[0]
    if layout_pattern is None:
        n_rows, n_cols = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (2, 3), 6: (2, 3)}[n_sessions]
        layout_pattern = [[r * n_cols + c < n_sessions for c in range(n_cols)] for r in range(n_rows)]
    grid = []
    for row in layout_pattern:
        grid.append([queue.pop(0) if here else -1 for here in row])
    assert not queue
    return np.array(grid)


# ------------------------------------------------------------------------------------------ the mosaic
def mosaic_channels_rule(frames, src, ch0, n_ch, crop=None):
    """out[i, j hc + y, (k n_ch + q) wc + x] = 0 where s = src[i, j, k] is negative or >= p, y_min + y >= h or
    x_min + x >= w; else the grey level of frames[s, ch0 + q, y_min + y, x_min + x]."""
    frames = np.asarray(frames)
    p, _, h, w = frames.shape
    y_min, x_min, hc, wc = (0, 0, h, w) if crop is None else tuple(int(v) for v in crop)
    src = np.asarray(src)
    t_n, r_n, c_n = src.shape
    out = np.zeros((t_n, r_n * hc, c_n * n_ch * wc), dtype=np.uint8)
    for i in range(t_n):
        for j in range(r_n):
            for k in range(c_n):
                s = int(src[i, j, k])
                if s < 0 or s >= p:
                    continue
                for q in range(n_ch):
                    plane = frames[s, ch0 + q]
                    grey = plane if plane.dtype == np.uint8 else quantise_u8(plane)
                    part = grey[y_min:y_min + hc, x_min:x_min + wc]
                    oy, ox = j * hc, (k * n_ch + q) * wc
                    out[i, oy:oy + part.shape[0], ox:ox + part.shape[1]] = part
    return out
