"""Numpy restatements of the state-run search and the syllable movie, written for this project's tests: plain loops,
no attempt at speed, and none of the code under test.

  runs_of            the rows (trial, beg, end, state) by a loop over trials and frames
  frames_of / trans_of   the histograms by np.add.at
  chunks_of / durations_of   the reference's get_discrete_chunks / get_state_durations structures from per-trial paths
  plan_of            the panels of the syllable movie, frame by frame (a second loop, independent of
                     fitting.eval.syllable_movie_plan)
  stamped / movie_of the stamped movie by slicing
"""

import numpy as np


def runs_of(states, offsets):
    """int32 (R, 4): one row (trial, beg, end, state) per maximal stretch of equal states inside one trial."""
    states = np.asarray(states)
    rows = []
    for s in range(len(offsets) - 1):
        path = states[offsets[s]:offsets[s + 1]]
        beg = 0
        for i in range(1, len(path) + 1):
            if i == len(path) or path[i] != path[beg]:
                rows.append((s, beg, i, int(path[beg])))
                beg = i
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def frames_of(states, offsets, K):
    out = np.zeros((K,), dtype=np.int64)
    for s in range(len(offsets) - 1):
        np.add.at(out, np.asarray(states[offsets[s]:offsets[s + 1]], dtype=np.int64), 1)
    return out


def trans_of(states, offsets, K):
    out = np.zeros((K, K), dtype=np.int64)
    for s in range(len(offsets) - 1):
        path = np.asarray(states[offsets[s]:offsets[s + 1]], dtype=np.int64)
        np.add.at(out, (path[:-1], path[1:]), 1)
    return out


def chunks_of(paths, K, include_edges=True):
    """Per state the [chunk, beg, end] of its stretches in the trials ``paths``, in order of appearance."""
    out = [[] for _ in range(K)]
    for c, path in enumerate(paths):
        beg = 0
        for i in range(1, len(path) + 1):
            if i == len(path) or path[i] != path[beg]:
                if include_edges or (beg > 0 and i < len(path)):
                    out[int(path[beg])].append([c, beg, i])
                beg = i
    return [np.asarray(o, dtype=np.int64).reshape(-1, 3) for o in out]


def durations_of(paths, K, include_edges=True):
    if K == 1:
        return []
    return [c[:, 2] - c[:, 1] for c in chunks_of(paths, K, include_edges)]


def plan_of(state_list, max_frames, n_buffer, n_pre_frames, n_rows=None, single_syllable=None):
    """(src, mark, n_rows, n_cols) of the syllable movie: every panel is played frame by frame, as a viewer would
    see it, into lists of (chunk, row, marked)."""
    states = [single_syllable] if single_syllable is not None else list(range(len(state_list)))
    if single_syllable is not None:
        n_rows = 1
    if n_rows is None:
        n_rows = int(np.sqrt(len(states)))
    n_cols = -(-len(states) // n_rows)
    films = []
    for k in states:
        film = []
        todo = [tuple(int(v) for v in inst) for inst in state_list[k]]
        while todo and len(film) < max_frames:
            chunk, beg, end = todo.pop(0)
            lead = min(n_pre_frames, beg)
            for i, row in enumerate(range(beg - lead, end)):
                film.append((chunk, row, int(i in (lead, lead + 1))))
            film += [(-1, -1, 0)] * n_buffer
        if len(state_list[k]):
            film += [(-1, -1, 0)] * max(max_frames - len(film), 0)            # out of instances: blanks to max_frames
        films.append(film)
    n_t = max(len(f) for f in films)
    src = np.full((n_t, n_rows, n_cols, 2), -1, dtype=np.int64)
    mark = np.zeros((n_t, n_rows, n_cols), dtype=np.uint8)
    for p, film in enumerate(films):
        for t, (chunk, row, m) in enumerate(film):
            src[t, p // n_cols, p % n_cols] = (chunk, row)
            mark[t, p // n_cols, p % n_cols] = m
    return src, mark, n_rows, n_cols


def quantise(x):
    """fp32 unit floats -> grey levels, unit_float_to_u8's rule."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x), 0, np.clip(np.rint(x * np.float32(255)), 0, 255)).astype(np.uint8)


def stamped(movie, mark, panel_hw, box=(5, 5, 10, 10), value=255):
    """A copy of ``movie`` (T, R * Hp, Cc * Wp) with the box set in every marked panel, by slicing."""
    out = np.array(movie, copy=True)
    hp, wp = panel_hw
    y0, x0, h, w = box
    ya, yb = min(max(y0, 0), hp), min(max(y0 + h, 0), hp)
    xa, xb = min(max(x0, 0), wp), min(max(x0 + w, 0), wp)
    for t, r, c in zip(*np.nonzero(mark)):
        out[t, r * hp + ya:r * hp + yb, c * wp + xa:c * wp + xb] = value
    return out


def movie_of(trial_frames, src, mark):
    """The stamped syllable movie of a plan: panel (r, c) of frame t is the channels of frame src[t, r, c] stacked
    vertically, black where src is -1; then the boxes."""
    first = next(np.asarray(f) for f in trial_frames if f is not None and len(f))
    _, C, H, W = first.shape
    n_t, n_rows, n_cols, _ = src.shape
    movie = np.zeros((n_t, n_rows * C * H, n_cols * W), dtype=np.uint8)
    for t in range(n_t):
        for r in range(n_rows):
            for c in range(n_cols):
                chunk, row = src[t, r, c]
                if chunk < 0:
                    continue
                frame = np.asarray(trial_frames[chunk][row])
                frame = frame if frame.dtype == np.uint8 else quantise(frame)
                movie[t, r * C * H:(r + 1) * C * H, c * W:(c + 1) * W] = frame.reshape(C * H, W)
    return stamped(movie, mark, (C * H, W))
