"""Host-side helpers of the plotting code with the reference's names (``behavenet/plotting/__init__.py``), so that a
script written against the reference changes its import and nothing else.  Nothing here imports matplotlib."""

import numpy as np

__all__ = ['get_crop']


def get_crop(im, y_0, y_ext, x_0, x_ext):
    """The window ``[y_0 - y_ext, y_0 + y_ext) x [x_0 - x_ext, x_0 + x_ext)`` of the 2-d array ``im`` as a float64
    array ``(2 y_ext, 2 x_ext)``, zero where the window passes the bottom or the right edge (ref
    plotting/__init__.py:41-73).  A window that starts above or left of the image is a ValueError: the reference's
    slice wraps around there and returns no defined crop."""
    y_min, x_min = y_0 - y_ext, x_0 - x_ext
    if y_min < 0 or x_min < 0:
        raise ValueError('get_crop: the window starts at (%d, %d), outside the image' % (y_min, x_min))
    crop = np.zeros((2 * y_ext, 2 * x_ext))
    inside = np.asarray(im)[y_min:y_0 + y_ext, x_min:x_0 + x_ext]
    crop[:inside.shape[0], :inside.shape[1]] = inside
    return crop
