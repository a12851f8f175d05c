"""
peakdetect.peakdetect (the reference's peakdetect.py, after billauer's peakdet) on the device: dd_peakdetect_f64.

Same positions, values and pop rule as the reference for finite input, any lookahead >= 1 and delta >= 0.  Non-finite input
raises ValueError (DD_ERR_INVALID), where the reference's comparisons would silently skip NaN.
"""
import numpy as np

from . import afsk


def peakdetect(y_axis, x_axis=None, lookahead=200, delta=0):
    """-> [max_peaks, min_peaks], each a list of [x, y] pairs; x from x_axis (index when None)"""
    if x_axis is None:
        x_axis = range(len(y_axis))
    if len(y_axis) != len(x_axis):
        raise ValueError("Input vectors y_axis and x_axis must have same length")
    y = np.asarray(y_axis, dtype=np.float64)
    x = np.asarray(x_axis)
    if lookahead < 1:
        raise ValueError("Lookahead must be '1' or above in value")
    if not (np.isscalar(delta) and delta >= 0):
        raise ValueError("delta must be a positive number")
    (mp, mv), (np_, nv) = afsk.peak_lists(y, int(lookahead), float(delta))
    mp, mv, np_, nv = mp.to_host(), mv.to_host(), np_.to_host(), nv.to_host()
    return [[[x[i], v] for i, v in zip(mp, mv)], [[x[i], v] for i, v in zip(np_, nv)]]
