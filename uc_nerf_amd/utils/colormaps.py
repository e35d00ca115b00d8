"""Colour tables for the depth pictures (`utils.utils.visualize_depth`).  A table is a 256 x 3 uint8 numpy array; every function of this package
that takes `cmap=` accepts any such table."""
import numpy as np

_JET = None


def _matlab_jet(m):
    """MATLAB's jet(m) as published: a trapezoid u = [1/n .. 1, ones(n - 1), 1 .. 1/n] with n = ceil(m / 4), placed at offsets ceil(n / 2) (green),
    + n (red) and - n (blue) and cut at the ends.  -> [m,3] float64 in (r, g, b) column order."""
    n = int(np.ceil(m / 4))
    u = np.concatenate([np.arange(1, n + 1) / n, np.ones(n - 1), np.arange(n, 0, -1) / n])
    g = int(np.ceil(n / 2)) - int(m % 4 == 1) + np.arange(1, len(u) + 1)              # 1-based rows, as MATLAB writes it
    r, b = g + n, g - n
    keep_r, keep_g, keep_b = r <= m, g <= m, b >= 1
    J = np.zeros((m, 3))
    J[r[keep_r] - 1, 0] = u[:keep_r.sum()]
    J[g[keep_g] - 1, 1] = u[:keep_g.sum()]
    J[b[keep_b] - 1, 2] = u[len(u) - keep_b.sum():]
    return J


def jet_lut():
    """A Jet table in OpenCV's column order (column 0 blue, 1 green, 2 red), 256 x 3 uint8, built from the published definition of OpenCV's Jet:
    the 64 control points of the MATLAB jet, linearly interpolated over [0, 1] to 256 entries, times 255, rounded half to even.

    cv2 is not installed where this package is developed, so THIS TABLE CANNOT BE VERIFIED AGAINST OPENCV HERE and has not been: entries may
    differ from cv2's by a unit where the interpolation lands next to a rounding boundary, and an OpenCV release that ships another
    parametrisation of Jet would differ by more.  Someone who has cv2 produces the authoritative table with

        cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET).reshape(256, 3)

    and passes it as `cmap=`.  The returned array is a copy."""
    global _JET
    if _JET is None:
        ctrl = _matlab_jet(64)                                       # (r, g, b)
        x, xi = np.linspace(0.0, 1.0, 64), np.linspace(0.0, 1.0, 256)
        rgb = np.stack([np.interp(xi, x, ctrl[:, c]) for c in range(3)], axis=1)
        _JET = np.rint(rgb[:, ::-1] * 255.0).astype(np.uint8)        # (b, g, r); np.rint rounds half to even
    return _JET.copy()


def as_table(cmap):
    """cmap=None -> jet_lut(); anything else must be a 256 x 3 uint8 table (numpy array or CPU / device tensor) and is returned as numpy."""
    if cmap is None:
        return jet_lut()
    t = cmap.detach().cpu().numpy() if hasattr(cmap, "detach") else np.asarray(cmap)
    if t.dtype != np.uint8 or t.shape != (256, 3):
        raise ValueError("a colour table is 256 x 3 uint8 (see utils.colormaps.jet_lut), got %s %s" % (t.dtype, t.shape))
    return np.ascontiguousarray(t)
