"""Pillow's `Image.resize(wh, Image.BILINEAR)` for 8-bit RGB restated in numpy (ImagingResample with box=None, reducing_gap=None: the coefficient
table of an axis in double, its 22-bit quantisation, the horizontal pass rounded and clipped to bytes, the vertical pass on those bytes), and the
cases the resize tests share.  tests/test_resize_host.py holds the restatement against Pillow itself, byte for byte; the kernel and the library's
host function are held against the restatement."""
import math

import numpy as np

PRECISION_BITS = 22


def tri(a):
    a = abs(a)
    return 1.0 - a if a < 1.0 else 0.0


def ksize(in_size, out_size):
    support = 1.0 * max(in_size / out_size, 1.0)
    return int(math.ceil(support)) * 2 + 1


def coeffs(in_size, out_size):
    """(start [out], count [out], k [out, ksize]) int32: precompute_coeffs and normalize_coeffs_8bpc for the triangle filter.  Python floats are C
    doubles and int() truncates as a C cast does."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ks = int(math.ceil(support)) * 2 + 1
    start, count, k = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32), np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [tri((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5)
        start[xx], count[xx] = xmin, n
    return start, count, k


def one_pass(a, axis, out_size):
    """One pass of [..] uint8 `a` along `axis`: clip8((2^21 + sum in * k) >> 22) with an accumulator that is checked to stay inside 32 bits."""
    a = np.moveaxis(a, axis, 0)
    start, count, k = coeffs(a.shape[0], out_size)
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for xx in range(out_size):
        s, n = int(start[xx]), int(count[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[xx, :n].astype(np.int64), a[s:s + n].astype(np.int64), axes=(0, 0))
        assert acc.max() < 2 ** 31 and acc.min() >= 0
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(frames, out_wh):
    """uint8 [N,Hin,Win,3] -> [N,H,W,3], out_wh = (W, H): horizontal first, to bytes; then vertical.  A pass along an axis of unchanged size is
    skipped."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    W, H = out_wh
    out = frames
    if out.shape[2] != W:
        out = one_pass(out, 2, W)
    if out.shape[1] != H:
        out = one_pass(out, 1, H)
    return np.ascontiguousarray(out).copy()


# (Hin, Win, (W, H)): the smallest shapes at which the kernel (8 x 32 output tiles) can still go wrong
SHAPES = [
    (37, 53, (16, 12)),      # inexact ratios
    (64, 80, (20, 16)),      # the workload's exact ratio of 4
    (12, 16, (16, 12)),      # up on one axis, down on the other
    (8, 12, (20, 31)),       # up-scale, two taps
    (5, 7, (5, 3)),          # horizontal pass skipped
    (5, 7, (9, 7)),          # vertical pass skipped
    (6, 9, (9, 6)),          # copy
    (9, 9, (1, 1)),
    (2, 3, (7, 5)),
    (40, 150, (70, 9)),      # output extents that straddle tile edges and are no multiple of 4
    (150, 40, (9, 70)),
]
REFUSED = (7, 1000, (3, 2))  # 1000 -> 3 is beyond the documented ratio bound of 16
CASES = [(hin, win, wh, n) for hin, win, wh in SHAPES for n in (1, 3)]
CASE_IDS = ["%dx%d-to-%dx%d-N%d" % (hin, win, wh[1], wh[0], n) for hin, win, wh, n in CASES]
KINDS = ("random", "extremes", "all255", "impulse_corner", "impulse_centre", "impulse_tile_edge")
TILE_H, TILE_W = 8, 32


def data(kind, n, hin, win, seed=0):
    """uint8 [n,hin,win,3]."""
    rs = np.random.RandomState(seed + 1000 * KINDS.index(kind))
    if kind == "random":
        return rs.randint(0, 256, (n, hin, win, 3)).astype(np.uint8)
    if kind == "extremes":                                   # the worst rounding
        return (rs.randint(0, 2, (n, hin, win, 3)) * 255).astype(np.uint8)
    if kind == "all255":                                     # the clip and the accumulator's headroom
        return np.full((n, hin, win, 3), 255, np.uint8)
    if kind == "impulse_corner":
        return impulse(n, hin, win, 0, 0)
    if kind == "impulse_centre":
        return impulse(n, hin, win, hin // 2, win // 2)
    raise ValueError(kind)


def impulse(n, hin, win, y, x):
    """A single 255 on zeros per frame, for footprint read-out: frame f has it at row y + f (clipped), column x, channel f % 3."""
    a = np.zeros((n, hin, win, 3), np.uint8)
    for f in range(n):
        a[f, min(hin - 1, y + f), x, f % 3] = 255
    return a


def tile_edge_pixel(hin, win, wh):
    """Input pixel whose footprint straddles the corner between the first output tile and its neighbours (clipped into the image)."""
    W, H = wh
    return min(hin - 1, TILE_H * hin // H), min(win - 1, TILE_W * win // W)


def case_data(kind, n, hin, win, wh):
    if kind == "impulse_tile_edge":
        return impulse(n, hin, win, *tile_edge_pixel(hin, win, wh))
    return data(kind, n, hin, win)


_refs = {}


def reference(kind, n, hin, win, wh):
    """(input, restated output) of a case, computed once."""
    key = (kind, n, hin, win, wh)
    if key not in _refs:
        a = case_data(kind, n, hin, win, wh)
        out = resize(a, wh)
        a.setflags(write=False)
        out.setflags(write=False)
        _refs[key] = (a, out)
    return _refs[key]
