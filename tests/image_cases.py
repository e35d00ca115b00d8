"""Case builders and a float32 numpy restatement for the whole-image kernels (csrc/image.hip: ucnerf_image_put, ucnerf_depth_minmax,
ucnerf_depth_colormap) and the visualize_depth mirror (uc_nerf_amd/utils/utils.py).  Shared by tests/test_image_cases_host.py (CPU) and
tests/test_hip_image.py (GPU); everything here is deterministic and cached, nothing touches a device.

The restatement says, in elementary numpy steps, what the reference's visualize_depth (utils/utils.py:58-77) computes in float32:

    x   = nan_to_num(depth)                      NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX
    t   = (x - mi) / d                           one IEEE division
          from the data:      mi = min(x), ma = max(x), d = fl32(fl32(ma - mi) + fl32(1e-8))
          from a caller's (mi, ma) Python floats: mi -> fl32(mi), d = fl32(double(ma) - double(mi) + 1e-8)
    v   = fl32(255 * t)                          a second rounding
    idx = uint8(v) truncated toward zero; DEFINED where numpy is not: NaN -> 0, v < 0 -> 0, v > 255 -> 255
    out[c] = fl32(table[idx][c] / 255)           channel c = column c of the table

It is written apart from the package's own numpy path on purpose (explicit loops over the special values, np.trunc instead of a clip and a
cast), so that the host test's bit-for-bit comparison of the two says something."""
import functools

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
GROUP_PIXELS = 1024          # pixels one workgroup covers and folds into one atomicMin / atomicMax (csrc/image.hip: IM_GROUP = 256 threads x 4)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def same_bits(a, b):
    """Bit for bit, -0.0 apart from +0.0; any NaN matches any NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | ((a != a) & (b != b))).all())


def same_values(a, b):
    """Equal as float32 values (+0 == -0), NaN matching NaN -- every other value has one bit pattern, so this is bit for bit but for the sign of zero."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


# ------------------------------------------------------------------------------------------------ restatement
def nan_to_num32(depth):
    x = np.array(depth, dtype=F32, copy=True)
    x[x != x] = F32(0.0)
    x[x == np.inf] = FLT_MAX
    x[x == -np.inf] = -FLT_MAX
    return x


def minmax_reference(depth):
    """(min, max) of nan_to_num(depth) as float32 scalars."""
    x = nan_to_num32(depth)
    return x.min(), x.max()


def index_reference(depth, minmax=None):
    x = nan_to_num32(depth)
    with np.errstate(all="ignore"):
        if minmax is None:
            mi, ma = minmax_reference(depth)
            d = F32(F32(ma - mi) + F32(1e-8))
        else:
            mi, d = F32(float(minmax[0])), F32(float(minmax[1]) - float(minmax[0]) + 1e-8)
        t = np.divide(np.subtract(x, mi, dtype=F32), d, dtype=F32)
        v = np.multiply(F32(255.0), t, dtype=F32)
    idx = np.zeros(v.shape, np.uint8)
    ok = (v == v) & (v >= 0)                                   # NaN and negatives stay 0
    idx[ok & (v > 255)] = 255
    mid = ok & (v <= 255)
    idx[mid] = np.trunc(v[mid]).astype(np.int64).astype(np.uint8)
    return idx


def color_reference(idx, table):
    """[3, *idx.shape] float32: table[idx][c] / 255, one IEEE division."""
    out = np.empty((3,) + idx.shape, F32)
    for c in range(3):
        out[c] = np.divide(table[:, c][idx].astype(F32), F32(255.0), dtype=F32)
    return out


# ------------------------------------------------------------------------------------------------ depth maps
def random_table(seed=5):
    """A table no two columns of which agree and which is not symmetric: a swapped channel or a transposed table cannot pass."""
    t = np.random.default_rng(seed).integers(0, 256, (256, 3)).astype(np.uint8)
    assert len({t[:, c].tobytes() for c in range(3)}) == 3
    return t


DEPTH_NAMES = ("constant", "two_valued", "lattice", "random", "given_range", "nonfinite", "nonfinite_given", "negative_and_tiny")


@functools.lru_cache(maxsize=None)
def depth_case(name):
    """-> dict(name, depth [H,W] float32, minmax None or a pair of Python floats)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    minmax = None
    if name == "constant":
        depth = np.full((5, 7), 3.5, F32)                      # ma == mi: every index 0 (0 / 1e-8)
    elif name == "two_valued":
        depth = np.where(rng.random((9, 13)) < 0.5, F32(1.25), F32(2.75)).astype(F32)
    elif name == "lattice":
        depth = np.arange(256, dtype=F32).reshape(8, 32)      # mi = 0, ma = 255, d = fl32(255 + 1e-8) = 255: v = 255 fl(j / 255) = j exactly; a low quotient gives j - 1
    elif name == "random":
        depth = (0.5 + 6.5 * rng.random((67, 63))).astype(F32)      # 4221 pixels: four workgroups and a ragged tail
    elif name == "given_range":
        depth = (0.5 + 6.5 * rng.random((41, 37))).astype(F32)
        minmax = (2.0, 5.0)                                    # inside the data's range: both ends saturate
    elif name in ("nonfinite", "nonfinite_given"):
        depth = (1.0 + 3.0 * rng.random((11, 17))).astype(F32)
        flat = depth.reshape(-1)
        flat[[3, 50, 120]] = np.nan
        flat[[7, 99]] = np.inf
        flat[[8, 140]] = -np.inf
        minmax = (0.0, 10.0) if name == "nonfinite_given" else None
    elif name == "negative_and_tiny":
        depth = (rng.standard_normal((10, 11)) * 2).astype(F32)
        flat = depth.reshape(-1)
        flat[[0, 5, 9]] = [-0.0, 0.0, 1e-40]                   # a denormal
        flat[[20, 21]] = [-1e-40, np.nan]
    else:
        raise KeyError(name)
    depth.setflags(write=False)
    return dict(name=name, depth=depth, minmax=minmax)


# ------------------------------------------------------------------------------------------------ min / max data
MINMAX_COUNTS = (1, 63, 64, 65, GROUP_PIXELS - 1, GROUP_PIXELS, GROUP_PIXELS + 1, 2 * GROUP_PIXELS + 37)
MINMAX_KINDS = ("tame", "wild", "negative", "all_nan")


@functools.lru_cache(maxsize=None)
def minmax_data(count, kind):
    """tame: NaN, +-0, denormals and negatives among ordinary values, the largest value LAST (the ragged tail), the smallest in the middle;
    wild: the same with +-inf (the range becomes +-FLT_MAX); negative: every value below zero (the keys of negatives order the other way
    round); all_nan: nothing but NaN (range 0 .. 0)."""
    rng = np.random.default_rng(1000 * count + len(kind))
    x = (rng.standard_normal(count) * 3).astype(F32)
    if kind == "all_nan":
        x[:] = np.nan
    elif kind == "negative":
        x = -np.abs(x) - F32(1e-3)
        if count > 8:
            x[count // 3] = -1e-40
    else:
        special = [np.nan, -0.0, 0.0, 1e-40, -1e-40] + ([np.inf, -np.inf] if kind == "wild" else [])
        if count >= 63:
            x[(np.arange(len(special)) * 9 + 1)] = special
        if kind == "tame":
            x[count - 1] = 77.5
            x[count // 2] = -66.25 if count > 1 else 77.5
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ assembly
@functools.lru_cache(maxsize=None)
def put_case(H=5, W=7, seed=2):
    """rgb [H W, 3] and depth [H W] with what a clamp can get wrong: NaN, -0.0, the neighbours of 0 and 1, denormals, far outside values."""
    rng = np.random.default_rng(seed)
    n = H * W
    rgb = (rng.random((n, 3)) * 1.4 - 0.2).astype(F32)
    one, zero = F32(1.0), F32(0.0)
    special = [np.nan, -0.0, 0.0, np.nextafter(one, F32(2)), np.nextafter(one, zero), np.nextafter(zero, one), np.nextafter(zero, -one), 1e-40, -1e-40,
               1e30, -1e30, np.inf, -np.inf, 1.0]
    flat = rgb.reshape(-1)
    flat[(np.arange(len(special)) * 7 + 2) % flat.size] = special
    depth = (1.0 + 3.0 * rng.random(n)).astype(F32)
    depth[[1, n - 1]] = [np.nan, -0.0]
    depth[n // 2] = 1e-40
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


def assemble_reference(rgb, depth, H, W):
    """The reference's host ops (train.py:277-279): torch.clamp(torch.cat(rgbs).reshape(H, W, 3).permute(2, 0, 1), 0, 1), cat(depths).reshape(H, W)."""
    import torch
    img = torch.clamp(torch.from_numpy(np.array(rgb)).reshape(H, W, 3).permute(2, 0, 1), 0, 1).contiguous().numpy()
    return img, np.array(depth).reshape(H, W)
