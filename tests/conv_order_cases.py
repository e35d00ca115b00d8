"""Cases and restatement for the summation order of the two convolution kernels (csrc/lpips.hip: ucnerf_conv2d_bias_relu, csrc/conv3d.hip:
ucnerf_conv3d), numpy and torch-CPU only.

THE ORDER (include/ucnerf_hip.h).  The convolution is y[co][q] = sum_k w[co][k] x[k][q], k = ci * taps + t over the weight's flat row (the
transposed form: a parity class's live taps, ascending).  Within the j-th run of 32 consecutive k, S_j is an fmaf chain over ascending k from
+0; T = ((+0 + S_0) + S_1) + ... over ascending j; then + bias, the activation, + skip.  A tap in the padding is an operand of +0.

THE LATTICE, and why float64 numpy restates it exactly.  x = integers in [-2047, 2047] times 2^-8 (about one in eight exactly 0), w = integers in
[-2047, 2047] times 2^-10, bias and skip on the 2^-8 grid.  Every product is an exact multiple of 2^-18 below 2^4; every float32 partial sum is
a multiple of 2^-18 too (rounding to 24 bits cannot leave the grid) and stays below 2^15 as long as sum_k |w| |x| does (`check_lattice`
asserts both per case).  So float64(a) * float64(b) + float64(c) is exact (at most 33 bits) and ONE rounding of it to float32 is the true fmaf:
no math.fma, no double rounding.  Sums pass 2^6, where the float32 spacing exceeds 2^-18: float32 rounds, and the order shows.

THE ALTERNATIVES (`ALTERNATIVES`), each one change to the order: (a) one unblocked chain, (b) runs of 16, (c) runs of 64, (d) the runs folded in
descending j, (e) the k inside one instruction's group taken highest first (groups of 4 for conv3d's 16x16x4 MFMA, of 2 for conv2d's 32x32x2),
(f) the group's products summed exactly and rounded once into the accumulator, (g) the group summed pairwise in float32, then added.  On this
lattice a group's own sum (at most four products below 2^4 on the 2^-18 grid: 24 bits) never rounds, so (f) and (g) give the same bits; both
are kept because they are different mistakes."""
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = np.float32, np.float64
RUN = 32
GROUP = {"conv2d": 2, "conv3d": 4, "conv3dT": 4}                         # k per MFMA instruction
DOC = "doc"
ALTERNATIVES = ("a_chain", "b_run16", "c_run64", "d_fold_desc", "e_high_first", "f_group_exact", "g_group_pairwise")
VARIANTS = ("conv2d", "conv3d_16", "conv3d_32", "conv3d_single", "conv3dT_16", "conv3dT_32")
SUM_BOUND = 2.0 ** 15

# name: (kind, variant, n, cin, cout, K, stride, pad, size)
CASES = {
    "c3_16_k216": ("conv3d", "conv3d_16", 2, 8, 8, 3, 1, 1, (3, 4, 5)),          # 7 runs, the last 24; a 16-voxel tile spans the two images
    "c3_16_k81": ("conv3d", "conv3d_16", 1, 3, 5, 3, 1, 1, (3, 3, 4)),           # last run 17
    "c3_16_k40": ("conv3d", "conv3d_16", 1, 40, 8, 1, 1, 0, (2, 3, 4)),
    "c3_16_k1728": ("conv3d", "conv3d_16", 2, 1728, 8, 1, 1, 0, (4, 5, 6)),      # cin raised for (e)-(g): 54 runs without a padded tap
    "c3_32_k432": ("conv3d", "conv3d_32", 1, 16, 20, 3, 2, 1, (4, 5, 6)),
    "c3_32_two_tiles": ("conv3d", "conv3d_32", 1, 8, 33, 3, 1, 1, (2, 3, 3)),
    "c3_32_k1728": ("conv3d", "conv3d_32", 1, 1728, 20, 1, 1, 0, (3, 4, 5)),     # cin raised for (e)-(g)
    "c3_single": ("conv3d", "conv3d_single", 2, 8, 1, 3, 1, 1, (3, 4, 5)),       # x and row 0 of c3_16_k216
    "c3_single_k1728": ("conv3d", "conv3d_single", 2, 1728, 1, 1, 1, 0, (4, 5, 6)),      # x and row 0 of c3_16_k1728
    "c3T_16": ("conv3dT", "conv3dT_16", 2, 16, 8, 3, 2, 1, (2, 3, 3)),           # class k = 16 / 32 / 64 / 128
    "c3T_32": ("conv3dT", "conv3dT_32", 1, 12, 17, 3, 2, 1, (2, 2, 3)),          # class k = 12 / 24 / 48 / 96: one class is a single short run
    "c3T_16_cin864": ("conv3dT", "conv3dT_16", 1, 864, 8, 3, 2, 1, (3, 4, 4)),   # cin raised for (e)-(g): class k = 864 .. 6912
    "c3T_32_cin960": ("conv3dT", "conv3dT_32", 1, 960, 17, 3, 2, 1, (3, 3, 4)),  # cin raised for (e)-(g): class k = 960 .. 7680
    "c2_k75": ("conv2d", "conv2d", 1, 3, 8, 5, 2, 2, (9, 11)),
    "c2_two_images": ("conv2d", "conv2d", 2, 8, 16, 3, 1, 1, (5, 7)),            # a 64-pixel tile spans the two images
    "c2_k576": ("conv2d", "conv2d", 1, 64, 70, 3, 1, 1, (4, 5)),                 # 18 runs, two channel tiles
    "c2_k16": ("conv2d", "conv2d", 1, 16, 8, 1, 1, 0, (3, 5)),
    "c2_k2592": ("conv2d", "conv2d", 2, 2592, 8, 1, 1, 0, (5, 7)),               # cin raised for (e)-(g): 81 runs without a padded tap
}

ROW0_OF = {"c3_single": "c3_16_k216", "c3_single_k1728": "c3_16_k1728"}      # the cout = 1 cases: another case's x and weight row 0

# the integer lattices of test_hip_conv3d.py / test_hip_lpips.py (their shapes, bounds and seeds), on which the restatement must equal torch
INT_CONV3D = ((1, 8, 8, 3, 1, 1, 4, 5, 7), (1, 8, 16, 3, 2, 1, 8, 8, 8), (1, 4, 8, 3, 2, 1, 5, 7, 9), (1, 16, 1, 3, 1, 1, 3, 4, 5), (1, 3, 5, 1, 1, 0, 2, 3, 4),
              (1, 33, 65, 3, 1, 1, 3, 3, 3), (2, 8, 8, 3, 1, 1, 5, 7, 11))
INT_CONV3DT = ((8, 4, 1, 1, 1), (16, 8, 2, 3, 5), (33, 17, 3, 2, 2))
INT_CONV2D = ((3, 64, 11, 4, 2, 31, 35), (5, 33, 3, 1, 1, 7, 9), (64, 40, 5, 1, 2, 3, 3), (2, 1, 3, 1, 1, 1, 1))


# ------------------------------------------------------------------------------------------------ the lattice
def _grid(shape, seed, scale, zeros):
    r = np.random.RandomState(seed)
    v = r.randint(-2047, 2048, size=shape).astype(F64)
    if zeros:
        v[r.randint(0, 8, size=shape) == 0] = 0.0
    return (v * scale).astype(F32)


def lattice_x(shape, seed):
    return _grid(shape, seed, 2.0 ** -8, True)


def lattice_w(shape, seed):
    return _grid(shape, seed, 2.0 ** -10, False)


def lattice_b(shape, seed):
    return _grid(shape, seed, 2.0 ** -8, False)


def out_shape(case):
    kind, _, n, cin, cout, K, stride, pad, size = CASES[case] if isinstance(case, str) else case
    if kind == "conv3dT":
        return (n, cout) + tuple(2 * s for s in size)
    return (n, cout) + tuple((s + 2 * pad - K) // stride + 1 for s in size)


@functools.lru_cache(maxsize=None)
def data(name):
    """-> dict x, w (torch's layout for the form), b, skip: read-only float32 numpy arrays."""
    kind, _, n, cin, cout, K, stride, pad, size = CASES[name]
    seed = zlib.crc32(name.encode()) % 100000
    if name in ROW0_OF:
        first = data(ROW0_OF[name])
        x, w = first["x"], first["w"][:1]
    else:
        x = lattice_x((n, cin) + size, seed)
        w = lattice_w((cin, cout) + (K,) * len(size) if kind == "conv3dT" else (cout, cin) + (K,) * len(size), seed + 1)
    d = dict(x=x, w=w, b=lattice_b((cout,), seed + 2), skip=lattice_b(out_shape(name), seed + 3))
    for v in d.values():
        v.setflags(write=False)
    return d


def more_rows(name, rows):
    """`rows` further weight rows [rows,cin,K,K,K] for the launches that put a case's rows into a taller tile."""
    kind, _, n, cin, cout, K, stride, pad, size = CASES[name]
    return lattice_w((rows, cin) + (K,) * len(size), zlib.crc32(name.encode()) % 100000 + 7)


# ------------------------------------------------------------------------------------------------ the sum, in a named order
def _r32(v):
    return v.astype(F32).astype(F64)


def gemm(A, B, order=DOC, group=4):
    """T [M,N] float32 = sum_k A[M,k] B[k,N] in the named order (module docstring); exact on the lattice (`check_lattice`)."""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    M, k = A.shape
    N = B.shape[1]
    run = {"a_chain": max(k, 1), "b_run16": 16, "c_run64": 64}.get(order, RUN)
    sums = []
    for c in range(0, k, run):
        end = min(c + run, k)
        acc = np.zeros((M, N), F64)
        for g0 in range(c, end, group):
            ks = list(range(g0, min(g0 + group, end)))
            if order in ("f_group_exact", "g_group_pairwise"):
                p = [A[:, i, None] * B[i][None, :] for i in ks]
                if order == "f_group_exact":
                    s = p[0]
                    for q in p[1:]:
                        s = s + q                                        # (exact in float64)
                else:
                    while len(p) > 1:
                        p = [_r32(p[i] + p[i + 1]) if i + 1 < len(p) else p[i] for i in range(0, len(p), 2)]
                    s = p[0]
                acc = _r32(acc + s)
            else:
                for i in (ks[::-1] if order == "e_high_first" else ks):
                    acc = _r32(A[:, i, None] * B[i][None, :] + acc)      # the fmaf: exact in float64, rounded once
        sums.append(acc)
    if order == "d_fold_desc":
        sums = sums[::-1]
    T = np.zeros((M, N), F64)
    for s in sums:
        T = _r32(T + s)
    return T.astype(F32)


def check_lattice(A, B, b=None, skip=None):
    """Asserts what the exactness argument needs of one GEMM's operands: the grids, and sum_k |a| |b| < 2^15 for every output (a bound on every
    partial sum in every order)."""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    assert np.array_equal(A * 2.0 ** 10, np.rint(A * 2.0 ** 10)) and float(np.abs(A).max()) <= 2047 * 2.0 ** -10
    assert np.array_equal(B * 2.0 ** 8, np.rint(B * 2.0 ** 8)) and float(np.abs(B).max()) <= 2047 * 2.0 ** -8
    top = float((np.abs(A) @ np.abs(B)).max())
    assert top < SUM_BOUND, top
    for v in (b, skip):
        if v is not None:
            v = np.asarray(v, F64)
            assert np.array_equal(v * 2.0 ** 8, np.rint(v * 2.0 ** 8)) and float(np.abs(v).max()) < 8.0
    return top


def epilogue(T, b, relu, skip):
    """T [n,cout,...] float32 -> y: + bias, the activation, + skip, each one float32 operation."""
    y = (T.astype(F32) + np.asarray(b, F32).reshape((1, -1) + (1,) * (T.ndim - 2))).astype(F32)
    if relu:
        y = np.where(y > 0, y, np.where(y != y, y, F32(0))).astype(F32)
    if skip is not None:
        y = (y + np.asarray(skip, F32)).astype(F32)
    return y


# ------------------------------------------------------------------------------------------------ the forms as GEMMs
def forward_operands(x, w, stride, pad):
    """x [n,cin,*size], w [cout,cin,K..] -> A [cout, cin taps], B [cin taps, n * outputs], the output's spatial shape.  k = ci * taps + t, t the
    flat tap index; a tap in the padding is +0."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    nd, K = x.ndim - 2, w.shape[2]
    n, cin = x.shape[:2]
    out = tuple((s + 2 * pad - K) // stride + 1 for s in x.shape[2:])
    xp = np.pad(x, ((0, 0), (0, 0)) + ((pad, pad),) * nd)
    cols = []
    for t in itertools.product(range(K), repeat=nd):
        at = tuple(slice(t[a], t[a] + stride * (out[a] - 1) + 1, stride) for a in range(nd))
        cols.append(xp[(slice(None), slice(None)) + at])
    B = np.stack(cols, 2)                                                # [n,cin,taps,*out]
    B = B.transpose((1, 2, 0) + tuple(range(3, 3 + nd))).reshape(cin * K ** nd, -1)
    return w.reshape(w.shape[0], -1), B, out


def _forward(x, w, b, stride, pad, relu, skip, order, group):
    A, B, out = forward_operands(x, w, stride, pad)
    n, cout = x.shape[0], w.shape[0]
    T = gemm(A, B, order, group).reshape((cout, n) + out)
    return epilogue(np.moveaxis(T, 0, 1), b, relu, skip)


def conv2d(x, w, b, stride, pad, relu=False, order=DOC):
    return _forward(x, w, b, stride, pad, relu, None, order, GROUP["conv2d"])


def conv3d(x, w, b, stride, pad, relu=False, skip=None, order=DOC):
    return _forward(x, w, b, stride, pad, relu, skip, order, GROUP["conv3d"])


def transposed_operands(x, w, cls):
    """Parity class cls = (pd, ph, pw) of conv_transpose3d(K 3, stride 2, pad 1, output_padding 1): out[o] = sum x[i] w[k] over o = 2 i - 1 + k.
    An even o takes k = 1 (i = o / 2); an odd o takes k = 0 (i = (o + 1) / 2, past the end: +0) and k = 2 (i = (o - 1) / 2), in that order.
    x [n,cin,D,H,W], w [cin,cout,3,3,3] -> A [cout, cin taps], B [cin taps, n D H W] over the class's voxels j (o = 2 j + parity)."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    n, cin, D, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1), (0, 1)))
    axes = [[(1, 0)] if p == 0 else [(0, 1), (2, 0)] for p in cls]       # (k, input offset) per axis, k ascending
    cols, rows = [], []
    for (kd, dd), (kh, dh), (kw, dw) in itertools.product(*axes):
        cols.append(xp[:, :, dd:dd + D, dh:dh + H, dw:dw + W])
        rows.append(w[:, :, kd, kh, kw])                                 # [cin,cout]
    taps = len(cols)
    B = np.stack(cols, 2).transpose(1, 2, 0, 3, 4, 5).reshape(cin * taps, -1)
    A = np.stack(rows, 1).reshape(cin * taps, -1).T                      # [cout, ci * taps + t]
    return np.ascontiguousarray(A), B


def conv3d_transposed(x, w, b, relu=False, skip=None, order=DOC):
    n, cin, D, H, W = x.shape
    cout = w.shape[1]
    T = np.empty((n, cout, 2 * D, 2 * H, 2 * W), F32)
    for cls in itertools.product((0, 1), repeat=3):
        A, B = transposed_operands(x, w, cls)
        t = gemm(A, B, order, GROUP["conv3dT"]).reshape(cout, n, D, H, W)
        T[:, :, cls[0]::2, cls[1]::2, cls[2]::2] = np.moveaxis(t, 0, 1)
    return epilogue(T, b, relu, skip)


def operands(name):
    """Every GEMM of a case: [(A, B)] (one, or the eight classes of the transposed form)."""
    kind, _, n, cin, cout, K, stride, pad, size = CASES[name]
    d = data(name)
    if kind == "conv3dT":
        return [transposed_operands(d["x"], d["w"], cls) for cls in itertools.product((0, 1), repeat=3)]
    return [forward_operands(d["x"], d["w"], stride, pad)[:2]]


@functools.lru_cache(maxsize=None)
def sums(name, order=DOC):
    """T [n,cout,...] of the case in the named order, before the bias (read-only)."""
    kind, _, n, cin, cout, K, stride, pad, size = CASES[name]
    d = data(name)
    zero = np.zeros(cout, F32)
    if kind == "conv2d":
        T = conv2d(d["x"], d["w"], zero, stride, pad, False, order)
    elif kind == "conv3d":
        T = conv3d(d["x"], d["w"], zero, stride, pad, False, None, order)
    else:
        T = conv3d_transposed(d["x"], d["w"], zero, False, None, order)
    T.setflags(write=False)
    return T


def restate(name, relu=False, skip=False, order=DOC):
    """The case's output in the named order."""
    d = data(name)
    return epilogue(sums(name, order), d["b"], relu, d["skip"] if skip else None)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def share(a, b):
    """The share of elements whose bits differ."""
    return float((bits(a) != bits(b)).mean())


def shares(name):
    """{alternative: share of the case's outputs (bias added, no activation, no skip) by which it differs from the documented order}."""
    return {alt: share(restate(name), restate(name, order=alt)) for alt in ALTERNATIVES}


def closest(name, got, relu=False, skip=False):
    """For a failure message: {order: elements of `got` that differ from the case restated in that order}."""
    return {o: int((bits(got) != bits(restate(name, relu, skip, o))).sum()) for o in (DOC,) + ALTERNATIVES}


# ------------------------------------------------------------------------------------------------ torch, for the checks on the restatement
def torch_conv(name_or_kind, x, w, b, stride, pad, dtype):
    kind = CASES[name_or_kind][0] if name_or_kind in CASES else name_or_kind
    x, w, b = (torch.from_numpy(np.array(v)).to(dtype) for v in (x, w, b))
    if kind == "conv2d":
        return F.conv2d(x, w, b, stride=stride, padding=pad)
    if kind == "conv3d":
        return F.conv3d(x, w, b, stride=stride, padding=pad)
    return F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
