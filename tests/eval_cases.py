"""Cases and numpy references for the evaluation-metric kernels (tests/test_eval_cases_host.py, tests/test_hip_eval_metrics.py).

REFERENCES.  utils/evaluation.py restated in numpy, once in float32 operation for operation (what the reference computes on float32 inputs;
pinned to its own output by fixture G20) and once in float64 (medians, ratio and every later operation in float64 on the same pixels: the
validity test and the clamp bounds are float32(min_depth), float32(max_depth) in both, so that the two differ by arithmetic precision only).
SSIM is skimage.metrics.structural_similarity(data_range=1, channel_axis=2) restated from its documented default: uniform 7 x 7 window per
channel, K1 = 0.01, K2 = 0.03, sample covariance (49 / 48), the mean of S over the windows that lie inside the image, then over the channels.

MEDIAN cases: one image of 1 x (N + 2) pixels with N valid ones (two are invalid: gt = 0 and gt = 150), for every N of MEDIAN_N and every kind
of MEDIAN_KINDS; the expected medians, ratio and counts are the float32 restatement's (np.median), compared bit for bit / as integers.

EXACT error cases: ground truth in {1, 2, 4, 8}, d = gt - pred a multiple of 1/4 with |d| <= gt / 2, both medians exactly 2 (ratio exactly 1), the
valid count of every image a power of two.  d^2 is a multiple of 1/16 (<= 16), |d| / gt of 1/32 (<= 1/2), d^2 / gt of 1/128 (<= 2): every partial
sum of at most 4096 terms is an integer below 2^21 in its unit, so no addition rounds and abs_rel, sq_rel, rmse do not depend on the association
order; check_exact asserts the float32 and float64 restatements agree exactly.  rmse_log is not exact (log) and is left out.

EXACT image cases: pixels are multiples of 1/16, squared differences multiples of 1/256 (<= 1), sums of at most 3 x 64 x 64 of them below 2^22
units: exact.  The expected mse is float32(sum) / float32(3 H W), ONE correctly rounded division -- the reference's three nested means round
three times, which is why the closed form and not the restatement is the expectation there.

CONTINUOUS cases and bars: random depths and images; bars()[name] = 4 x the float32 restatement's largest distance from the float64 one over the
continuous cases (the standing rule of profiles/composite_edges.md).  The bars move with the host's log / log10."""
import functools
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

F32, F64 = np.float32, np.float64
ERR_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log")
IMG_NAMES = ("mse", "psnr", "ssim")
BAR_NAMES = ERR_NAMES + IMG_NAMES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SSIM_TILE = 16                                       # windows per tile side of ssim_tile_kernel (csrc/metrics.hip)


# ------------------------------------------------------------------------------------------------ references
def compute_errors(gt, pred):
    """utils/evaluation.py:8-26 in the dtype of its arguments; returns the seven values and the three counts."""
    thresh = np.maximum((gt / pred), (pred / gt))
    counts = [int((thresh < t).sum()) for t in (1.25, 1.25 ** 2, 1.25 ** 3)]
    a1, a2, a3 = [(thresh < t).mean() for t in (1.25, 1.25 ** 2, 1.25 ** 3)]
    rmse = (gt - pred) ** 2
    rmse = np.sqrt(rmse.mean())
    rmse_log = (np.log(gt) - np.log(pred)) ** 2
    rmse_log = np.sqrt(rmse_log.mean())
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    return (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3), counts


def depth_reference(gt, pred, mask=None, min_depth=0.0001, max_depth=100, dtype=F32):
    """utils/evaluation.py:29-69 in `dtype`.  gt, pred [n,H,W] float32, mask [n,H,W] uint8 or None.  Returns dict: empty, ratio, medians,
    counts [n,4] (valid, a1, a2, a3), errors [n,7] float64 (NaN rows for the images left out), flags [n], mean [7] float64."""
    assert gt.dtype == F32 and pred.dtype == F32 and gt.shape == pred.shape and gt.ndim == 3
    n = gt.shape[0]
    lo, hi = F32(min_depth), F32(max_depth)
    gts, preds, kept = [], [], []
    counts = np.zeros((n, 4), np.int64)
    errors = np.full((n, 7), np.nan, F64)
    for i in range(n):
        m = (gt[i] > lo) * (gt[i] < hi)
        if mask is not None:
            m = m * (mask[i].astype(np.uint8) > 0.5)
        if m.sum() == 0:
            continue
        gts.append(gt[i][m].astype(dtype))
        preds.append(pred[i][m].astype(dtype))
        kept.append(i)
    out = dict(empty=not kept, counts=counts, errors=errors, flags=np.array([i not in kept for i in range(n)]))
    if not kept:
        out.update(ratio=dtype(np.nan), medians=(dtype(np.nan), dtype(np.nan)), mean=np.full(7, np.nan))
        return out
    med_g, med_p = np.median(np.concatenate(gts)), np.median(np.concatenate(preds))
    ratio = med_g / med_p
    assert ratio.dtype == dtype
    for i, g, q in zip(kept, gts, preds):
        with np.errstate(all="ignore"):
            q = q * ratio
            q[q < dtype(lo)] = dtype(lo)
            q[q > dtype(hi)] = dtype(hi)
            e, c = compute_errors(g, q)
        assert q.dtype == dtype and all(np.asarray(v).dtype == dtype for v in e[:4])
        errors[i] = e
        counts[i] = [g.size] + c
    out.update(ratio=ratio, medians=(med_g, med_p), mean=errors[kept].mean(0))
    return out


def ssim_reference(gt, pred, dtype=F64):
    """[n,3,H,W] -> per-image SSIM [n] in `dtype` (the windows' means by sliding_window_view: direct sums, no cumulative-sum cancellation)."""
    x, y = gt.astype(dtype), pred.astype(dtype)
    c1, c2, cov = dtype(0.01 ** 2), dtype(0.03 ** 2), dtype(49.0 / 48.0)
    win = lambda a: sliding_window_view(a, (7, 7), axis=(-2, -1)).mean((-2, -1), dtype=dtype)      # noqa: E731
    ux, uy, uxx, uyy, uxy = win(x), win(y), win(x * x), win(y * y), win(x * y)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert s.dtype == dtype and s.shape[-2:] == (gt.shape[-2] - 6, gt.shape[-1] - 6)
    return s.mean((-2, -1), dtype=dtype).mean(-1, dtype=dtype)


def image_reference(gt, pred, dtype=F32):
    """utils/evaluation.py:82-83 (per image) and the SSIM restatement, in `dtype`: dict mse [n], psnr [n], ssim [n]."""
    assert gt.dtype == F32 and pred.dtype == F32 and gt.shape == pred.shape and gt.ndim == 4 and gt.shape[1] == 3
    g, q = gt.astype(dtype), pred.astype(dtype)
    mse = ((g - q) ** 2).mean(-1).mean(-1).mean(-1)
    with np.errstate(divide="ignore"):
        psnr = -10 * np.log10(mse)
    assert mse.dtype == dtype and psnr.dtype == dtype
    small = gt.shape[-2] < 7 or gt.shape[-1] < 7                     # (no window fits: skimage raises; the image error stands on its own)
    return dict(mse=mse, psnr=psnr, ssim=np.full(gt.shape[0], np.nan, dtype) if small else ssim_reference(gt, pred, dtype))


def same_bits(a, b):
    """Equal as float32 values (+0 == -0), NaN matching NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(((a == b) | ((a != a) & (b != b))).all())


# ------------------------------------------------------------------------------------------------ median cases
MEDIAN_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MEDIAN_KINDS = ("random", "equal", "ties", "ulp", "binades", "negative", "last_image", "masked")
BIG_KINDS = ("random", "ties", "negative")          # on one 256 x 320 image: several blocks and the global histogram take part
BIG_HW = (256, 320)


def _median_values(N, kind, rng):
    """(gt [N], pred [N]) valid pixels, shuffled."""
    g = rng.uniform(0.5, 10.0, N).astype(F32)
    q = rng.uniform(0.3, 8.0, N).astype(F32)
    if kind == "equal":
        g[:], q[:] = 2.0, 3.0
    elif kind == "ties":                             # the middle third (at least the middle value) is one value: ties straddle the middle
        a, b = N // 3, max(N - N // 3, N // 3 + 1)
        g, q = np.sort(g), np.sort(q)
        g[a:b], q[a:b] = g[N // 2], q[N // 2]
    elif kind == "ulp":                              # the two middle values differ in the last mantissa bit only
        g, q = np.sort(g), np.sort(q)
        k = max(N // 2 - 1, 0)
        for v, mid in ((g, F32(3.1415927)), (q, F32(1.7320508))):
            v[:k] = rng.uniform(0.5, 1.0, k)
            v[k] = mid
            if k + 1 < N:
                v[k + 1] = np.nextafter(mid, F32(np.inf))
                v[k + 2:] = rng.uniform(4.0, 8.0, N - k - 2)
    elif kind == "binades":                          # pred over 30 binades; gt over the 19 that min_depth .. max_depth hold
        g = (2.0 ** rng.uniform(-13.0, 6.5, N)).astype(F32)
        q = (2.0 ** rng.uniform(-15.0, 15.0, N)).astype(F32)
    elif kind == "negative":                         # the key transform: negative values, -0.0 and +0.0 among the predictions
        q = rng.uniform(-4.0, 6.0, N).astype(F32)
        if N >= 63:                                  # a few zeros of both signs, away from the middle rank: np.median takes -0.0 == +0.0 in whatever
            neg = np.flatnonzero(q < 0)              # order its partition leaves them, the selection sorts -0.0 first, so a median AT zero may differ
            q[neg[:2]], q[neg[2:4]] = np.copysign(F32(0), F32(-1)), F32(0)      # in sign (and with it the sign of an infinite ratio): not a case with one right answer
    perm = rng.permutation(N)
    return g[perm], q[perm]


def _with_invalid(g, q, rng):
    """Two invalid pixels (gt = 0 at the front, gt = 150 in the middle) around N valid ones: [1, N + 2]."""
    N = g.size
    gt, pred = np.empty(N + 2, F32), rng.uniform(0.3, 8.0, N + 2).astype(F32)
    at = np.ones(N + 2, bool)
    at[0] = at[1 + N // 2] = False
    gt[at], pred[at] = g, q
    gt[0], gt[1 + N // 2] = 0.0, 150.0
    return gt[None], pred[None]


def median_case(N, kind):
    rng = np.random.default_rng(1000 * N + MEDIAN_KINDS.index(kind))
    g, q = _median_values(N, "random" if kind in ("last_image", "masked") else kind, rng)
    gt, pred = _with_invalid(g, q, rng)
    mask = None
    if kind == "last_image":                         # three images, the valid pixels confined to the last
        z = np.zeros_like(gt)
        gt, pred = np.stack([z, z, gt]), np.stack([pred + 1, pred + 2, pred])
    elif kind == "masked":                           # image 0 has valid depths of another scale: the uint8 mask removes every pixel of it
        gt, pred = np.stack([gt * 3, gt]), np.stack([pred * 5, pred])
        mask = np.stack([np.zeros(gt.shape[1:], np.uint8), np.full(gt.shape[1:], 255, np.uint8)])
        mask[1, 0, 0] = 0                            # (already invalid)
    else:
        gt, pred = gt[None], pred[None]
    return _finish_depth_case("median_N%d_%s" % (N, kind), gt.reshape(-1, 1, N + 2), pred.reshape(-1, 1, N + 2),
                              None if mask is None else mask.reshape(-1, 1, N + 2), N)


def big_median_case(kind):
    H, W = BIG_HW
    rng = np.random.default_rng(77 + MEDIAN_KINDS.index(kind))
    N = H * W - 2
    g, q = _median_values(N, kind, rng)
    gt, pred = _with_invalid(g, q, rng)
    return _finish_depth_case("median_big_%s" % kind, gt.reshape(1, H, W), pred.reshape(1, H, W), None, N)


def _finish_depth_case(name, gt, pred, mask, n_valid=None):
    gt, pred = np.ascontiguousarray(gt, F32), np.ascontiguousarray(pred, F32)
    case = dict(name=name, gt=gt, pred=pred, mask=mask, min_depth=0.0001, max_depth=100)
    with np.errstate(all="ignore"):
        case["f32"] = depth_reference(gt, pred, mask, dtype=F32)
        case["f64"] = depth_reference(gt, pred, mask, dtype=F64)
    # self-checks: the two restatements select the same pixels, and the float32 medians are the float64 ones up to the one rounding of the mean
    assert np.array_equal(case["f32"]["counts"][:, 0], case["f64"]["counts"][:, 0]) and np.array_equal(case["f32"]["flags"], case["f64"]["flags"])
    if n_valid is not None:
        assert int(case["f32"]["counts"][:, 0].sum()) == n_valid, name
    if not case["f32"]["empty"]:
        for a, b in zip(case["f32"]["medians"], case["f64"]["medians"]):
            assert a.dtype == F32 and abs(float(a) - float(b)) <= 2.0 ** -23 * abs(float(b)), name
    return case


MEDIAN_BUILDERS = {"median_N%d_%s" % (N, k): functools.partial(median_case, N, k) for N in MEDIAN_N for k in MEDIAN_KINDS}
MEDIAN_BUILDERS.update({"median_big_%s" % k: functools.partial(big_median_case, k) for k in BIG_KINDS})
MEDIAN_NAMES = tuple(MEDIAN_BUILDERS)


@functools.lru_cache(maxsize=None)
def median(name):
    return MEDIAN_BUILDERS[name]()


def check_median_case(case):
    """What a kind promises, read off the case itself (so that a slip in a builder cannot pass for coverage)."""
    name, r = case["name"], case["f32"]
    kind = name.split("_", 2)[2]
    valid = (case["gt"] > F32(1e-4)) & (case["gt"] < F32(100))
    if case["mask"] is not None:
        valid &= case["mask"] > 0
    g, q = np.sort(case["gt"][valid]), np.sort(case["pred"][valid])
    N = g.size
    lo, hi = (N - 1) // 2, N // 2
    assert same_bits(r["medians"][0], (g[lo] + g[hi]) / F32(2)) and same_bits(r["medians"][1], (q[lo] + q[hi]) / F32(2)), name
    if kind == "equal":
        assert g[0] == g[-1] and q[0] == q[-1]
    elif kind == "ties" and N >= 3:
        assert g[lo - 1] == g[hi] == g[min(hi + 1, N - 1)] or N < 6
        assert g[lo] == g[hi]
    elif kind == "ulp" and N >= 2:
        assert q[N // 2] == np.nextafter(q[N // 2 - 1], F32(np.inf)) and g[N // 2] == np.nextafter(g[N // 2 - 1], F32(np.inf))
    elif kind == "binades" and N >= 63:
        assert np.log2(q[-1] / q[0]) > 25 and np.log2(g[-1] / g[0]) > 15
    elif kind == "negative" and N >= 63:
        raw = case["pred"][valid]                    # (unsorted: a vectorised sort need not keep the sign of a zero)
        assert (q < 0).sum() > N // 5 and (np.signbit(raw) & (raw == 0)).sum() == 2 and (~np.signbit(raw) & (raw == 0)).sum() == 2
    if kind == "negative":
        assert q[lo] != 0 and q[hi] != 0, name       # (see _median_values)
    elif kind == "last_image":
        assert list(r["flags"]) == [True, True, False]
    elif kind == "masked":
        assert list(r["flags"]) == [True, False] and ((case["gt"][0] > 1e-4) & (case["gt"][0] < 100)).sum() == N
    return N


# ------------------------------------------------------------------------------------------------ exact error cases
EXACT_SPECS = {"exact_N4": (1, 4), "exact_N64": (1, 64), "exact_N1024_x3": (3, 1024), "exact_N4096": (1, 4096)}


def exact_case(name):
    n, N = EXACT_SPECS[name]
    rng = np.random.default_rng(31 * N + n)
    gts, preds = [], []
    for _ in range(n):
        g = np.concatenate([np.full(N // 4, 1.0), np.full(N // 2, 2.0), rng.choice([4.0, 8.0], N // 4)]).astype(F32)
        steps = lambda lo, hi, k: rng.integers(lo, hi + 1, k) / 4.0      # noqa: E731  multiples of 1/4 in [lo / 4, hi / 4]
        d = np.empty(N, F32)
        d[:N // 4] = steps(-2, 2, N // 4)                                  # gt 1: pred in [0.5, 1.5], below 2
        two = N // 2
        below = (two - 2) // 2
        d[N // 4:N // 4 + 2] = 0.0                                         # two predictions of exactly 2: the middle ranks
        d[N // 4 + 2:N // 4 + 2 + below] = steps(1, 4, below)              # gt 2: pred in [1, 1.75]
        d[N // 4 + 2 + below:N // 4 + two] = steps(-4, -1, two - 2 - below)      # pred in [2.25, 3]
        hi_g = g[N // 4 + two:]
        d[N // 4 + two:] = np.where(hi_g == 4.0, steps(-8, 7, N // 4), steps(-16, 16, N // 4))      # pred in [2.25, 6] / [4, 12], above 2
        perm = rng.permutation(N)
        g, q = g[perm], (g - d)[perm]
        gt, pred = np.zeros(N + 3, F32), np.full(N + 3, 5.0, F32)          # three invalid pixels: N + 3 is no multiple of anything
        at = np.ones(N + 3, bool)
        at[[0, N // 2, N + 2]] = False
        gt[at], pred[at] = g, q
        gts.append(gt)
        preds.append(pred)
    case = _finish_depth_case(name, np.stack(gts)[:, None, :], np.stack(preds)[:, None, :], None, n * N)
    check_exact(case, N)
    return case


def check_exact(case, N):
    a, b = case["f32"], case["f64"]
    assert N & (N - 1) == 0 and N % 4 == 0
    assert float(a["ratio"]) == 1.0 and float(b["ratio"]) == 1.0 and float(a["medians"][0]) == 2.0 == float(a["medians"][1]), case["name"]
    valid = case["gt"] > 0
    g, q = case["gt"][valid].astype(F64), case["pred"][valid].astype(F64)
    d = g - q
    assert bool((np.log2(g) % 1 == 0).all()) and bool(((4 * d) % 1 == 0).all()) and bool((np.abs(d) <= g / 2).all())
    assert float((d * d).max()) * N * 16 < 2 ** 24 and float((d * d / g).max()) * N * 128 < 2 ** 24 and float((np.abs(d) / g).max()) * N * 32 < 2 ** 24
    assert bool(((d * d / g * 128) % 1 == 0).all()) and bool(((np.abs(d) / g * 32) % 1 == 0).all())
    assert np.array_equal(a["counts"], b["counts"]) and bool((a["counts"][:, 0] == N).all())
    for k in (0, 1, 2):                              # abs_rel, sq_rel, rmse: the float64 restatement rounded to float32 IS the float32 one
        assert same_bits(a["errors"][:, k], b["errors"][:, k].astype(F32)), (case["name"], ERR_NAMES[k])
    # closed forms, from integer arithmetic
    for i in range(case["gt"].shape[0]):
        v = case["gt"][i] > 0
        gi, di = case["gt"][i][v].astype(F64), (case["gt"][i][v].astype(F64) - case["pred"][i][v].astype(F64))
        want = (np.abs(di) / gi).sum() / N, (di * di / gi).sum() / N, np.sqrt((di * di).sum() / N)
        assert same_bits(a["errors"][i, :3], np.array(want).astype(F32)), case["name"]


@functools.lru_cache(maxsize=None)
def exact(name):
    return exact_case(name)


# ------------------------------------------------------------------------------------------------ exact image cases
EXACT_IMAGE_HW = ((1, 1), (7, 9), (64, 64))
EXACT_IMAGE_N = (1, 3)


@functools.lru_cache(maxsize=None)
def exact_image(n, H, W):
    """(gt, pred [n,3,H,W], expected mse [n] float32).  H, W may be below the SSIM window: such a size is run with ssim=False."""
    rng = np.random.default_rng(100 * H + W + n)
    gt = (rng.integers(0, 17, (n, 3, H, W)) / 16.0).astype(F32)
    pred = (rng.integers(0, 17, (n, 3, H, W)) / 16.0).astype(F32)
    d = gt.astype(F64) - pred.astype(F64)
    total = (d * d).reshape(n, -1).sum(-1)
    assert bool(((d * d * 256) % 1 == 0).all()) and float(total.max()) * 256 < 2 ** 24
    want = total.astype(F32) / F32(3 * H * W)
    assert bool((total.astype(F32).astype(F64) == total).all()) and want.dtype == F32
    return gt, pred, want


# ------------------------------------------------------------------------------------------------ continuous cases
def load_g20():
    with np.load(os.path.join(GOLDEN, "g20_depth_eval.npz")) as z:
        return {k: z[k] for k in z.files}


def _cont_depth(name):
    if name == "g20":
        g = load_g20()
        return _finish_depth_case("cont_g20", g["gt_depths"], g["pred_depths"], None)
    n, H, W, masked = {"d_9x11": (2, 9, 11, False), "d_37x53": (3, 37, 53, True), "d_256x320": (2, 256, 320, True)}[name]
    rng = np.random.default_rng(H * W + n)
    gt = rng.uniform(0.5, 12.0, (n, H, W)).astype(F32)
    pred = (gt * rng.uniform(0.6, 1.9, (n, H, W)) * 0.37).astype(F32)      # (a scale the median ratio has to undo; thresholds on both sides of 1.25^k)
    gt[:, H // 3] = 0.0                                                    # a band without ground truth
    gt[0, :2, :5] = 200.0
    pred[rng.random((n, H, W)) < 0.01] = 1e-7                              # the lower clamp bites after scaling
    pred[rng.random((n, H, W)) < 0.01] = 1e4                               # ... and the upper one
    mask = None
    if masked:
        mask = (rng.random((n, H, W)) < 0.8).astype(np.uint8) * 255
    return _finish_depth_case("cont_" + name, gt, pred, mask)


CONT_DEPTH_NAMES = ("g20", "d_9x11", "d_37x53", "d_256x320")
CONT_IMAGE_SPECS = {"i_9x11": (2, 9, 11, "random"), "i_33x47": (3, 33, 47, "random"), "i_40x40_near": (2, 40, 40, "near"), "i_256x320": (1, 256, 320, "near")}
CONT_IMAGE_NAMES = tuple(CONT_IMAGE_SPECS)


@functools.lru_cache(maxsize=None)
def cont_depth(name):
    return _cont_depth(name)


def image_pair(n, H, W, kind, seed=0):
    """gt, pred [n,3,H,W] in [0,1]: 'random' pair, 'near' (a smooth image and a noisy rendering of it), 'identical', 'constant', 'complement'."""
    rng = np.random.default_rng(7 * H + W + n + seed)
    if kind == "near":
        yy, xx = np.mgrid[0:H, 0:W]
        base = 0.5 + 0.4 * np.sin(xx / 5.0 + np.arange(3)[:, None, None]) * np.cos(yy / 7.0)
        gt = np.broadcast_to(base, (n, 3, H, W)) + rng.uniform(-0.05, 0.05, (n, 3, H, W))
        pred = gt + rng.normal(0, 0.02, (n, 3, H, W))
    else:
        gt = rng.random((n, 3, H, W))
        pred = rng.random((n, 3, H, W))
    gt, pred = np.clip(gt, 0, 1).astype(F32), np.clip(pred, 0, 1).astype(F32)
    if kind == "identical":
        pred = gt.copy()
    elif kind == "constant":
        gt = np.full((n, 3, H, W), 0.3, F32)
        pred = gt.copy()
    elif kind == "complement":
        pred = F32(1) - gt
    return np.ascontiguousarray(gt), np.ascontiguousarray(pred)


@functools.lru_cache(maxsize=None)
def image_case(n, H, W, kind):
    gt, pred = image_pair(n, H, W, kind)
    return dict(name="img_%dx%dx%d_%s" % (n, H, W, kind), gt=gt, pred=pred, f32=image_reference(gt, pred, F32), f64=image_reference(gt, pred, F64))


def cont_image(name):
    return image_case(*CONT_IMAGE_SPECS[name])


def depth_distances(errors, ref64):
    """Max |value - float64 reference| per error name over the images that are kept (NaN rows must agree -> inf)."""
    errors, want = np.asarray(errors, F64), ref64["errors"]
    keep = ~ref64["flags"]
    if not np.array_equal(np.isnan(errors[:, :4]).any(1), ref64["flags"]):
        return dict.fromkeys(ERR_NAMES, float("inf"))
    return {k: float(np.abs(errors[keep, j] - want[keep, j]).max()) if keep.any() else 0.0 for j, k in enumerate(ERR_NAMES)}


def image_distances(got, ref64):
    return {k: float(np.abs(np.asarray(got[k], F64) - ref64[k]).max()) for k in IMG_NAMES}


@functools.lru_cache(maxsize=None)
def bars():
    """{name: 4 x the float32 restatement's largest distance from the float64 one over the continuous cases}."""
    worst = dict.fromkeys(BAR_NAMES, 0.0)
    for name in CONT_DEPTH_NAMES:
        c = cont_depth(name)
        assert np.array_equal(c["f32"]["counts"][:, 0], c["f64"]["counts"][:, 0])
        for k, v in depth_distances(c["f32"]["errors"], c["f64"]).items():
            worst[k] = max(worst[k], v)
    for name in CONT_IMAGE_NAMES:
        c = cont_image(name)
        for k, v in image_distances(c["f32"], c["f64"]).items():
            worst[k] = max(worst[k], v)
    assert all(0 < v < float("inf") for v in worst.values()), worst
    return {k: 4.0 * v for k, v in worst.items()}


def over_the_bar(dist, what):
    b = bars()
    return ["%s %s: %.3e > bar %.3e" % (what, k, v, b[k]) for k, v in dist.items() if not v <= b[k]]


def ssim_one_window(gt, pred):
    """Closed form of a 7 x 7 image pair [3,7,7] in float64: one window per channel."""
    out = []
    for c in range(3):
        x, y = gt[c].astype(F64).ravel(), pred[c].astype(F64).ravel()
        ux, uy = x.sum() / 49, y.sum() / 49
        vx, vy, vxy = ((x - ux) ** 2).sum() / 48, ((y - uy) ** 2).sum() / 48, ((x - ux) * (y - uy)).sum() / 48      # the sample covariance itself
        out.append((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4)))
    return float(np.mean(out))
