"""Case builders and the float64 restatement of multi-view depth fusion (include/ucnerf_hip.h, e1) shared by tests/test_fusion_host.py and
tests/test_hip_fusion.py.  CPU only: nothing here touches a device.  The restatement is the yardstick of the GPU tests, never the kernel.

`consistency_ref` restates ucnerf_depth_consistency in float64 numpy on the float32 inputs the kernel is given, and flags the UNDECIDED pixels:
those with a (pixel, source) pair whose decision float32 rounding may flip -- |e - pix_thresh| <= 1e-3 pix_thresh, |rho - rel_thresh| <= 1e-3
rel_thresh, u / v within 1e-3 of an image bound, |Q.z| or |d'| below 1e-6.  `compact_ref` restates ucnerf_points_compact (float64 points, the
colour rule in float32 as stated).

Lattice cases: a fronto-parallel plane at z0 = 4, identity rotations, fx = fy = 64, integer principal point, translations multiples of
z0 / fx = 1/16 along x / y: every re-projection lands on an integer pixel, every value is dyadic, and the expectations are integer index arithmetic.
Differential cases: a tilted plane and the lower envelope of two planes (each camera's depth map analytic), seeded small rotations and
translations, 10 % of the pixels multiplied by 1.05 .. 2."""
import numpy as np

Z0, FX = 4.0, 64.0
MARGIN = 1e-3
THRESH = dict(pix_thresh=1.0, rel_thresh=0.01, conf_thresh=0.0, min_views=3)


# ------------------------------------------------------------------------------------------------ the restatement
def rigid_inverse(c2w):
    """[R^T | -R^T t] of [N,4,4] in float64 (what the kernel forms when w2cs is not given)."""
    c2w = np.asarray(c2w, dtype=np.float64)
    out = np.zeros_like(c2w)
    out[:, :3, :3] = np.swapaxes(c2w[:, :3, :3], 1, 2)
    out[:, :3, 3] = -np.einsum("nji,nj->ni", c2w[:, :3, :3], c2w[:, :3, 3])
    out[:, 3, 3] = 1
    return out


def _apply(M, P):
    return P @ M[:3, :3].T + M[:3, 3]


def _back(K, x, y, d):
    return np.stack([(x - K[0, 2]) / K[0, 0] * d, (y - K[1, 2]) / K[1, 1] * d, d], -1)


def _proj(K, Q):
    return K[0, 0] * Q[..., 0] / Q[..., 2] + K[0, 2], K[1, 1] * Q[..., 1] / Q[..., 2] + K[1, 2]


def _pos_finite(v):
    return np.isfinite(v) & (v > 0)


def consistency_ref(depth, intrinsics, c2ws, src_ids, w2cs=None, conf=None, pix_thresh=1.0, rel_thresh=0.01, conf_thresh=0.0, min_views=3):
    """-> dict(count uint8, mask bool, fused float64, undecided bool), all [N,H,W]."""
    depth = np.asarray(depth, dtype=np.float64)
    K, c2w = np.asarray(intrinsics, dtype=np.float64), np.asarray(c2ws, dtype=np.float64)
    w2c = rigid_inverse(c2w) if w2cs is None else np.asarray(w2cs, dtype=np.float64)
    src_ids = np.asarray(src_ids).reshape(len(depth), -1)
    N, H, W = depth.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    count, fused = np.zeros((N, H, W), np.int64), np.zeros((N, H, W))
    valid_all, undecided = np.zeros((N, H, W), bool), np.zeros((N, H, W), bool)
    with np.errstate(all="ignore"):
        for r in range(N):
            d = depth[r]
            valid = _pos_finite(d)
            if conf is not None:
                c = np.asarray(conf[r], dtype=np.float64)
                valid &= np.isfinite(c) & (c >= np.float64(np.float32(conf_thresh)))
            X = _apply(c2w[r], _back(K[r], xx, yy, d))
            total = d.copy()
            for s in src_ids[r]:
                s = int(s)
                if s < 0 or s == r or s >= N:
                    continue
                Q = _apply(w2c[s], X)
                und = valid & (np.abs(Q[..., 2]) < 1e-6)
                ok = valid & _pos_finite(Q[..., 2])
                u, v = _proj(K[s], Q)
                und |= ok & ((np.abs(u) <= MARGIN) | (np.abs(u - (W - 1)) <= MARGIN) | (np.abs(v) <= MARGIN) | (np.abs(v - (H - 1)) <= MARGIN))
                ok &= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
                x0, y0 = np.floor(us), np.floor(vs)
                a, b = us - x0, vs - y0
                x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
                dsrc = np.zeros((H, W))
                for wgt, ty, tx in (((1 - a) * (1 - b), y0, x0), (a * (1 - b), y0, x1), ((1 - a) * b, y1, x0), (a * b, y1, x1)):
                    tap = depth[s][ty, tx]
                    used = wgt != 0
                    ok &= ~used | _pos_finite(tap)
                    dsrc = dsrc + np.where(used, wgt * np.where(used, tap, 1.0), 0.0)
                dsrc = np.where(ok, dsrc, 1.0)
                Qr = _apply(w2c[r], _apply(c2w[s], _back(K[s], us, vs, dsrc)))
                dp = Qr[..., 2]
                und |= ok & (np.abs(dp) < 1e-6)
                ok &= _pos_finite(dp)
                xr, yr = _proj(K[r], Qr)
                e = np.hypot(xr - xx, yr - yy)
                rho = np.abs(dp - d) / d
                und |= ok & ((np.abs(e - pix_thresh) <= MARGIN * pix_thresh) | (np.abs(rho - rel_thresh) <= MARGIN * rel_thresh))
                ok &= (e < np.float64(np.float32(pix_thresh))) & (rho < np.float64(np.float32(rel_thresh)))
                count[r] += ok
                total = total + np.where(ok, dp, 0.0)
                undecided[r] |= und
            fused[r] = np.where(valid, total / (count[r] + 1), 0.0)
            count[r] = np.where(valid, count[r], 0)
            valid_all[r] = valid
    return dict(count=count.astype(np.uint8), mask=valid_all & (count >= min_views), fused=fused, undecided=undecided)


def color_rule(rgb):
    """(uint8)(clamp(c, 0, 1) * 255 + 0.5) in float32, NaN -> 0; rgb [...] float32."""
    v = np.asarray(rgb, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    return (v * np.float32(255) + np.float32(0.5)).astype(np.float32).astype(np.uint8)


def points_ref(fused, intrinsics, c2ws):
    """The world point of EVERY pixel in float64: [N,H,W,3]."""
    fused = np.asarray(fused, dtype=np.float64)
    K, c2w = np.asarray(intrinsics, dtype=np.float64), np.asarray(c2ws, dtype=np.float64)
    N, H, W = fused.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([_apply(c2w[n], _back(K[n], xx, yy, fused[n])) for n in range(N)])


def compact_ref(fused, mask, rgb, intrinsics, c2ws):
    """-> (points float64 [total,3], colors uint8 [total,3]) in (view, y, x) order."""
    mask = np.asarray(mask).astype(bool)
    pts = points_ref(fused, intrinsics, c2ws)[mask]
    cols = color_rule(np.moveaxis(np.asarray(rgb), 1, -1)[mask])
    return pts, cols


# ------------------------------------------------------------------------------------------------ cameras
def intrinsics_of(N, H, W, fx=FX, cx=None, cy=None):
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = fx
    K[:, 0, 2] = W // 2 if cx is None else cx
    K[:, 1, 2] = H // 2 if cy is None else cy
    K[:, 2, 2] = 1
    return K


def identity_cams(shifts):
    """c2ws [N,4,4] float32: identity rotations, camera n at (kx, ky, 0) / 16 for shifts[n] = (kx, ky) in pixels at z0."""
    c2w = np.tile(np.eye(4, dtype=np.float32), (len(shifts), 1, 1))
    c2w[:, 0, 3] = np.asarray(shifts, dtype=np.float32)[:, 0] * np.float32(Z0 / FX)
    c2w[:, 1, 3] = np.asarray(shifts, dtype=np.float32)[:, 1] * np.float32(Z0 / FX)
    return c2w


# ------------------------------------------------------------------------------------------------ lattice
LATTICE_SHAPES = ((1, 1), (2, 3), (5, 7), (33, 65))
LATTICE_VIEWS = ((1, 1), (1, 4), (2, 1), (2, 4), (5, 1), (5, 4))       # (N, S)
SHIFTS = ((0, 0), (2, -1), (-3, 1), (1, 2), (-1, -2))


def lattice_case(H, W, N, S, seed=0):
    """-> dict of inputs (depth, intrinsics, c2ws, src_ids, rgb) and the expectations from integer index arithmetic: count [N,H,W] uint8 (the
    sources whose shifted pixel lies inside the image), points [N,H,W,3] float32 (closed form), colors [N,H,W,3] uint8."""
    rs = np.random.RandomState(seed + 131 * H + 17 * W + 7 * N + S)
    shifts = np.array(SHIFTS[:N])
    K = intrinsics_of(N, H, W)
    c2w = identity_cams(shifts)
    src = np.array([[(r + 1 + j) % N for j in range(S)] for r in range(N)], dtype=np.int32)      # holds r itself when S >= N: skipped by rule
    if S > 1:
        src[:, S - 1] = -1                                                                        # and one empty slot
    depth = np.full((N, H, W), Z0, np.float32)
    rgb = rs.uniform(-0.2, 1.2, (N, 3, H, W)).astype(np.float32)
    flat = rgb.reshape(-1)
    special = np.array([np.nan, 0.0, 1.0, -0.0, 0.5, 127.5 / 255, 254.5 / 255, 2.0, -3.0, np.inf, -np.inf], np.float32)
    flat[rs.permutation(flat.size)[:min(len(special), flat.size)]] = special[:min(len(special), flat.size)]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    count = np.zeros((N, H, W), np.int64)
    for r in range(N):
        for s in src[r]:
            if s < 0 or s == r:
                continue
            dx, dy = shifts[r] - shifts[s]
            count[r] += (xs + dx >= 0) & (xs + dx <= W - 1) & (ys + dy >= 0) & (ys + dy <= H - 1)
    pts = np.zeros((N, H, W, 3), np.float32)
    for n in range(N):
        pts[n, ..., 0] = (xs - K[n, 0, 2]).astype(np.float32) / np.float32(FX) * np.float32(Z0) + c2w[n, 0, 3]
        pts[n, ..., 1] = (ys - K[n, 1, 2]).astype(np.float32) / np.float32(FX) * np.float32(Z0) + c2w[n, 1, 3]
        pts[n, ..., 2] = Z0
    return dict(depth=depth, intrinsics=K, c2ws=c2w, src_ids=src, rgb=rgb, count=count.astype(np.uint8), points=pts,
                colors=color_rule(np.moveaxis(rgb, 1, -1)), shifts=shifts)


# ------------------------------------------------------------------------------------------------ differential scenes
DIFF_CASES = (("tilted", 24, 40, 3, True), ("tilted", 33, 65, 5, False), ("two-plane", 24, 40, 7, False), ("two-plane", 33, 65, 11, True))
DIFF_IDS = ["%s-%dx%d-%s" % (c[0], c[1], c[2], "w2c" if c[4] else "rigid") for c in DIFF_CASES]
PLANES = {"tilted": (((0.15, -0.1, 1.0), 4.0),), "two-plane": (((0.3, 0.1, 1.0), 4.2), ((-0.25, -0.05, 1.0), 4.0))}


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def diff_case(name, H, W, seed, give_w2c, N=5, S=4):
    """-> dict(depth, intrinsics, c2ws, w2cs (float32 of the float64 inverse, or None: the kernel's rigid inverse), src_ids, rgb)."""
    rs = np.random.RandomState(seed)
    K = intrinsics_of(N, H, W, fx=1.5 * W, cx=W / 2, cy=H / 2)
    c2w = np.tile(np.eye(4), (N, 1, 1))
    for n in range(N):
        c2w[n, :3, :3] = _rodrigues(rs.uniform(-0.04, 0.04, 3))
        c2w[n, :3, 3] = rs.uniform(-0.3, 0.3, 3) * (1, 1, 0.3)
    c2w32 = c2w.astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((N, H, W))
    for n in range(N):
        dcam = np.stack([(xx - K[n, 0, 2]) / K[n, 0, 0], (yy - K[n, 1, 2]) / K[n, 1, 1], np.ones_like(xx)], -1)
        dw = dcam @ c2w32[n, :3, :3].astype(np.float64).T
        z = np.full((H, W), np.inf)
        for normal, c in PLANES[name]:
            normal = np.asarray(normal)
            z = np.minimum(z, (c - normal @ c2w32[n, :3, 3].astype(np.float64)) / (dw @ normal))
        depth[n] = z
    assert np.isfinite(depth).all() and depth.min() > 1
    out = rs.rand(N, H, W) < 0.10
    depth = np.where(out, depth * rs.uniform(1.05, 2.0, (N, H, W)), depth).astype(np.float32)
    src = np.array([[(r + 1 + j) % N for j in range(S)] for r in range(N)], dtype=np.int32)
    w2c = np.linalg.inv(c2w32.astype(np.float64)).astype(np.float32) if give_w2c else None
    rgb = rs.rand(N, 3, H, W).astype(np.float32)
    return dict(depth=depth, intrinsics=K, c2ws=c2w32, w2cs=w2c, src_ids=src, rgb=rgb)


_diff_cache = {}


def diff_ref(i):
    """(case, restatement) of DIFF_CASES[i], computed once and shared: do not modify."""
    if i not in _diff_cache:
        case = diff_case(*DIFF_CASES[i])
        _diff_cache[i] = (case, consistency_ref(case["depth"], case["intrinsics"], case["c2ws"], case["src_ids"], w2cs=case["w2cs"], **THRESH))
    return _diff_cache[i]


# ------------------------------------------------------------------------------------------------ compaction
ITEMS, CHUNK = 1024, 256        # ops.COMPACT_BLOCK_ITEMS, ops.COMPACT_SCAN_CHUNK (asserted equal in tests/test_fusion_host.py)
# (N, H, W, mask kind): pixel counts on both sides of one workgroup (1023, 1024, 1025), several workgroups with a ragged end, about 70 k pixels
# (69 workgroup counts), and both sides of the scan's second pass (256 * 1024 = 262144 pixels: 262143, 262144, 262145 -> 256, 256, 257 counts)
COMPACT_CASES = ((1, 1, 1, "all"), (1, 3, 5, "none"), (1, 31, 33, "all"), (1, 32, 32, "all"), (1, 25, 41, "all"), (2, 33, 65, "alternating"),
                 (3, 33, 65, "random"), (2, 137, 257, "random"), (1, 3, 87381, "random"), (1, 512, 512, "all"), (1, 5, 52429, "random"))
COMPACT_IDS = ["%dx%dx%d-%s" % c for c in COMPACT_CASES]


def compact_case(N, H, W, kind, seed=5):
    rs = np.random.RandomState(seed + N * H * W)
    n = N * H * W
    mask = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0, "random": rs.rand(n) < 0.37}[kind].reshape(N, H, W)
    fused = rs.uniform(1.0, 6.0, (N, H, W)).astype(np.float32)
    rgb = rs.uniform(-0.1, 1.1, (N, 3, H, W)).astype(np.float32)
    K = intrinsics_of(N, H, W, fx=1.2 * W, cx=W / 2, cy=H / 2)
    c2w = np.tile(np.eye(4), (N, 1, 1))
    for k in range(N):
        c2w[k, :3, :3] = _rodrigues(rs.uniform(-0.3, 0.3, 3))
        c2w[k, :3, 3] = rs.uniform(-1, 1, 3)
    return dict(fused=fused, mask=mask, rgb=rgb, intrinsics=K, c2ws=c2w.astype(np.float32))
