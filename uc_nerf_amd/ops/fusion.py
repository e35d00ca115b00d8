"""Multi-view depth fusion on the device: the geometric consistency filter over per-view depth maps (one launch) and the compaction of the
surviving pixels to a coloured point cloud (one ABI call, a counted fixed-order scan).  No atomics: two calls on the same inputs give the same
bits.  include/ucnerf_hip.h (e1) has the arithmetic order and every rule for invalid inputs."""
import torch

from .. import _lib as L
from ._core import _dev, _dev_as, _f32, _launch, _ptr

FUSION_MAX_SRC = 32            # source slots of one depth_consistency call (a workgroup keeps their matrices in LDS)
COMPACT_BLOCK_ITEMS = 1024     # pixels a workgroup of the compaction counts and ranks
COMPACT_SCAN_CHUNK = 256       # workgroup counts the scan takes in one pass (a second pass starts at 256 * 1024 pixels)


def _views(name, t, N, tail, dev, what):
    t = _f32(t, name)
    if t.device != dev or tuple(t.shape) != (N,) + tail:
        raise RuntimeError("uc_nerf_amd.%s: %s must be a float32 %s tensor on %s, got %s on %s"
                           % (what, name, list((N,) + tail), dev, list(t.shape), t.device))
    return t


def depth_consistency(depth, intrinsics, c2ws, src_ids, w2cs=None, conf=None, pix_thresh=1.0, rel_thresh=0.01, conf_thresh=0.0, min_views=3):
    """The geometric consistency filter of the MVSNet / CasMVSNet fusion step over N views: ucnerf_depth_consistency, ONE launch on the current
    stream, nothing synchronised or read back.  depth [N,H,W] z-depth; intrinsics [N,3,3] with ZERO SKEW; c2ws [N,4,4]; src_ids int32 [N,S],
    S <= FUSION_MAX_SRC: the source views of every view, an entry < 0, == the view itself or >= N is skipped; w2cs [N,4,4] or None = the RIGID
    inverse of c2ws formed on the device ([R^T | -R^T t], the translation -fmaf(R[2][r], t[2], fmaf(R[1][r], t[1], R[0][r] * t[0])); not an
    LU inverse); conf [N,H,W] or None.  All float32 on one ROCm device.
    A pixel (x, y) of view r is valid iff its depth d is finite and > 0 and (with conf) its conf is finite and >= conf_thresh.  A source s is
    consistent with it iff the pixel's world point projects into s in front of the camera and inside [0, W-1] x [0, H-1], the bilinear sample of
    depth_s there touches only finite depths > 0 (a tap of weight 0 is not read), and the sample back-projected from s and projected into r
    lands at (x', y', d') with d' finite and > 0, |(x' - x, y' - y)| < pix_thresh and |d' - d| / d < rel_thresh.
    -> (mask bool [N,H,W] = valid and count >= min_views, fused float32 [N,H,W] = (d + the consistent d' in source order) / (count + 1), 0 where
    the pixel is not valid, count uint8 [N,H,W])."""
    dev = _dev(depth)
    depth = _f32(depth, "depth")
    if depth.dim() != 3:
        raise RuntimeError("uc_nerf_amd.depth_consistency: depth must be [N,H,W], got %s" % (tuple(depth.shape),))
    N, H, W = (int(v) for v in depth.shape)
    intrinsics = _views("intrinsics", intrinsics, N, (3, 3), dev, "depth_consistency")
    c2ws = _views("c2ws", c2ws, N, (4, 4), dev, "depth_consistency")
    w2cs = None if w2cs is None else _views("w2cs", w2cs, N, (4, 4), dev, "depth_consistency")
    conf = None if conf is None else _views("conf", conf, N, (H, W), dev, "depth_consistency")
    if not (torch.is_tensor(src_ids) and src_ids.is_cuda and src_ids.device == dev and src_ids.dim() == 2 and src_ids.shape[0] == N):
        raise RuntimeError("uc_nerf_amd.depth_consistency: src_ids must be an int32 [%d,S] tensor on %s" % (N, dev))
    src_ids = _dev_as(src_ids, "src_ids", torch.int32)
    out = torch.empty(2 * N * H * W, dtype=torch.uint8, device=dev)
    count, mask = out[:N * H * W].view(N, H, W), out[N * H * W:].view(N, H, W)
    fused = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    p = L.DepthConsistencyParams()
    p.N, p.H, p.W, p.S, p.min_views = N, H, W, int(src_ids.shape[1]), int(min_views)
    p.pix_thresh, p.rel_thresh, p.conf_thresh = float(pix_thresh), float(rel_thresh), float(conf_thresh)
    p.depth, p.intrinsics, p.c2ws, p.w2cs, p.src_ids, p.conf = _ptr(depth), _ptr(intrinsics), _ptr(c2ws), _ptr(w2cs), _ptr(src_ids), _ptr(conf)
    p.count, p.mask, p.fused = _ptr(count), _ptr(mask), _ptr(fused)
    _launch("ucnerf_depth_consistency", p, dev)
    return mask.view(torch.bool), fused, count


def points_compact(fused, mask, rgb, intrinsics, c2ws, cap=None):
    """The masked pixels as a coloured point cloud: ucnerf_points_compact on the current stream (three kernels: workgroup counts, an exclusive
    scan in a fixed order, the scatter; no atomics), nothing synchronised or read back.  fused [N,H,W] float32; mask [N,H,W] bool (or uint8:
    non-zero = kept); rgb [N,3,H,W] float32; intrinsics [N,3,3] with zero skew; c2ws [N,4,4]; cap: rows to allocate, default N H W.
    -> (points float32 [cap,3] world, colors uint8 [cap,3] = (uint8)(clamp(c, 0, 1) * 255 + 0.5) with NaN -> 0, total int64 [1] on the device).
    Row k is the k-th masked pixel in (view, y, x) order.  `total` is the full number of masked pixels even when cap is smaller; only
    min(total, cap) rows are written, the others are left as allocated (uninitialised)."""
    dev = _dev(fused)
    fused = _f32(fused, "fused")
    if fused.dim() != 3:
        raise RuntimeError("uc_nerf_amd.points_compact: fused must be [N,H,W], got %s" % (tuple(fused.shape),))
    N, H, W = (int(v) for v in fused.shape)
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.device == dev and mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) == (N, H, W)):
        raise RuntimeError("uc_nerf_amd.points_compact: mask must be a bool or uint8 [%d,%d,%d] tensor on %s" % (N, H, W, dev))
    mask = mask.contiguous()
    rgb = _views("rgb", rgb, N, (3, H, W), dev, "points_compact")
    intrinsics = _views("intrinsics", intrinsics, N, (3, 3), dev, "points_compact")
    c2ws = _views("c2ws", c2ws, N, (4, 4), dev, "points_compact")
    n = N * H * W
    cap = n if cap is None else int(cap)
    rows = max(cap, 0)                                          # (a cap the library refuses allocates nothing: its check raises first)
    points = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((rows, 3), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws_bytes = L.lib().ucnerf_points_compact_workspace_bytes(n)
    L.check(min(ws_bytes, 0), "ucnerf_points_compact_workspace_bytes")
    workspace = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    p = L.PointsCompactParams()
    p.N, p.H, p.W, p.cap = N, H, W, cap
    p.fused, p.mask, p.rgb, p.intrinsics, p.c2ws = _ptr(fused), _ptr(mask), _ptr(rgb), _ptr(intrinsics), _ptr(c2ws)
    p.workspace, p.points, p.colors, p.total = _ptr(workspace), _ptr(points), _ptr(colors), _ptr(total)
    _launch("ucnerf_points_compact", p, dev)
    return points, colors, total
