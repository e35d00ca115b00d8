"""From per-view maps to geometry: the fusion step of the MVSNet / CasMVSNet family on the device.

Every pixel's depth is re-projected into its neighbouring views, kept only where enough of them agree, averaged with the agreeing depths and
back-projected to a coloured world-space point (`ops.depth_consistency`, `ops.points_compact`: one gather-bound launch and a deterministic
compaction; the maps never leave the device).  The rules -- bilinear sampling that refuses invalid taps, the closed image rectangle
[0, W-1] x [0, H-1] -- are this project's own: no third-party fusion script is reproduced.

    out = system.render_path(scene, path)                                      # {'rgb': [P,3,H,W], 'depth': [P,H,W]}
    cloud = fuse_views(out["depth"], out["rgb"], K.expand(P, 3, 3), poses_4x4)
    cloud.save_ply("scene.ply")                                                # the one host read
"""
import numpy as np
import torch

from . import ops
from .data import formats


def source_table(c2ws, n_src):
    """Host function: int32 [N, n_src], row r = the n_src views nearest to view r by `formats.get_nearest_pose_ids`'s criterion (distance of
    the camera centres, r itself excluded), nearest first; -1 where fewer than n_src other views exist.  c2ws: [N,3,4] or [N,4,4], a numpy array
    or a tensor (a device tensor is copied to the host: one blocking read)."""
    c2ws = c2ws.detach().cpu().numpy() if torch.is_tensor(c2ws) else np.asarray(c2ws)
    N, n_src = len(c2ws), int(n_src)
    if c2ws.ndim != 3 or c2ws.shape[1] < 3 or c2ws.shape[2] != 4 or n_src < 0:
        raise ValueError("source_table: c2ws must be [N,3,4] or [N,4,4] and n_src >= 0, got %s, %d" % (c2ws.shape, n_src))
    table = np.full((N, n_src), -1, dtype=np.int32)
    for r in range(N):
        ids = formats.get_nearest_pose_ids(c2ws[r], c2ws, n_src, tar_id=r) if N > 1 else []
        ids = [int(i) for i in ids if int(i) != r]
        table[r, :len(ids)] = ids
    return table


class PointCloud:
    """A fused cloud on the device: points float32 [cap,3] (world), colors uint8 [cap,3], total int64 [1] -- the number of valid rows, known only
    on the device until `trim()` reads it (the one host read; its value is kept)."""

    def __init__(self, points, colors, total):
        self.points, self.colors, self.total = points, colors, total
        self._n = None

    def trim(self):
        """-> (points [n,3], colors [n,3]): the valid rows, n = min(total, cap), as views.  Reads `total` back (synchronises) on the first call."""
        if self._n is None:
            self._n = min(int(self.total.item()), int(self.points.shape[0]))
        return self.points[:self._n], self.colors[:self._n]

    def save_ply(self, path):
        """Writes the valid rows with `formats.write_ply` (binary little-endian, float x y z, uchar red green blue).  -> the number of points."""
        points, colors = self.trim()
        formats.write_ply(path, points.cpu().numpy(), colors.cpu().numpy())
        return int(points.shape[0])


def fuse_views(depth, rgb, intrinsics, c2ws, src_ids=None, n_src=4, w2cs=None, conf=None, cap=None, **thresholds):
    """depth [N,H,W], rgb [N,3,H,W] in [0, 1], intrinsics [N,3,3] (zero skew), c2ws [N,4,4]: float32 device tensors, as `UCNeRFSystem.render_path`
    and `render_validation_image` leave them.  src_ids: int32 [N,S] device tensor (or a host array, uploaded), default `source_table(c2ws, n_src)`
    -- that default reads c2ws back to the host once; pass src_ids to stay on the device.  w2cs / conf / cap: `ops.depth_consistency`'s and
    `ops.points_compact`'s.  **thresholds: pix_thresh, rel_thresh, conf_thresh, min_views.  -> PointCloud; nothing else is read back."""
    bad = set(thresholds) - {"pix_thresh", "rel_thresh", "conf_thresh", "min_views"}
    if bad:
        raise TypeError("fuse_views: unknown arguments %s" % sorted(bad))
    if src_ids is None:
        src_ids = source_table(c2ws, n_src)
    if not torch.is_tensor(src_ids):
        src_ids = torch.from_numpy(np.ascontiguousarray(np.asarray(src_ids), dtype=np.int32))
    src_ids = src_ids.to(depth.device)
    mask, fused, _ = ops.depth_consistency(depth, intrinsics, c2ws, src_ids, w2cs=w2cs, conf=conf, **thresholds)
    return PointCloud(*ops.points_compact(fused, mask, rgb, intrinsics, c2ws, cap=cap))
