"""The input side on the device: one sample of the reference's dataset assembled from a resident scene in one launch, Pillow's BILINEAR
resize of the decoded colour frames (bit for bit) that fills such a scene from frames at their native size, and the training step's three
target gathers out of such a sample's maps in one launch."""
import ctypes as C

import torch

from .. import _lib as L
from ._core import _cur_dev, _dev, _launch, _ptr

SAMPLE_MAX_ROWS = 1024      # the reference's rays_depth[:1024]
SAMPLE_MAX_VIEWS = 9        # the MLP's view_num range
RESIZE_MAX_RATIO = 16       # UCNERF_RESIZE_MAX_RATIO: in <= 16 * out on each axis (a workgroup's tile has to fit in LDS)

_RESIDENT = ("frames", "depth_img", "weight_img", "row1", "col1", "row2", "col2", "kp_depth", "kp_weight", "kp_coord",
             "c2w", "w2c", "intrinsic", "affine", "affine_inv", "ref_proj_inv")
_RESIDENT_DTYPES = {"frames": torch.uint8, "row1": torch.int32, "col1": torch.int32, "row2": torch.int32, "col2": torch.int32, "kp_coord": torch.int32}


def _sample_params(res):
    """The parameter struct of a resident scene, filled once with everything that does not change between samples (kept on `res`)."""
    p = getattr(res, "_sample_params", None)
    if p is not None:
        return p
    dev = res.frames.device
    if dev.type != "cuda":
        raise RuntimeError("uc_nerf_amd.sample_assemble: the scene must be resident on a ROCm device, it is on %s (there is no host route)" % dev)
    for name in _RESIDENT:
        t = getattr(res, name)
        want = _RESIDENT_DTYPES.get(name, torch.float32)
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == want and t.is_contiguous()):
            raise RuntimeError("uc_nerf_amd.sample_assemble: resident array %s must be a contiguous %s tensor on %s" % (name, want, dev))
    N, H, W = int(res.N), int(res.H), int(res.W)
    if res.frames.dim() != 2 or res.frames.shape[0] != N or res.depth_img.shape != (N, H, W) or res.weight_img.shape != (N, H, W):
        raise RuntimeError("uc_nerf_amd.sample_assemble: frames must be [N, frame_stride] bytes and the maps [N,H,W]")
    for name, per in (("c2w", 16), ("w2c", 16), ("intrinsic", 9), ("affine", 48), ("affine_inv", 48), ("ref_proj_inv", 16)):
        if getattr(res, name).numel() != N * per:
            raise RuntimeError("uc_nerf_amd.sample_assemble: %s must hold %d floats per frame" % (name, per))
    K = res.kp_depth.numel()
    if res.kp_weight.numel() != K or res.kp_coord.numel() != 2 * K or len(res.offsets) != N + 1 or res.offsets[-1] != K:
        raise RuntimeError("uc_nerf_amd.sample_assemble: the keypoint lists and their offsets disagree")
    p = L.SampleAssembleParams()
    p.N, p.H, p.W, p.frame_stride, p.kp_total = N, H, W, res.frames.shape[1], K
    p.h1, p.w1, p.h2, p.w2 = res.row1.numel(), res.col1.numel(), res.row2.numel(), res.col2.numel()
    for k in range(3):
        p.mean[k], p.std[k], p.unpre_mean[k], p.unpre_std[k] = res.mean[k], res.std[k], res.unpre_mean[k], res.unpre_std[k]
    p.near_far[0], p.near_far[1] = res.near_far
    for name in _RESIDENT:
        setattr(p, name, _ptr(getattr(res, name)))
    res._sample_params = p
    return p


def _carve(sizes):
    """Offsets (in floats, each a multiple of 4: 16-byte aligned planes, an 8-byte aligned int64 run) of consecutive segments, and the total."""
    at, offs = 0, []
    for n in sizes:
        offs.append(at)
        at += (n + 3) // 4 * 4
    return offs, at


def sample_assemble(res, view_ids, perm, n_rows, unpreprocess=False):
    """One sample out of a resident scene (`uc_nerf_amd.data.DeviceScene` holds one): ucnerf_sample_assemble, one launch on the current stream,
    nothing synchronised or read back.  `res` carries the resident device tensors (frames [N, frame_stride] uint8, depth_img / weight_img [N,H,W],
    the four int32 index maps, the concatenated keypoint lists with their host `offsets`, the per-frame matrices) and the host constants
    (mean, std, unpre_mean, unpre_std, near_far).  view_ids: Python ints, the target first.  perm: int32 device tensor of at least `n_rows`
    distinct indices below the target's keypoint count (not read when n_rows == 0; may then be None).
    Returns a dict of float32 device tensors with the batch-of-one shapes of the reference's DataLoader: images [1,V,3,H,W] (and images_unpre),
    sd1 / wt1 [1,h1,w1], sd2 / wt2 [1,h2,w2], rays_depth [1,n_rows,3,3], c2ws / w2cs [1,V,4,4], intrinsics [1,V,3,3], affine_mat / affine_mat_inv
    [1,V,3,4,4], proj_mats [1,V,3,4], near_fars [1,1,V,2], view_ids [1,V] int64.  All of them are views of one allocation."""
    p = _sample_params(res)
    dev = res.frames.device
    V = len(view_ids)
    if not 1 <= V <= SAMPLE_MAX_VIEWS:
        raise RuntimeError("uc_nerf_amd.sample_assemble: %d views, expected 1..%d" % (V, SAMPLE_MAX_VIEWS))
    n_rows = int(n_rows)
    if n_rows > 0:
        if not (torch.is_tensor(perm) and perm.device == dev and perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() >= n_rows):
            raise RuntimeError("uc_nerf_amd.sample_assemble: perm must be a contiguous int32 tensor of at least %d indices on %s" % (n_rows, dev))
    H, W, HW = p.H, p.W, p.H * p.W
    n1, n2 = p.h1 * p.w1, p.h2 * p.w2
    img = V * 3 * HW
    sizes = [img, img if unpreprocess else 0, n1, n2, n1, n2, n_rows * 9, V * 16, V * 16, V * 9, V * 48, V * 48, V * 12, V * 2, V * 2]
    offs, total = _carve(sizes)
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    seg = [buf[o:o + n] for o, n in zip(offs, sizes)]
    target = int(view_ids[0])
    p.V, p.n_rows = V, n_rows
    for v in range(SAMPLE_MAX_VIEWS):
        p.view_ids[v] = int(view_ids[v]) if v < V else 0
    if 0 <= target < p.N:                                        # (anything else is refused by the library's own check, with its message)
        p.kp_first, p.n_kp = int(res.offsets[target]), int(res.offsets[target + 1] - res.offsets[target])
    else:
        p.kp_first, p.n_kp = 0, 0
    p.perm = _ptr(perm) if n_rows > 0 else 0
    base = buf.data_ptr()
    (p.images, p.images_unpre, p.sd1, p.sd2, p.wt1, p.wt2, p.rays_depth, p.c2ws, p.w2cs, p.intrinsics, p.affine_mat, p.affine_mat_inv, p.proj_mats,
     p.near_fars, p.view_ids_out) = [base + 4 * o if n else 0 for o, n in zip(offs, sizes)]
    _launch("ucnerf_sample_assemble", p, dev)
    out = dict(images=seg[0].view(1, V, 3, H, W), sd1=seg[2].view(1, p.h1, p.w1), sd2=seg[3].view(1, p.h2, p.w2), wt1=seg[4].view(1, p.h1, p.w1),
               wt2=seg[5].view(1, p.h2, p.w2), rays_depth=seg[6].view(1, n_rows, 3, 3), c2ws=seg[7].view(1, V, 4, 4), w2cs=seg[8].view(1, V, 4, 4),
               intrinsics=seg[9].view(1, V, 3, 3), affine_mat=seg[10].view(1, V, 3, 4, 4), affine_mat_inv=seg[11].view(1, V, 3, 4, 4),
               proj_mats=seg[12].view(1, V, 3, 4), near_fars=seg[13].view(1, 1, V, 2), view_ids=seg[14].view(torch.int64).view(1, V))
    if unpreprocess:
        out["images_unpre"] = seg[1].view(1, V, 3, H, W)
    return out


NOVEL_MAX_CAND = 4096       # candidates of one novel_assemble call (every workgroup of a source slot ranks them all)
_NOVEL_RESIDENT = ("frames", "c2w", "w2c", "intrinsic", "affine", "affine_inv")


def _novel_params(res):
    """The parameter struct of `novel_assemble` for a resident scene, filled once with what does not change between poses (kept on `res`)."""
    p = getattr(res, "_novel_params", None)
    if p is not None:
        return p
    s = _sample_params(res)                                       # (its checks are this struct's checks: device, dtypes, shapes)
    p = L.NovelAssembleParams()
    p.N, p.H, p.W, p.frame_stride = s.N, s.H, s.W, s.frame_stride
    for k in range(3):
        p.mean[k], p.std[k], p.unpre_mean[k], p.unpre_std[k] = s.mean[k], s.std[k], s.unpre_mean[k], s.unpre_std[k]
    p.near_far[0], p.near_far[1] = s.near_far[0], s.near_far[1]
    for name in _NOVEL_RESIDENT:
        setattr(p, name, _ptr(getattr(res, name)))
    res._novel_params = p
    return p


def novel_assemble(res, poses, index, cand, V, intrinsic=None, unpreprocess=False):
    """The batch of a FREE camera pose out of a resident scene (`uc_nerf_amd.data.DeviceScene.sample_pose` calls this): ucnerf_novel_assemble, one
    launch on the current stream, nothing synchronised or read back.  `res` as for `sample_assemble`.  poses: contiguous float32 device tensor
    [P,3,4], camera-to-world [R | t]; index: Python int, the pose of this call; cand: contiguous int32 device tensor [n_cand], V <= n_cand <=
    NOVEL_MAX_CAND, the frames that may serve as sources (an entry outside 0..N-1 is clamped into that range on the device); V: views of the
    batch, 2..SAMPLE_MAX_VIEWS -- the pose itself and its V - 1 nearest candidates (squared distance of the camera centres in float32, ascending,
    ties to the lower position in `cand`, NaN last); intrinsic: contiguous float32 device tensor [3,3] with ZERO SKEW, default frame 0's.
    Slot 0 carries the pose's matrices in closed form: w2cs[0] is the rigid inverse [R^T | -R^T t], affine_mat_inv[0] is c2w . diag(K_s^-1, 1)
    -- neither is an LU inverse; a rotation block that is not orthonormal gives what the formulas give (include/ucnerf_hip.h has the fmaf orders).
    Slots 1..V-1 are the selected frames as `sample_assemble` gives them, bit for bit, except proj_mats[v] = (affine[v][2] @ affine_mat_inv[0][2])[:3].
    Returns a dict of device tensors, views of one allocation: images [1,V,3,H,W] (slot 0 all 0.0: a free pose has no ground truth; with
    unpreprocess also images_unpre), c2ws / w2cs [1,V,4,4], intrinsics [1,V,3,3], affine_mat / affine_mat_inv [1,V,3,4,4], proj_mats [1,V,3,4],
    near_fars [1,1,V,2], view_ids [1,V] int64 = (-1, selected frame ids)."""
    p = _novel_params(res)
    dev = res.frames.device
    V, index = int(V), int(index)
    if not (torch.is_tensor(poses) and poses.device == dev and poses.dtype == torch.float32 and poses.is_contiguous() and poses.dim() == 3
            and tuple(poses.shape[1:]) == (3, 4)):
        raise RuntimeError("uc_nerf_amd.novel_assemble: poses must be a contiguous float32 [P,3,4] tensor on %s" % dev)
    if not (torch.is_tensor(cand) and cand.device == dev and cand.dtype == torch.int32 and cand.is_contiguous() and cand.dim() == 1):
        raise RuntimeError("uc_nerf_amd.novel_assemble: cand must be a contiguous int32 [n_cand] tensor on %s" % dev)
    if intrinsic is not None and not (torch.is_tensor(intrinsic) and intrinsic.device == dev and intrinsic.dtype == torch.float32
                                      and intrinsic.is_contiguous() and tuple(intrinsic.shape) == (3, 3)):
        raise RuntimeError("uc_nerf_amd.novel_assemble: intrinsic must be a contiguous float32 [3,3] tensor on %s" % dev)
    H, W, HW = p.H, p.W, p.H * p.W
    Va = min(max(V, 0), SAMPLE_MAX_VIEWS)                         # (a V the library refuses allocates nothing that matters: its check raises first)
    img = Va * 3 * HW
    sizes = [img, img if unpreprocess else 0, Va * 16, Va * 16, Va * 9, Va * 48, Va * 48, Va * 12, Va * 2, Va * 2]
    offs, total = _carve(sizes)
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    seg = [buf[o:o + n] for o, n in zip(offs, sizes)]
    p.V, p.P, p.pose_index, p.n_cand = V, int(poses.shape[0]), index, int(cand.numel())
    p.poses, p.cand, p.intrinsic_in = _ptr(poses), _ptr(cand), (_ptr(intrinsic) if intrinsic is not None else 0)
    base = buf.data_ptr()
    (p.images, p.images_unpre, p.c2ws, p.w2cs, p.intrinsics, p.affine_mat, p.affine_mat_inv, p.proj_mats, p.near_fars,
     p.view_ids_out) = [base + 4 * o if n else 0 for o, n in zip(offs, sizes)]
    _launch("ucnerf_novel_assemble", p, dev)
    out = dict(images=seg[0].view(1, V, 3, H, W), c2ws=seg[2].view(1, V, 4, 4), w2cs=seg[3].view(1, V, 4, 4), intrinsics=seg[4].view(1, V, 3, 3),
               affine_mat=seg[5].view(1, V, 3, 4, 4), affine_mat_inv=seg[6].view(1, V, 3, 4, 4), proj_mats=seg[7].view(1, V, 3, 4),
               near_fars=seg[8].view(1, 1, V, 2), view_ids=seg[9].view(torch.int64).view(1, V))
    if unpreprocess:
        out["images_unpre"] = seg[1].view(1, V, 3, H, W)
    return out


def resize_coeffs(in_size, out_size):
    """Pillow's BILINEAR coefficient table of one axis (`in_size` -> `out_size` pixels) from ucnerf_resize_bilinear_coeffs: host arithmetic in
    double, no device.  Returns int32 CPU tensors (start [out], count [out], k [out, ksize]): output pixel xx is
    clip8((2^21 + sum_x in[start[xx] + x] * k[xx, x]) >> 22) over x < count[xx]; k[xx, count[xx]:] is 0."""
    in_size, out_size = int(in_size), int(out_size)
    lib = L.lib()
    ksize = lib.ucnerf_resize_bilinear_ksize(in_size, out_size)
    L.check(min(ksize, 0), "ucnerf_resize_bilinear_ksize")
    start, count = torch.empty(out_size, dtype=torch.int32), torch.empty(out_size, dtype=torch.int32)
    k = torch.empty((out_size, ksize), dtype=torch.int32)
    rc = lib.ucnerf_resize_bilinear_coeffs(in_size, out_size, C.c_void_p(start.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(k.data_ptr()))
    L.check(min(rc, 0), "ucnerf_resize_bilinear_coeffs")
    return start, count, k


_resize_tables = {}      # (in, out, device) -> the three tables on that device


def _device_coeffs(in_size, out_size, dev):
    key = (in_size, out_size, str(dev))
    t = _resize_tables.get(key)
    if t is None:
        t = _resize_tables[key] = tuple(a.to(dev) for a in resize_coeffs(in_size, out_size))
    return t


def resize_bilinear_u8(src, out_wh, out=None, out_frame_stride=None):
    """`PIL.Image.fromarray(frame).resize(out_wh, PIL.Image.BILINEAR)` of every frame of `src`, bit for bit (Pillow 12.2.0's), in one launch on the
    current stream: ucnerf_resize_bilinear_u8.  src: contiguous uint8 device tensor [N,Hin,Win,3]; out_wh = (W, H).  Returns a contiguous uint8
    [N,H,W,3].  With `out` (a contiguous uint8 device tensor of N frames, `out_frame_stride` bytes apart -- default: out.shape[1] of a [N, stride]
    tensor; a multiple of 4 and at least 3 H W, as DeviceScene's padded storage is) the frames are written there, the bytes between 3 H W and the
    stride are left as they are, and `out` is returned.  The device coefficient tables are cached per (in, out, device).  Each axis may shrink by at
    most RESIZE_MAX_RATIO; nothing is synchronised or read back."""
    dev = _dev(src)
    if src.dtype != torch.uint8:
        raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: src must be uint8, got %s" % src.dtype)
    if src.dim() != 4 or src.shape[3] != 3:
        raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: src must be [N,Hin,Win,3], got %s" % (tuple(src.shape),))
    if not src.is_contiguous():
        raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: src must be contiguous")
    N, Hin, Win = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    W, H = int(out_wh[0]), int(out_wh[1])
    if W < 1 or H < 1 or Hin < 1 or Win < 1:
        raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: %d x %d -> %d x %d (a size below 1)" % (Hin, Win, H, W))
    frame = 3 * H * W
    packed = None
    if out is None:
        stride = (frame + 3) // 4 * 4
        buf = torch.empty((N, stride), dtype=torch.uint8, device=dev)
        packed = buf if stride == frame else None
        dst = buf
    else:
        if not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.uint8 and out.is_contiguous()):
            raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: out must be a contiguous uint8 tensor on %s" % dev)
        if out_frame_stride is None:
            if out.dim() != 2 or out.shape[0] != N:
                raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: out must be [%d, frame_stride] bytes (or give out_frame_stride), got %s"
                                   % (N, tuple(out.shape)))
            out_frame_stride = out.shape[1]
        stride = int(out_frame_stride)
        if N and out.numel() < (N - 1) * stride + frame:
            raise RuntimeError("uc_nerf_amd.resize_bilinear_u8: out holds %d bytes, %d frames of stride %d need %d"
                               % (out.numel(), N, stride, (N - 1) * stride + frame))
        dst = out
    p = L.ResizeParams()
    p.N, p.Hin, p.Win, p.H, p.W = N, Hin, Win, H, W
    p.src_frame_stride, p.dst_frame_stride = 3 * Hin * Win, stride
    if N:
        sx, cx, kx = _device_coeffs(Win, W, dev)
        sy, cy, ky = _device_coeffs(Hin, H, dev)
        p.ksize_x, p.ksize_y = kx.shape[1], ky.shape[1]
        p.src, p.dst = _ptr(src), _ptr(dst)
        p.start_x, p.count_x, p.k_x, p.start_y, p.count_y, p.k_y = _ptr(sx), _ptr(cx), _ptr(kx), _ptr(sy), _ptr(cy), _ptr(ky)
    _launch("ucnerf_resize_bilinear_u8", p, dev)
    if out is not None:
        return out
    if packed is not None:
        return packed.view(N, H, W, 3)
    return dst[:, :frame].contiguous().view(N, H, W, 3)        # (3 H W is no multiple of 4: one device copy out of the padded rows)


# one sticky status word per device (bit 0: a depth ray, bit 1: a patch ray of some step_targets call had a coordinate outside the image),
# allocated once and kept for the life of the process
_target_words = {}


def _target_word(device=None):
    idx = _cur_dev() if device is None or torch.device(device).index is None else torch.device(device).index
    w = _target_words.get(idx)
    if w is None:
        w = _target_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return w


def step_targets_status(clear=False, device=None):
    """The status word of `step_targets` on `device` (default: the current one) as an int: bit 0 set = a depth ray, bit 1 set = a patch ray of
    some call since the last clear had a coordinate outside the image (its element was NaN).  SYNCHRONISES (reads the word back); clear=True
    also zeroes it afterwards."""
    w = _target_word(device)
    v = int(w.item())
    if clear:
        w.zero_()
    return v


def step_targets_status_clear(device=None):
    """Enqueues a clear of the status word on the current stream (no synchronisation)."""
    _target_word(device).zero_()


def _target_map(t, name, H, W, dev):
    if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (1, H, W)):
        raise RuntimeError("uc_nerf_amd.step_targets: %s must be a contiguous float32 [1,%d,%d] tensor on %s (it is read in place)" % (name, H, W, dev))
    return t


def step_targets(sparse_depths, sparse_weights, dpt, pixel_coordinates, n_rays, patch_num, patch_size, status=None):
    """The training step's three target gathers (train.py:166-176) in ONE launch on the current stream (ucnerf_step_targets), nothing
    synchronised or read back, no autograd (the outputs are data):
        target_depths  = sparse_depths[:, r[n_rays:], c[n_rays:]]        [1, n_total - n_rays]
        target_weights = sparse_weights[:, r[n_rays:], c[n_rays:]]       [1, n_total - n_rays]
        patch_dpt      = dpt[:, r[:P], c[:P]].reshape(-1, ps, ps, 1)     [patch_num, ps, ps, 1],  P = patch_num * ps * ps
    with (r, c) = pixel_coordinates [2, n_total], int64 or float32 holding whole numbers (`build_rays`'s, as it returns them: no .long()).
    The maps are contiguous float32 [1,H,W] device tensors and are read in place (`DeviceScene.sample`'s views are).  Indexing is torch's: a
    row in [-H, H) or a column in [-W, W) wraps; the values are copied bit for bit.  A coordinate outside that range, or a float that is no
    whole number, gives NaN in its element and sets a bit of `status` (a one-element int32 device tensor; default: the device's own word, see
    `step_targets_status`): bit 0 for a depth ray, bit 1 for a patch ray -- torch raises a device-side assert there.  n_total == n_rays and
    patch_num == 0 give empty tensors; with both nothing is launched."""
    dev = _dev(sparse_depths)
    if sparse_depths.dim() != 3:
        raise RuntimeError("uc_nerf_amd.step_targets: sparse_depths must be [1,H,W], got %s" % (tuple(sparse_depths.shape),))
    H, W = int(sparse_depths.shape[1]), int(sparse_depths.shape[2])
    for t, name in ((sparse_depths, "sparse_depths"), (sparse_weights, "sparse_weights"), (dpt, "dpt")):
        _target_map(t, name, H, W, dev)
    pix = pixel_coordinates
    if not (torch.is_tensor(pix) and pix.device == dev and pix.dim() == 2 and pix.shape[0] == 2 and pix.dtype in (torch.int64, torch.float32)):
        raise RuntimeError("uc_nerf_amd.step_targets: pixel_coordinates must be an int64 or float32 [2, n_total] tensor on %s" % dev)
    pix = pix.contiguous()
    n_total, n_rays, patch_num, ps = int(pix.shape[1]), int(n_rays), int(patch_num), int(patch_size)
    if status is None:
        status = _target_word(dev)
    elif not (torch.is_tensor(status) and status.is_cuda and status.dtype == torch.int32 and status.numel() == 1 and status.device == dev):
        raise RuntimeError("uc_nerf_amd.step_targets: status must be a one-element int32 tensor on the maps' device")
    p = L.StepTargetsParams()
    p.H, p.W, p.n_total, p.n_rays, p.patch_num, p.patch_size = H, W, n_total, n_rays, patch_num, ps
    p.coord_is_float = int(pix.dtype == torch.float32)
    n_depth, n_patch = max(n_total - n_rays, 0), max(patch_num, 0) * max(ps, 0) ** 2
    # (sizes the library refuses allocate nothing that matters: its check raises before anything is launched)
    out = torch.empty(2 * n_depth + min(n_patch, n_total), device=dev)
    t_depths, t_weights, patch = out[:n_depth], out[n_depth:2 * n_depth], out[2 * n_depth:]
    p.sparse_depths, p.sparse_weights, p.dpt, p.pixel_coordinates = _ptr(sparse_depths), _ptr(sparse_weights), _ptr(dpt), _ptr(pix)
    p.target_depths, p.target_weights, p.patch_dpt, p.status = _ptr(t_depths), _ptr(t_weights), _ptr(patch), _ptr(status)
    _launch("ucnerf_step_targets", p, dev)
    return t_depths.view(1, n_depth), t_weights.view(1, n_depth), patch.view(patch_num, ps, ps, 1)
