"""A scene resident on the device, and the reference's training / validation sample assembled from it in one launch.

The reference's `ScaredDataset.__getitem__` (data/scared.py:387-522) builds every sample on the host: V images through PIL, ToTensor and
Normalize, four cv2 resizes of the sparse maps, 3 V projection matrices and their inverses, a shuffled keypoint list; the DataLoader collates it
at batch_size=1 and copies it to the device.  Almost all of that is constant per FRAME.  `DeviceScene` computes the per-frame part once, on the
host, with the reference's own calls (so the bits agree), uploads it once, and leaves one launch per sample (`ops.sample_assemble`).

The colour frames' resize to `img_wh` is built as well: `DeviceScene.from_native` takes the decoded frames at their native size and runs the
reference's `PIL.Image.resize(img_wh, PIL.Image.BILINEAR)` on the device, with Pillow's bits (`ops.resize_bilinear_u8`; compared byte for byte
with Pillow 12.2.0).  Still the caller's job: decoding the files (JPEG / PNG / .npz), and the two cv2 resizes of the float maps (`dpt`,
`depths_h`), which cannot be verified without OpenCV: those two arrive at `img_wh`.

Two documented differences from the reference's sample:
  * every floating tensor is float32 (numpy's `np.zeros` maps come through the reference's collation as float64);
  * `proj_mats` is a fixed-order float32 product formed on the device (fmaf over k = 0..3 from a first product, include/ucnerf_hip.h) instead
    of `torch.matmul`'s.
`rays_depth` is [1,n,3,3]: the reference's comment says N x 4 x 3, its concatenate of depth, weight and (h, w, 1) rows makes three rows, and
train.py:127-131 reads rows 0..2.
"""
import numpy as np
import torch

from . import formats

MEAN = (0.485, 0.456, 0.406)        # data/scared.py:381
STD = (0.229, 0.224, 0.225)
MAX_ROWS = 1024                     # data/scared.py:503


def pyramid_index(size, k):
    """Source index of every row (column) of a nearest-neighbour level of `size // k` rows (columns), formed in double as cv2's INTER_NEAREST
    does: min(floor(dst * (size / (size // k))), size - 1).  int32 [size // k].  Not verified against OpenCV (cv2 is not a dependency; OpenCV
    forms the scale as 1 / (dst_size / size), which may differ from size / dst_size in the last bit where the ratio is inexact)."""
    d = size // k
    if d == 0:
        return np.zeros(0, np.int32)
    return np.minimum(np.floor(np.arange(d, dtype=np.float64) * (size / d)), size - 1).astype(np.int32)


def normalise_weights(w):
    """The reference's `w -= w.min(); w /= w.max()` in float64 (data/scared.py:407-408, :434-435) on a copy.  Idempotent, so doing it once is
    what the reference's repeated in-place application leaves.  Weights that are all equal give 0 / 0 = NaN there; that is kept: no exception,
    no warning, NaN out.  An empty array comes back empty (the reference raises on a frame without keypoints)."""
    w = np.array(w, dtype=np.float64)
    if w.size == 0:
        return w
    with np.errstate(invalid="ignore", divide="ignore"):
        w -= w.min()
        w /= w.max()
    return w


def frame_matrices(pose, focal, img_wh):
    """One frame's matrices with the calls of data/scared.py:455-484: float32 torch tensors, torch.inverse for w2c and ref_proj_inv,
    np.linalg.inv on the float32 stage matrices.  Returns float32 arrays c2w, w2c [4,4], intrinsic [3,3], affine, affine_inv [3,4,4],
    ref_proj_inv [4,4]."""
    c2w = torch.eye(4).float()
    c2w[:3] = torch.FloatTensor(np.asarray(pose))
    w2c = torch.inverse(c2w)
    intrinsic = torch.tensor([[focal[0], 0, img_wh[0] / 2], [0, focal[1], img_wh[1] / 2], [0, 0, 1]]).float()
    aff, aff_inv = [], []
    for scale in range(3):
        proj_mat_l = torch.eye(4)
        stage_intrinsic = intrinsic.clone()
        stage_intrinsic[:2] = intrinsic[:2] / (2 ** (2 - scale))
        proj_mat_l[:3, :4] = stage_intrinsic @ w2c[:3, :4]
        aff.append(proj_mat_l.numpy())
        aff_inv.append(np.linalg.inv(proj_mat_l.numpy()))
    aff, aff_inv = np.stack(aff), np.stack(aff_inv)
    ref_proj_inv = torch.inverse(torch.tensor(aff[2]))
    return c2w.numpy(), w2c.numpy(), intrinsic.numpy(), aff, aff_inv, ref_proj_inv.numpy()


def scene_constants(poses, focal, bounds, sparse, img_wh):
    """Everything `DeviceScene` keeps per frame, as host numpy arrays (the host-side builder: no device needed).
    poses [N,3,4] float64, focal (fx, fy), bounds [N,2]: `formats.load_poses_bounds`'s; sparse: per frame a dict with 'depth' [n], 'coord' [n,2]
    = (h, w), 'weight' [n], 'depth_img', 'weight_img' [H,W] (`formats.colmap_sparse_depth`'s; a frame may hold no keypoint).  The caller's arrays
    are not modified."""
    W, H = int(img_wh[0]), int(img_wh[1])
    N = len(poses)
    if len(sparse) != N or len(bounds) != N:
        raise ValueError("scene_constants: %d poses, %d bounds, %d sparse-depth records" % (N, len(bounds), len(sparse)))
    mats = [frame_matrices(poses[i], focal, (W, H)) for i in range(N)]
    c = {name: np.ascontiguousarray(np.stack([m[k] for m in mats]), dtype=np.float32)
         for k, name in enumerate(("c2w", "w2c", "intrinsic", "affine", "affine_inv", "ref_proj_inv"))}
    bounds = np.asarray(bounds)
    c["near_far"] = np.array([bounds.min() * 0.9, bounds.max() * 1.1]).astype(np.float32)
    depth_img, weight_img, kd, kw, kc, offsets = [], [], [], [], [], [0]
    for i, s in enumerate(sparse):
        d_img, w_img = np.asarray(s["depth_img"]), np.asarray(s["weight_img"])
        if d_img.shape != (H, W) or w_img.shape != (H, W):
            raise ValueError("scene_constants: frame %d's maps are %s, expected %s" % (i, d_img.shape, (H, W)))
        depth_img.append(d_img.astype(np.float32))
        weight_img.append(normalise_weights(w_img).astype(np.float32))
        n = len(s["depth"])
        coord = np.asarray(s["coord"]).reshape(n, 2)
        if n and (coord.min() < 0 or coord[:, 0].max() >= H or coord[:, 1].max() >= W):
            raise ValueError("scene_constants: frame %d has a keypoint outside the %d x %d image" % (i, H, W))
        kd.append(np.asarray(s["depth"], dtype=np.float64).reshape(n).astype(np.float32))
        kw.append(normalise_weights(np.asarray(s["weight"]).reshape(n)).astype(np.float32))
        kc.append(coord.astype(np.int32))
        offsets.append(offsets[-1] + n)
    c["depth_img"], c["weight_img"] = np.stack(depth_img), np.stack(weight_img)
    c["kp_depth"], c["kp_weight"] = np.concatenate(kd), np.concatenate(kw)
    c["kp_coord"] = np.ascontiguousarray(np.concatenate(kc).reshape(-1, 2))
    c["offsets"] = np.array(offsets, dtype=np.int64)
    c["row1"], c["col1"], c["row2"], c["col2"] = pyramid_index(H, 4), pyramid_index(W, 4), pyramid_index(H, 2), pyramid_index(W, 2)
    return c


class DeviceScene:
    """One scene of the reference's dataset, resident on `device`; `sample()` is its `__getitem__` as one launch.

    Resident (uploaded once): the uint8 frames, the float32 depth / normalised weight maps, dpt and depths_h, the keypoint lists (CSR: `offsets`
    stays on the host as well), the per-frame matrices and the four pyramid index maps.  A frame whose weights are all equal carries NaN weights
    (0 / 0 in the reference's normalisation): that is kept, nothing is raised.  On device="cpu" the object only holds the constants
    (there is no host route for `sample()`)."""

    def __init__(self, consts, frames, dpt, depths_h=None, poses=None, device="cuda", scan=0, mean=MEAN, std=STD):
        device = torch.device(device)
        frames = np.asarray(frames)
        N, H, W = consts["depth_img"].shape
        if frames.dtype != np.uint8 or frames.shape != (N, H, W, 3):
            raise ValueError("DeviceScene: frames must be uint8 [%d,%d,%d,3], got %s %s" % (N, H, W, frames.dtype, frames.shape))
        self._init_resident(consts, dpt, depths_h, poses, device, scan, mean, std)
        # the bytes are read as dwords, four pixels to a thread: every frame starts on a dword
        stride = (3 * H * W + 3) // 4 * 4
        padded = np.zeros((N, stride), np.uint8)
        padded[:, :3 * H * W] = frames.reshape(N, -1)
        self.frames = torch.from_numpy(padded).to(device)

    def _init_resident(self, consts, dpt, depths_h, poses, device, scan, mean, std):
        """Everything resident but the frames."""
        N, H, W = consts["depth_img"].shape
        dpt = np.asarray(dpt, dtype=np.float32)
        depths_h = np.zeros((N, H, W), np.float32) if depths_h is None else np.asarray(depths_h, dtype=np.float32)
        if dpt.shape != (N, H, W) or depths_h.shape != (N, H, W):
            raise ValueError("DeviceScene: dpt and depths_h must be [%d,%d,%d]" % (N, H, W))
        self.N, self.H, self.W, self.device = N, H, W, device
        self.offsets = [int(o) for o in consts["offsets"]]
        self.poses = None if poses is None else np.asarray(poses)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)        # noqa: E731
        self.dpt, self.depths_h = up(dpt), up(depths_h)
        for name in ("depth_img", "weight_img", "kp_depth", "kp_weight", "kp_coord", "row1", "col1", "row2", "col2",
                     "c2w", "w2c", "intrinsic", "affine", "affine_inv", "ref_proj_inv"):
            setattr(self, name, up(consts[name]))
        self.near_far = (float(consts["near_far"][0]), float(consts["near_far"][1]))
        # Normalize's float32 mean / std; unpreprocess's constants as train.py:65-68 forms them: a double quotient rounded to float32
        self.mean, self.std = [float(np.float32(m)) for m in mean], [float(np.float32(s)) for s in std]
        self.unpre_mean = [float(np.float32(-m / s)) for m, s in zip(mean, std)]
        self.unpre_std = [float(np.float32(1 / s)) for s in std]
        self.scan = torch.tensor([int(scan)], device=device)

    @classmethod
    def from_arrays(cls, poses, focal, bounds, sparse, frames, dpt, depths_h=None, img_wh=None, device="cuda", scan=0):
        """poses [N,3,4], focal (fx, fy) and bounds [N,2] as `formats.load_poses_bounds` returns them; the rest as `from_records`."""
        frames = np.asarray(frames)
        if img_wh is None:
            img_wh = (frames.shape[2], frames.shape[1])
        return cls(scene_constants(poses, focal, bounds, sparse, img_wh), frames, dpt, depths_h, poses=poses, device=device, scan=scan)

    @classmethod
    def from_records(cls, record, sparse, frames, dpt, depths_h=None, img_wh=None, device="cuda", scan=0):
        """record: `formats.load_poses_bounds`'s; sparse: `formats.colmap_sparse_depth`'s per-frame list (image-name order); frames uint8
        [N,H,W,3] already at img_wh = (W, H); dpt float32 [N,H,W] already resized; depths_h float32 [N,H,W] or None (zeros)."""
        return cls.from_arrays(record["poses"], record["focal"], record["bounds"], sparse, frames, dpt, depths_h, img_wh, device, scan)

    @classmethod
    def from_native(cls, poses, focal, bounds, sparse, frames, dpt, depths_h=None, img_wh=None, batch=32, device="cuda", scan=0):
        """As `from_arrays`, from frames at their NATIVE size: `frames` is an iterable of decoded uint8 arrays [h, w, 3] (sizes may differ between
        frames), and every one goes through the reference's `PIL.Image.resize(img_wh, PIL.Image.BILINEAR)` on the device, bit for bit
        (`ops.resize_bilinear_u8`).  Consecutive frames of equal shape are uploaded and resized `batch` at a time, straight into the resident padded
        storage: no full-size copy of the scene is ever resident, on either side.  `img_wh` = (W, H) is required; `dpt` and `depths_h` are already
        at `img_wh`, as in `from_arrays`.  There is no host route: `device` must be a ROCm device.  `sample()` is the same code on the result."""
        from .. import ops
        if img_wh is None:
            raise ValueError("DeviceScene.from_native: img_wh = (W, H) is required (the frames come at their native size)")
        W, H = int(img_wh[0]), int(img_wh[1])
        if W < 1 or H < 1:
            raise ValueError("DeviceScene.from_native: img_wh = %r" % (tuple(img_wh),))
        batch = int(batch)
        if batch < 1:
            raise ValueError("DeviceScene.from_native: batch = %d, expected at least 1" % batch)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("DeviceScene.from_native: the resize runs on a ROCm device, got device=%s (there is no host route)" % device)
        self = cls.__new__(cls)
        self._init_resident(scene_constants(poses, focal, bounds, sparse, (W, H)), dpt, depths_h, poses, device, scan, MEAN, STD)
        N = self.N
        self.frames = torch.zeros((N, (3 * H * W + 3) // 4 * 4), dtype=torch.uint8, device=device)
        done, group = 0, []

        def flush():
            nonlocal done
            if group:
                src = torch.from_numpy(np.stack(group)).to(device)
                ops.resize_bilinear_u8(src, (W, H), out=self.frames[done:done + len(group)])
                done += len(group)
                del group[:]

        for i, fr in enumerate(frames):
            fr = np.asarray(fr)
            if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3 or fr.shape[0] < 1 or fr.shape[1] < 1:
                raise ValueError("DeviceScene.from_native: frame %d must be uint8 [h,w,3], got %s %s" % (i, fr.dtype, fr.shape))
            if i >= N:
                raise ValueError("DeviceScene.from_native: more than the %d frames the poses give" % N)
            if group and (len(group) == batch or group[0].shape != fr.shape):
                flush()
            group.append(fr)
        flush()
        if done != N:
            raise ValueError("DeviceScene.from_native: %d frames, %d poses" % (done, N))
        return self

    @classmethod
    def from_native_records(cls, record, sparse, frames, dpt, depths_h=None, img_wh=None, batch=32, device="cuda", scan=0):
        """`from_native` with `formats.load_poses_bounds`'s record, as `from_records` is to `from_arrays`."""
        return cls.from_native(record["poses"], record["focal"], record["bounds"], sparse, frames, dpt, depths_h, img_wh, batch, device, scan)

    def n_keypoints(self, frame):
        return self.offsets[frame + 1] - self.offsets[frame]

    def sample(self, target, src_views, perm=None, unpreprocess=False):
        """The reference's sample for (target, src_views) with the keys of data/scared.py:501-521 and the shapes its DataLoader gives at
        batch_size=1, all on the device, from one launch: images [1,V,3,H,W], depths_h, dpt, sparse_depths, sparse_depths_weight [1,H,W],
        sparse_depths_ms / weight_ms {stage1, stage2, stage3}, rays_depth [1,min(n_kp,1024),3,3], w2cs, c2ws [1,V,4,4], near_fars [1,1,V,2],
        proj_mats [1,V,3,4], intrinsics [1,V,3,3], view_ids [1,V] int64, affine_mat, affine_mat_inv [1,V,3,4,4], scan [1]; with
        unpreprocess=True also images_unpre, train.py:61-70 applied to images in the same launch.

        perm: int32 device tensor of at least min(n_kp, 1024) distinct indices below n_kp -- the reference's np.random.shuffle(...)[:1024]; row
        i of rays_depth is keypoint perm[i].  None draws torch.randperm(n_kp) on the device (n_kp is known on the host: nothing is read back).

        dpt, depths_h, sparse_depths, sparse_depths_weight, the two stage3 entries and scan are VIEWS into the resident arrays: they must not be
        written.  Everything else is freshly written memory of this call."""
        from .. import ops
        target = int(target)
        view_ids = [target] + [int(s) for s in src_views]
        if not 0 <= target < self.N:
            raise IndexError("DeviceScene.sample: target %d outside 0..%d" % (target, self.N - 1))
        n_kp = self.n_keypoints(target)
        n_rows = min(n_kp, MAX_ROWS)
        if perm is None and n_rows:
            perm = torch.randperm(n_kp, device=self.device, dtype=torch.int32)
        o = ops.sample_assemble(self, view_ids, perm, n_rows, unpreprocess=unpreprocess)
        t = slice(target, target + 1)
        sparse, weight = self.depth_img[t], self.weight_img[t]
        out = {"images": o["images"], "depths_h": self.depths_h[t], "dpt": self.dpt[t],
               "sparse_depths_ms": {"stage1": o["sd1"], "stage2": o["sd2"], "stage3": sparse}, "sparse_depths": sparse,
               "sparse_depths_weight": weight, "weight_ms": {"stage1": o["wt1"], "stage2": o["wt2"], "stage3": weight},
               "rays_depth": o["rays_depth"], "w2cs": o["w2cs"], "c2ws": o["c2ws"], "near_fars": o["near_fars"], "proj_mats": o["proj_mats"],
               "intrinsics": o["intrinsics"], "view_ids": o["view_ids"], "affine_mat": o["affine_mat"], "affine_mat_inv": o["affine_mat_inv"],
               "scan": self.scan}
        if unpreprocess:
            out["images_unpre"] = o["images_unpre"]
        return out

    def sample_pose(self, poses, index, n_views, candidates=None, intrinsic=None, unpreprocess=False):
        """The batch of a FREE camera pose, `poses[index]`, from one launch (`ops.novel_assemble`): what a rendered novel view starts from.
        poses: contiguous float32 device tensor [P,3,4], camera-to-world (upload a path once, then loop `index`); n_views: views of the batch,
        the pose and its n_views - 1 nearest source frames, picked ON THE DEVICE among `candidates` by camera-centre distance
        (`formats.get_nearest_pose_ids`'s criterion; ties to the earlier candidate, NaN last).  candidates: an int32 device tensor (used as it
        is), or a sequence of frame ids (uploaded by this call: one blocking copy), or None = the training index of `metas()` at its default
        sample_rate, uploaded once and kept on the object.  At least n_views candidates are needed.  intrinsic: float32 device [3,3] with zero
        skew, default frame 0's.
        -> images [1,V,3,H,W] (slot 0 all zeros: there is no ground truth; nothing on the render path reads it), w2cs, c2ws [1,V,4,4],
        near_fars [1,1,V,2], proj_mats [1,V,3,4], intrinsics [1,V,3,3], view_ids [1,V] int64 (slot 0 is -1), affine_mat, affine_mat_inv
        [1,V,3,4,4], scan [1]; with unpreprocess=True also images_unpre.  No depths_h, dpt, sparse_* or rays_depth: a free pose has none.
        Slot 0's w2c and affine_mat_inv are closed-form RIGID inverses of the pose given, not LU inverses: a rotation block that is not
        orthonormal gives what the formulas give.  No host arithmetic on matrices, no synchronisation, nothing read back; the ids of the
        selected frames exist only on the device."""
        from .. import ops
        if candidates is None:
            candidates = getattr(self, "_train_candidates", None)
            if candidates is None:
                candidates = self._train_candidates = torch.from_numpy(self.train_index().astype(np.int32)).to(self.device)
        elif not torch.is_tensor(candidates):
            candidates = torch.from_numpy(np.ascontiguousarray(np.asarray(candidates), dtype=np.int32)).to(self.device)
        o = ops.novel_assemble(self, poses, index, candidates, n_views, intrinsic=intrinsic, unpreprocess=unpreprocess)
        o["scan"] = self.scan
        return o

    def train_index(self, sample_rate=2):
        """The frames of the training split (data/scared.py:248-252): sample_rate // 2 :: sample_rate; the others are the test index."""
        return np.arange(self.N)[int(sample_rate / 2)::sample_rate]

    def nearest_train_views(self, frame, n_views, sample_rate=2):
        """The n_views - 1 training frames nearest to `frame` (`formats.get_nearest_pose_ids`), the frame itself left out: what
        `metas("val", n_views, sample_rate)` lists for a test frame, for any frame.  Host arithmetic; needs the scene's poses."""
        if self.poses is None:
            raise ValueError("DeviceScene.nearest_train_views needs the poses the scene was built from")
        train_index = self.train_index(sample_rate)
        at = np.nonzero(train_index == int(frame))[0]
        near = formats.get_nearest_pose_ids(self.poses[int(frame)], self.poses[train_index], n_views - 1, tar_id=int(at[0]) if len(at) else -1)
        return [int(i) for i in train_index[near]]

    def fusion_sources(self, frames, n_src):
        """int32 [len(frames), n_src] on the device: `fusion.source_table` of these frames' poses (positions in `frames`, -1 padding), for
        `ops.depth_consistency`.  Host arithmetic and one upload; the LAST table is kept (one entry, replaced when `frames` or `n_src`
        change), so a repeated reconstruction of the same frames uploads nothing."""
        from ..fusion import source_table
        if self.poses is None:
            raise ValueError("DeviceScene.fusion_sources needs the poses the scene was built from")
        key = (tuple(int(f) for f in frames), int(n_src))
        kept = getattr(self, "_fusion_sources", None)
        if kept is None or kept[0] != key:
            kept = self._fusion_sources = (key, torch.from_numpy(source_table(self.poses[list(key[0])], key[1])).to(self.device))
        return kept[1]

    def metas(self, split, n_views, sample_rate=2, num_samples=200, rng=None):
        """The (target, src_views) list of the reference's build_metas (data/scared.py:248-273).  Frames sample_rate // 2 :: sample_rate are the
        train index, the others the test index.  "train": `num_samples` entries; before each one `rng.shuffle` is applied to the train index in
        place (cumulatively, as the reference does with Python's `random`; pass `rng=random` for its very draws; default numpy's
        default_rng()), the first element is the target, the next n_views - 1 the sources.  "val": one entry per test frame with the
        n_views - 1 nearest train poses (`formats.get_nearest_pose_ids`); needs the scene's poses."""
        ids = np.arange(self.N)
        train_index = self.train_index(sample_rate)
        test_index = np.array([i for i in ids if i not in train_index])
        out = []
        if split == "train":
            rng = np.random.default_rng() if rng is None else rng
            select = train_index.copy()
            for _ in range(num_samples):
                rng.shuffle(select)
                out.append((int(select[0]), np.array(select[1:n_views]).tolist()))
        elif split == "val":
            if self.poses is None:
                raise ValueError("DeviceScene.metas('val') needs the poses the scene was built from")
            for k in range(len(test_index)):
                ref = int(test_index[k])
                near = formats.get_nearest_pose_ids(self.poses[ref], self.poses[train_index], n_views - 1)
                out.append((ref, np.array(train_index)[near].tolist()))
        else:
            raise ValueError("DeviceScene.metas: split must be 'train' or 'val', got %r" % (split,))
        return out
