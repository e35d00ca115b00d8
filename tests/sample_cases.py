"""Cases and the host restatement for the sample-assembly tests (tests/test_sample_host.py, tests/test_hip_sample.py).

`reference_sample` restates the reference's ScaredDataset.__getitem__ (data/scared.py:387-522) on ALREADY DECODED arrays, with the calls the
reference uses: float64 maps normalised in place (on a copy), np.repeat / np.concatenate for the keypoint rows, float32 torch tensors with
torch.inverse and np.linalg.inv for the matrices, `proj_mat_l @ ref_proj_inv` through torch.  What the reference gets from libraries this
project does not depend on is written out:
  * ToTensor + Normalize as np.float32(u) / np.float32(255), then - float32 mean, then / float32 std (torchvision is not importable here:
    not verified against torchvision; tests/test_sample_host.py checks it against the same torch calls torchvision makes);
  * cv2.resize(..., INTER_NEAREST) as the index formula min(floor(dst * (size / (size // k))), size - 1) in double (not verified against
    OpenCV: cv2 is not importable here).
The result is returned as float32 with the DataLoader's leading batch dimension of one (the package's documented difference: the reference's
np.zeros maps arrive as float64).  rays_depth is [n,3,3]: the reference's concatenate of the depth, weight and (h, w, 1) rows along axis 1
makes three rows (its comment says N x 4 x 3).

Scenes are the smallest at which each part can go wrong: 8 x 12 (multiples of 4), 10 x 14 (neither: clamped index maps), 5 x 7 (H W = 35, no
multiple of the four pixels a thread takes: the ragged vector tail); N = 4 frames; keypoints per frame 0, 3, exactly 1024 and 1030 (truncation;
coordinates repeat, later keypoints overwrite earlier ones in the maps); one frame whose weights are all equal (NaN); frames holding every
byte value in every channel.
"""
import numpy as np
import torch

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]


def pyramid_index(size, k):
    d = size // k
    return np.minimum(np.floor(np.arange(d) * (size / d)), size - 1).astype(np.int64) if d else np.zeros(0, np.int64)


def nearest_level(img, k):
    H, W = img.shape
    return img[np.ix_(pyramid_index(H, k), pyramid_index(W, k))]


def normalise(img_u8):
    """ToTensor then Normalize on one uint8 [H,W,3] frame -> float32 [3,H,W]."""
    x = img_u8.astype(np.float32) / np.float32(255)
    x = np.ascontiguousarray(x.transpose(2, 0, 1))
    mean, std = np.array(MEAN, np.float32)[:, None, None], np.array(STD, np.float32)[:, None, None]
    return (x - mean) / std


def unpreprocess(images):
    """train.py:61-70 on float32 [...,3,H,W]."""
    mean = np.array([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]).astype(np.float32)[:, None, None]
    std = np.array([1 / 0.229, 1 / 0.224, 1 / 0.225]).astype(np.float32)[:, None, None]
    return (images - mean) / std


def reference_sample(scene, target, src_views, perm=None):
    """scene: dict(poses [N,3,4], focal (fx, fy), bounds [N,2], sparse [per frame: depth, coord, weight, depth_img, weight_img], frames uint8
    [N,H,W,3], dpt, depths_h [N,H,W] float32, img_wh (W, H)).  perm: the row order standing for np.random.shuffle (None: the list's own)."""
    img_wh = scene["img_wh"]
    view_ids = [target] + list(src_views)
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = scene["sparse"][target]
        sparse_depth_img = np.array(rec["depth_img"], dtype=np.float64)
        weight_img = np.array(rec["weight_img"], dtype=np.float64)
        weight_img -= weight_img.min()
        weight_img /= weight_img.max()
        n = len(rec["depth"])
        if n:
            depth_value = np.repeat(np.asarray(rec["depth"], dtype=np.float64)[:, None, None], 3, axis=2)
            depth_coord = np.asarray(rec["coord"])
            depth_coord = np.concatenate((depth_coord.reshape(-1, 1, 2), np.ones((depth_coord.shape[0], 1, 1))), axis=2)
            weights = np.repeat(np.asarray(rec["weight"], dtype=np.float64)[:, None, None], 3, axis=2)
            weights -= weights.min()
            weights /= weights.max()
            rays_depth = np.concatenate([depth_value, weights, depth_coord], axis=1)
        else:
            rays_depth = np.zeros((0, 3, 3))          # (the reference raises on a frame without keypoints; an empty list here)
    if perm is not None:
        rays_depth = rays_depth[np.asarray(perm, dtype=np.int64)[:min(n, 1024)]]
    rays_depth = rays_depth[:1024]

    near_far = [scene["bounds"].min() * 0.9, scene["bounds"].max() * 1.1]
    imgs, near_fars, affine_mat, affine_mat_inv, proj_mats, intrinsics, w2cs, c2ws = [], [], [], [], [], [], [], []
    for i, vid in enumerate(view_ids):
        near_fars.append(near_far)
        imgs.append(normalise(scene["frames"][vid]))
        c2w = torch.eye(4).float()
        c2w[:3] = torch.FloatTensor(scene["poses"][vid])
        w2c = torch.inverse(c2w)
        c2ws.append(c2w)
        w2cs.append(w2c)
        intrinsic = torch.tensor([[scene["focal"][0], 0, img_wh[0] / 2], [0, scene["focal"][1], img_wh[1] / 2], [0, 0, 1]]).float()
        intrinsics.append(intrinsic.clone())
        aff, aff_inv = [], []
        for scale in range(3):
            proj_mat_l = torch.eye(4)
            stage_intrinsic = intrinsic.clone()
            stage_intrinsic[:2] = intrinsic[:2] / (2 ** (2 - scale))
            proj_mat_l[:3, :4] = stage_intrinsic @ w2c[:3, :4]
            aff.append(proj_mat_l)
            aff_inv.append(np.linalg.inv(proj_mat_l))
        aff, aff_inv = np.stack(aff), np.stack(aff_inv)
        affine_mat.append(aff)
        affine_mat_inv.append(aff_inv)
        proj_mat_l = torch.tensor(aff[2])
        if i == 0:
            ref_proj_inv = torch.inverse(proj_mat_l)
            proj_mats.append(torch.eye(4))
        else:
            proj_mats.append(proj_mat_l @ ref_proj_inv)
    images = np.stack(imgs).astype(np.float32)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))[None]          # noqa: E731
    t = target
    out = {"images": f32(images), "images_unpre": f32(unpreprocess(images)), "depths_h": f32(scene["depths_h"][t]), "dpt": f32(scene["dpt"][t]),
           "sparse_depths_ms": {"stage1": f32(nearest_level(sparse_depth_img, 4)), "stage2": f32(nearest_level(sparse_depth_img, 2)),
                                "stage3": f32(sparse_depth_img)},
           "sparse_depths": f32(sparse_depth_img), "sparse_depths_weight": f32(weight_img),
           "weight_ms": {"stage1": f32(nearest_level(weight_img, 4)), "stage2": f32(nearest_level(weight_img, 2)), "stage3": f32(weight_img)},
           "rays_depth": f32(rays_depth.astype(np.float32)), "w2cs": f32(np.stack(w2cs)), "c2ws": f32(np.stack(c2ws)),
           "near_fars": f32(np.stack([near_fars])), "proj_mats": f32(np.stack(proj_mats)[:, :3]), "intrinsics": f32(np.stack(intrinsics)),
           "view_ids": torch.from_numpy(np.array(view_ids))[None], "affine_mat": f32(np.stack(affine_mat)),
           "affine_mat_inv": f32(np.stack(affine_mat_inv)), "scan": torch.tensor([scene.get("scan", 0)]),
           "_ref_proj_inv": ref_proj_inv.clone()}
    return out


def reference_metas(n_frames, poses, split, n_views, sample_rate, num_samples, rng):
    """build_metas (data/scared.py:248-273) for one scan; `rng` stands for the module `random`."""
    from uc_nerf_amd.data.formats import get_nearest_pose_ids
    ids = np.arange(n_frames)
    train_index = ids[int(sample_rate / 2)::sample_rate]
    test_index = np.array([i for i in ids if i not in train_index])
    metas = []
    if split == "val":
        num_samples = len(test_index)
    for k in range(num_samples):
        if split == "train":
            random_select = train_index
            rng.shuffle(random_select)
            ref_view = random_select[0]
            src_views = np.array(random_select[1:n_views]).tolist()
        else:
            ref_view = test_index[k]
            src_views = get_nearest_pose_ids(poses[ref_view], poses[train_index], n_views - 1)
            src_views = np.array(train_index)[src_views].tolist()
        metas.append((int(ref_view), src_views))
    return metas


# ------------------------------------------------------------------------------------------------ scenes
def _rotation(rs):
    a = rs.uniform(-0.2, 0.2, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def make_scene(H, W, kp_counts, seed, equal_weights=()):
    """N = len(kp_counts) frames.  Keypoints in the order the dataset code appends them: the maps take the LAST keypoint at a coordinate.
    Frames in `equal_weights` carry one weight for all their keypoints (the 0 / 0 case).  The bytes of the frames run through 0..255 in every
    channel (channel c shifted by 85 c), continuing from frame to frame."""
    rs = np.random.RandomState(seed)
    N = len(kp_counts)
    poses = np.stack([np.concatenate([_rotation(rs), rs.uniform(-0.5, 0.5, (3, 1))], 1) for _ in range(N)])
    sparse = []
    for f, n in enumerate(kp_counts):
        depth = rs.uniform(1.0, 5.0, n)
        weight = np.full(n, 1.25) if f in equal_weights else 2 * np.exp(-rs.uniform(0.0, 2.0, n) ** 2)
        coord = np.stack([rs.randint(0, H, n), rs.randint(0, W, n)], 1).astype(np.int64).reshape(n, 2)
        depth_img, weight_img = np.zeros((H, W)), np.zeros((H, W))
        for k in range(n):
            weight_img[coord[k, 0], coord[k, 1]] = weight[k]
            depth_img[coord[k, 0], coord[k, 1]] = depth[k]
        sparse.append({"depth": depth, "coord": coord, "weight": weight, "depth_img": depth_img, "weight_img": weight_img})
    pix = np.arange(N * H * W).reshape(N, H, W, 1)
    frames = ((pix + 85 * np.arange(3)) % 256).astype(np.uint8)
    return {"poses": poses, "focal": [np.float64(0.9 * W), np.float64(1.1 * H)], "bounds": rs.uniform(0.5, 6.0, (N, 2)), "sparse": sparse,
            "frames": frames, "dpt": rs.rand(N, H, W).astype(np.float32), "depths_h": rs.rand(N, H, W).astype(np.float32), "img_wh": (W, H)}


SCENES = {
    "a8x12": dict(H=8, W=12, kp_counts=(0, 3, 1024, 1030), seed=11),
    "b10x14": dict(H=10, W=14, kp_counts=(1030, 3, 0, 1024), seed=12, equal_weights=(1,)),
    "c5x7": dict(H=5, W=7, kp_counts=(2, 4, 0, 7), seed=13),
}

# (scene, target, src_views): V = 1, 2 and 9; every keypoint count as a target; the target among the sources; all four frames (every byte)
CASES = [
    ("a8x12", 0, []),                              # V = 1, no keypoint: an empty rays_depth, an all-NaN weight map
    ("a8x12", 1, [2]),                             # V = 2, 3 keypoints
    ("a8x12", 2, [2, 0]),                          # exactly 1024 keypoints, the target among the sources
    ("a8x12", 3, [0, 1, 2, 3, 0, 1, 2, 3]),        # V = 9, 1030 keypoints (truncation), every frame
    ("b10x14", 0, [1, 2, 3, 0, 3, 2, 1, 0]),       # V = 9 at 10 x 14, 1030 keypoints
    ("b10x14", 1, [3]),                            # equal weights: NaN rows
    ("b10x14", 2, []),                             # V = 1, no keypoint
    ("b10x14", 3, [0, 1, 2, 3]),                   # V = 5, 1024 keypoints
    ("c5x7", 3, [0, 1]),                           # H W = 35: the last thread of an image holds 3 pixels
    ("c5x7", 2, []),
]
CASE_IDS = ["%s-t%d-V%d" % (s, t, 1 + len(v)) for s, t, v in CASES]

_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = make_scene(**SCENES[name])
    return _scenes[name]


def case_perm(name, target):
    """A fixed permutation of the target's keypoints (int64 numpy), standing for the reference's shuffle."""
    n = len(scene(name)["sparse"][target]["depth"])
    return np.random.RandomState(100 + target).permutation(n)
