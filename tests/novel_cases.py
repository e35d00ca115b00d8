"""Shared builders and the float64 restatement for the free-camera tests (tests/test_novel_host.py, tests/test_hip_novel.py).  CPU only.

`novel_matrices` restates, in float64 on the float32 inputs, what ucnerf_novel_assemble forms for slot 0: the rigid inverse [R^T | -R^T t], the
stage matrices K_s . w2c[:3,:4] and their inverses c2w . diag(K_s^-1, 1).  `select` restates the source-view choice: the stable argsort of the
float64 squared centre distances (numpy sorts NaN last, and `kind="stable"` keeps positions in order among equals and among NaNs).

Scenes (tests/sample_cases.make_scene, three keypoints a frame -- a free pose uses none of them):
  n15x21   N = 20 frames of 15 x 21: H W = 315 and 3 H W = 945 are no multiples of 4 (the last thread of an image holds 3 pixels, the last dword
           of a frame is the padding's), 315 pixels = 79 threads, one workgroup a view; the train index 1, 3, .., 19 holds ten frames, enough
           for V = SAMPLE_MAX_VIEWS = 9.  Frames 4 and 12 (both outside the train index) carry the identical pose.
  n16x20   N = 10 frames of 16 x 20 (the float4 store route).
  n40x52   N = 8 frames of 40 x 52: 2080 pixels = 520 threads, three workgroups a view.
"""
import numpy as np

import sample_cases as SC

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


SCENES = {"n15x21": dict(H=15, W=21, N=20, seed=71, twins=(4, 12)), "n16x20": dict(H=16, W=20, N=10, seed=72), "n40x52": dict(H=40, W=52, N=8, seed=73)}
_scenes = {}


def scene(name):
    if name not in _scenes:
        cfg = SCENES[name]
        sc = SC.make_scene(cfg["H"], cfg["W"], (3,) * cfg["N"], cfg["seed"])
        if "twins" in cfg:
            a, b = cfg["twins"]
            sc["poses"][b] = sc["poses"][a]
        _scenes[name] = sc
    return _scenes[name]


def device_scene(name, device):
    from uc_nerf_amd.data import DeviceScene
    sc = scene(name)
    return DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"], sc["dpt"], sc["depths_h"], sc["img_wh"], device=device)


def scene_intrinsic(sc):
    """The resident intrinsic of every frame of a scene, as data/scared.py:466 forms it, float32 [3,3]."""
    W, H = sc["img_wh"]
    return np.array([[sc["focal"][0], 0, W / 2], [0, sc["focal"][1], H / 2], [0, 0, 1]], dtype=np.float32)


def free_poses(n, seed):
    """n camera-to-world poses [n,3,4] float32 in the range of the scenes' own (rotations up to 0.2 rad an axis, centres in [-0.5, 0.5]^3)."""
    rs = np.random.RandomState(seed)
    return np.stack([np.concatenate([SC._rotation(rs), rs.uniform(-0.5, 0.5, (3, 1))], 1) for _ in range(n)]).astype(np.float32)


def novel_matrices(pose32, K32):
    """float64 restatement on float32 inputs.  -> dict(c2w, w2c [4,4], affine, affine_inv [3,4,4]) in float64."""
    pose, K = np.asarray(pose32, dtype=np.float32).astype(np.float64), np.asarray(K32, dtype=np.float32).astype(np.float64)
    R, t = pose[:, :3], pose[:, 3]
    c2w, w2c = np.eye(4), np.eye(4)
    c2w[:3] = pose
    w2c[:3, :3] = R.T
    w2c[:3, 3] = -(R.T @ t)
    affine, affine_inv = np.stack([np.eye(4)] * 3), np.stack([np.eye(4)] * 3)
    for s in range(3):
        Ks = K.copy()
        Ks[:2] /= 2 ** (2 - s)
        affine[s, :3, :4] = Ks @ w2c[:3, :4]
        fx, fy, cx, cy = Ks[0, 0], Ks[1, 1], Ks[0, 2], Ks[1, 2]
        Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])          # zero skew
        affine_inv[s, :3, :3] = R @ Kinv
        affine_inv[s, :3, 3] = t
    return {"c2w": c2w, "w2c": w2c, "affine": affine, "affine_inv": affine_inv}


def distances(t32, centres32, cand):
    """float64 squared distances of the camera centres centres32[cand[k]] (float32 values) to t32."""
    c = np.asarray(centres32, dtype=np.float32).astype(np.float64)[np.asarray(cand)]
    return ((c - np.asarray(t32, dtype=np.float32).astype(np.float64)) ** 2).sum(1)


def select(t32, centres32, cand, n_src):
    """-> (the selected frame ids, the float64 distances): cand[np.argsort(d64, kind="stable")[:n_src]]."""
    d = distances(t32, centres32, cand)
    return np.asarray(cand)[np.argsort(d, kind="stable")[:n_src]], d


def well_separated(d, rel=1e-4):
    """True when float32 rounding cannot reorder the distances: consecutive sorted values are either identical (the same centre twice: the
    float32 distances are identical too, position decides) or at least `rel` apart relative to the larger; NaNs (sorted last) are left out."""
    s = np.sort(d[~np.isnan(d)])
    gap, big = np.diff(s), s[1:]
    return bool(np.all((gap == 0) | (gap >= rel * big)))
