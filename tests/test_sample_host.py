"""Host-side checks of the device-resident scene (uc_nerf_amd/data/scene.py) and of tests/sample_cases.py's restatement of the reference's
sample assembly.  No GPU: the restatement against hand-worked values, DeviceScene's per-frame constants (on device="cpu" storage) bit-equal to the
restatement's, `metas` against build_metas, a scene read through the COLMAP / LLFF readers, and ucnerf_sample_assemble's argument checks."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import sample_cases as SC
from uc_nerf_amd.data import DeviceScene, formats, scene as S

HERE = os.path.dirname(os.path.abspath(__file__))


def _equal(a, b):
    """Bit for bit on float32, NaN positions equal."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def _two_frame_scene():
    H = W = 4
    poses = np.zeros((2, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[1, 0, 3] = 1.0                                              # frame 1 sits one unit along x
    depth_img, weight_img = np.zeros((H, W)), np.zeros((H, W))
    depth_img[2, 2], depth_img[3, 0], weight_img[2, 2], weight_img[3, 0] = 2.0, 4.0, 0.5, 1.5
    kp = {"depth": np.array([2.0, 4.0]), "coord": np.array([[2, 2], [3, 0]]), "weight": np.array([0.5, 1.5]), "depth_img": depth_img, "weight_img": weight_img}
    empty = {"depth": np.zeros(0), "coord": np.zeros((0, 2), np.int64), "weight": np.zeros(0), "depth_img": np.zeros((H, W)), "weight_img": np.zeros((H, W))}
    frames = np.zeros((2, H, W, 3), np.uint8)
    frames[0, 0, 0], frames[0, 0, 1], frames[1] = (255, 51, 0), (0, 255, 102), 255
    return {"poses": poses, "focal": [np.float64(2.0), np.float64(2.0)], "bounds": np.array([[1.0, 4.0], [2.0, 5.0]]), "sparse": [kp, empty], "frames": frames,
            "dpt": np.full((2, H, W), 0.25, np.float32), "depths_h": np.full((2, H, W), 0.5, np.float32), "img_wh": (W, H)}


def test_restatement_gives_the_hand_worked_sample_of_a_two_frame_scene():
    sc = _two_frame_scene()
    before = sc["sparse"][0]["weight_img"].copy()
    r = SC.reference_sample(sc, 0, [1])
    assert np.array_equal(sc["sparse"][0]["weight_img"], before)               # the restatement works on copies
    f = np.float32
    m, s = [f(x) for x in SC.MEAN], [f(x) for x in SC.STD]
    img = r["images"]
    assert img.shape == (1, 2, 3, 4, 4) and img.dtype == torch.float32
    assert img[0, 0, 0, 0, 0] == (f(1.0) - m[0]) / s[0] and img[0, 0, 1, 0, 0] == (f(51) / f(255) - m[1]) / s[1] and img[0, 0, 2, 0, 0] == (f(0) - m[2]) / s[2]
    assert img[0, 0, 2, 0, 1] == (f(102) / f(255) - m[2]) / s[2] and img[0, 1, 1, 3, 3] == (f(1.0) - m[1]) / s[1]
    um, us = f(-0.485 / 0.229), f(1 / 0.229)
    assert r["images_unpre"][0, 0, 0, 0, 0] == (((f(1.0) - m[0]) / s[0]) - um) / us
    # keypoint rows: [depth x3], [normalised weight x3], [h, w, 1] -- three rows, not the four of the reference's comment
    assert r["rays_depth"].shape == (1, 2, 3, 3)
    assert r["rays_depth"][0].tolist() == [[[2, 2, 2], [0, 0, 0], [2, 2, 1]], [[4, 4, 4], [1, 1, 1], [3, 0, 1]]]
    assert SC.reference_sample(sc, 0, [1], perm=[1, 0])["rays_depth"][0, 0].tolist() == [[4, 4, 4], [1, 1, 1], [3, 0, 1]]
    assert SC.reference_sample(sc, 1, [0])["rays_depth"].shape == (1, 0, 3, 3)
    # maps: weights divided by their maximum in double, rounded once; level 2 takes rows / columns 0 and 2, level 1 the corner
    assert r["sparse_depths_weight"][0, 2, 2] == f(0.5 / 1.5) and r["sparse_depths_weight"][0, 3, 0] == 1 and r["sparse_depths"][0, 3, 0] == 4
    assert r["sparse_depths_ms"]["stage2"][0].tolist() == [[0, 0], [0, 2]] and r["sparse_depths_ms"]["stage1"][0].tolist() == [[0]]
    assert r["weight_ms"]["stage2"][0, 1, 1] == f(0.5 / 1.5) and r["weight_ms"]["stage3"].shape == (1, 4, 4)
    assert torch.isnan(SC.reference_sample(sc, 1, [0])["sparse_depths_weight"]).all()             # 0 / 0 on a frame without keypoints
    # matrices
    assert r["intrinsics"][0, 1].tolist() == [[2, 0, 2], [0, 2, 2], [0, 0, 1]]
    assert r["w2cs"][0, 1].tolist() == [[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]] and r["c2ws"][0, 1, 0, 3] == 1
    assert r["affine_mat"][0, 1, 2].tolist() == [[2, 0, 2, -2], [0, 2, 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert r["affine_mat"][0, 1, 0].tolist() == [[0.5, 0, 0.5, -0.5], [0, 0.5, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert r["affine_mat_inv"][0, 0, 2].tolist() == [[0.5, 0, -1, 0], [0, 0.5, -1, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert r["proj_mats"][0].tolist() == [[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, -2], [0, 1, 0, 0], [0, 0, 1, 0]]]
    assert r["near_fars"].shape == (1, 1, 2, 2) and r["near_fars"][0, 0, 1].tolist() == [float(f(0.9)), float(f(5.5))]
    assert r["view_ids"].tolist() == [[0, 1]] and r["view_ids"].dtype == torch.int64 and r["dpt"].shape == (1, 4, 4)


def test_normalisation_is_what_torch_does_for_every_byte():
    """ToTensor is `.to(float32).div(255)`, Normalize `.sub_(mean).div_(std)` with float32 mean / std [3,1,1] (torchvision's functional code;
    torchvision itself is not importable here): the restatement's numpy arithmetic equals those torch calls on every byte in every channel."""
    u = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1).reshape(16, 16, 3)
    t = torch.from_numpy(u).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean, std = torch.as_tensor(SC.MEAN, dtype=torch.float32).view(-1, 1, 1), torch.as_tensor(SC.STD, dtype=torch.float32).view(-1, 1, 1)
    t = t.clone().sub_(mean).div_(std)
    got = SC.normalise(u)
    assert got.dtype == np.float32 and np.array_equal(got, t.numpy())
    mean_u = torch.tensor([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]).view(1, 3, 1, 1)
    std_u = torch.tensor([1 / 0.229, 1 / 0.224, 1 / 0.225]).view(1, 3, 1, 1)
    assert np.array_equal(SC.unpreprocess(got[None]), ((t[None] - mean_u) / std_u).numpy())
    try:
        from torchvision import transforms as T
    except ImportError:
        return
    tv = T.Compose([T.ToTensor(), T.Normalize(mean=SC.MEAN, std=SC.STD)])(u)
    assert np.array_equal(got, tv.numpy())


def test_pyramid_index_maps():
    assert S.pyramid_index(8, 4).tolist() == [0, 4] and S.pyramid_index(12, 2).tolist() == [0, 2, 4, 6, 8, 10]
    assert S.pyramid_index(10, 4).tolist() == [0, 5] and S.pyramid_index(14, 4).tolist() == [0, 4, 9] and S.pyramid_index(5, 2).tolist() == [0, 2]
    assert S.pyramid_index(7, 4).tolist() == [0] and S.pyramid_index(3, 4).tolist() == [] and S.pyramid_index(14, 4).dtype == np.int32
    for size in (5, 7, 10, 14, 256, 320):
        for k in (2, 4):
            assert np.array_equal(S.pyramid_index(size, k), SC.pyramid_index(size, k)) and (S.pyramid_index(size, k) < size).all()
    try:
        import cv2
    except ImportError:
        return
    for H, W in ((8, 12), (10, 14), (5, 7), (256, 320)):
        img = np.random.RandomState(0).rand(H, W)
        for k in (2, 4):
            if H // k and W // k:
                assert np.array_equal(cv2.resize(img, (W // k, H // k), interpolation=cv2.INTER_NEAREST), SC.nearest_level(img, k))


def _host_scene(name):
    sc = SC.scene(name)
    return sc, DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"], sc["dpt"], sc["depths_h"], sc["img_wh"], device="cpu")


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_per_frame_constants_equal_the_restatement_bit_for_bit(name):
    sc, ds = _host_scene(name)
    N, (W, H) = len(sc["poses"]), sc["img_wh"]
    assert (ds.N, ds.H, ds.W) == (N, H, W) and ds.frames.shape == (N, (3 * H * W + 3) // 4 * 4) and ds.frames.dtype == torch.uint8
    assert np.array_equal(ds.frames[:, :3 * H * W].numpy().reshape(N, H, W, 3), sc["frames"])
    assert ds.offsets == np.concatenate([[0], np.cumsum(SC.SCENES[name]["kp_counts"])]).tolist()
    saved = [s["weight_img"].copy() for s in sc["sparse"]]
    for t in range(N):
        r = SC.reference_sample(sc, t, [(t + 1) % N])
        assert _equal(ds.c2w[t], r["c2ws"][0, 0]) and _equal(ds.w2c[t], r["w2cs"][0, 0]) and _equal(ds.intrinsic[t], r["intrinsics"][0, 0])
        assert _equal(ds.affine[t], r["affine_mat"][0, 0]) and _equal(ds.affine_inv[t], r["affine_mat_inv"][0, 0])
        assert _equal(ds.ref_proj_inv[t], r["_ref_proj_inv"])
        assert _equal(ds.depth_img[t], r["sparse_depths"][0]) and _equal(ds.weight_img[t], r["sparse_depths_weight"][0])
        a, b = ds.offsets[t], ds.offsets[t + 1]
        rows = r["rays_depth"][0]                                              # the list's own order, the first 1024
        n = rows.shape[0]
        assert n == min(b - a, 1024)
        assert _equal(ds.kp_depth[a:a + n], rows[:, 0, 0]) and _equal(ds.kp_weight[a:a + n], rows[:, 1, 0])
        assert _equal(ds.kp_coord[a:a + n].to(torch.float32), rows[:, 2, :2]) and ds.kp_coord.dtype == torch.int32
        assert ds.near_far == tuple(r["near_fars"][0, 0, 0].tolist())
        for lvl, (rows_i, cols_i) in (("stage1", (ds.row1, ds.col1)), ("stage2", (ds.row2, ds.col2))):
            assert _equal(ds.depth_img[t][rows_i.long()][:, cols_i.long()], r["sparse_depths_ms"][lvl][0])
            assert _equal(ds.weight_img[t][rows_i.long()][:, cols_i.long()], r["weight_ms"][lvl][0])
    assert all(np.array_equal(s["weight_img"], w) for s, w in zip(sc["sparse"], saved))       # the caller's arrays are not normalised in place
    assert ds.mean == [float(np.float32(m)) for m in SC.MEAN] and ds.unpre_std[0] == float(np.float32(1 / 0.229))


def test_equal_weights_stay_nan_and_raise_nothing():
    sc, ds = _host_scene("b10x14")
    a, b = ds.offsets[1], ds.offsets[2]
    assert b - a == 3 and torch.isnan(ds.kp_weight[a:b]).all() and not torch.isnan(ds.kp_weight[:a]).any()
    assert torch.isnan(ds.weight_img[2]).all()                                 # a frame without keypoints: 0 / 0 everywhere
    with np.errstate(all="raise"):                                             # (the builder silences the division itself)
        assert np.isnan(S.normalise_weights(np.full(4, 1.25))).all() and S.normalise_weights(np.zeros(0)).size == 0
    with pytest.raises(RuntimeError, match="ROCm device"):
        ds.sample(0, [1])                                                      # no host route


@pytest.mark.parametrize("sample_rate,n_views", [(2, 3), (3, 4)])
def test_metas_follow_build_metas(sample_rate, n_views):
    sc = SC.scene("a8x12")
    rs = np.random.RandomState(5)
    N = 11
    poses = np.stack([np.concatenate([np.eye(3), rs.uniform(-1, 1, (3, 1))], 1) for _ in range(N)])
    ds = DeviceScene.__new__(DeviceScene)
    ds.N, ds.poses = N, poses
    for make in (lambda: random.Random(3), lambda: np.random.RandomState(3)):
        got = ds.metas("train", n_views, sample_rate=sample_rate, num_samples=7, rng=make())
        assert got == SC.reference_metas(N, poses, "train", n_views, sample_rate, 7, make()) and len(got) == 7
        assert all(isinstance(t, int) and len(s) == n_views - 1 and t not in s for t, s in got)
    val = ds.metas("val", n_views, sample_rate=sample_rate)
    assert val == SC.reference_metas(N, poses, "val", n_views, sample_rate, None, None)
    train = set(range(N)[sample_rate // 2::sample_rate])
    assert [t for t, _ in val] == [i for i in range(N) if i not in train] and all(set(s) <= train for _, s in val)
    assert len(ds.metas("train", n_views, sample_rate=sample_rate, num_samples=2)) == 2          # default rng
    with pytest.raises(ValueError):
        ds.metas("test", n_views)
    assert sc["frames"].shape[0] == 4


def test_scene_from_the_colmap_and_llff_readers():
    root = os.path.join(HERE, "golden", "colmap_tiny")
    img_wh = (32, 24)
    imgs = formats.read_images_binary(os.path.join(root, "sparse", "0", "images.bin"))
    pts = formats.read_points3d_binary(os.path.join(root, "sparse", "0", "points3D.bin"))
    record = formats.load_poses_bounds(os.path.join(root, "poses_bounds.npy"), img_wh=img_wh)
    sparse = formats.colmap_sparse_depth(imgs, pts, record["raw_bounds"], img_wh=img_wh, factor=2.0)
    N = len(sparse)
    rs = np.random.RandomState(2)
    frames, dpt = rs.randint(0, 256, (N, 24, 32, 3)).astype(np.uint8), rs.rand(N, 24, 32).astype(np.float32)
    ds = DeviceScene.from_records(record, sparse, frames, dpt, device="cpu")
    assert (ds.N, ds.H, ds.W) == (N, 24, 32) and ds.depths_h.shape == (N, 24, 32) and not ds.depths_h.any()
    assert ds.offsets == np.concatenate([[0], np.cumsum([len(s["depth"]) for s in sparse])]).tolist() and ds.offsets[-1] > 0
    sc = {"poses": record["poses"], "focal": record["focal"], "bounds": record["bounds"], "sparse": sparse, "frames": frames, "dpt": dpt,
          "depths_h": np.zeros((N, 24, 32), np.float32), "img_wh": img_wh}
    r = SC.reference_sample(sc, 2, [0, 4])
    a = ds.offsets[2]
    n = r["rays_depth"].shape[1]
    assert n == ds.n_keypoints(2) and _equal(ds.kp_weight[a:a + n], r["rays_depth"][0, :, 1, 0]) and _equal(ds.kp_depth[a:a + n], r["rays_depth"][0, :, 0, 0])
    assert _equal(ds.affine[4], r["affine_mat"][0, 2]) and _equal(ds.affine_inv[0], r["affine_mat_inv"][0, 1]) and _equal(ds.weight_img[2], r["sparse_depths_weight"][0])
    assert ds.near_far == tuple(r["near_fars"][0, 0, 0].tolist())
    val = ds.metas("val", 3)
    assert [t for t, _ in val] == [0, 2, 4] and all(set(s) <= {1, 3} for _, s in val)


def test_argument_checks_return_einval_without_a_device():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib as L
    lib = L.lib()
    assert lib.ucnerf_sample_assemble(None, None) == -1 and b"null params" in lib.ucnerf_last_error()

    def good():
        p = L.SampleAssembleParams()
        p.N, p.H, p.W, p.V, p.h1, p.w1, p.h2, p.w2, p.frame_stride = 4, 8, 12, 2, 2, 3, 4, 6, 288
        p.kp_total, p.kp_first, p.n_kp, p.n_rows = 40, 10, 20, 20
        p.view_ids[0], p.view_ids[1] = 1, 3
        for name, tp in p._fields_:
            if tp is L.vp:
                setattr(p, name, 64)               # non-null dummies, never dereferenced: validation fails first
        return p

    def refused(p, word):
        rc = lib.ucnerf_sample_assemble(C.addressof(p), None)
        return rc == -1 and word in lib.ucnerf_last_error()

    for field in ("N", "H", "W", "V", "h1", "w2", "frame_stride", "kp_total", "kp_first", "n_kp", "n_rows"):
        p = good()
        setattr(p, field, -1)
        assert refused(p, b"negative"), field
    for V in (0, 10):
        p = good()
        p.V = V
        assert refused(p, b"outside 1..9")
    for bad in (-1, 4):
        p = good()
        p.view_ids[1] = bad
        assert refused(p, b"view_ids[1]")
    p = good()
    p.view_ids[5] = 99                                 # beyond V: not looked at
    p.n_rows = 21
    assert refused(p, b"above n_kp")
    p = good()
    p.n_kp, p.n_rows, p.kp_total, p.kp_first = 2000, 1025, 4000, 0
    assert refused(p, b"above 1024")
    p = good()
    p.kp_first = 21
    assert refused(p, b"overrun")
    p = good()
    p.frame_stride = 290
    assert refused(p, b"multiple of 4")
    p.frame_stride = 284
    assert refused(p, b"multiple of 4")
    p = good()
    p.h1 = 9
    assert refused(p, b"larger than")
    for name in ("frames", "weight_img", "ref_proj_inv", "row1", "col2", "sd2", "wt1", "kp_coord", "perm", "rays_depth", "images", "proj_mats", "view_ids_out"):
        p = good()
        setattr(p, name, 0)
        assert refused(p, b"null"), name
    p = good()
    p.frames = 66
    assert refused(p, b"aligned")
    p = good()
    p.H, p.W, p.frame_stride = 1 << 13, 1 << 12, 1 << 30
    assert refused(p, b"2^24")
    # the Python wrapper refuses what it can see before the library is asked
    from uc_nerf_amd import ops
    _, ds = _host_scene("c5x7")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.sample_assemble(ds, [0, 1], None, 0)
