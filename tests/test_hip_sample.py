"""ucnerf_sample_assemble through DeviceScene.sample on the device against the host restatement of the reference's sample assembly
(tests/sample_cases.py): bit for bit wherever nothing but roundings the reference also makes is involved, proj_mats within the bound of a
four-term float32 dot product."""
import numpy as np
import pytest
import torch

import sample_cases as SC

pytestmark = pytest.mark.gpu

_dev_scenes, _refs = {}, {}


def dev_scene(name):
    from uc_nerf_amd.data import DeviceScene
    if name not in _dev_scenes:
        sc = SC.scene(name)
        _dev_scenes[name] = DeviceScene.from_arrays(sc["poses"], sc["focal"], sc["bounds"], sc["sparse"], sc["frames"], sc["dpt"], sc["depths_h"],
                                                    sc["img_wh"], device="cuda")
    return _dev_scenes[name]


def reference(name, target, src):
    key = (name, target, tuple(src))
    if key not in _refs:
        _refs[key] = SC.reference_sample(SC.scene(name), target, src, perm=SC.case_perm(name, target))
    return _refs[key]


def perm_tensor(name, target):
    return torch.from_numpy(SC.case_perm(name, target).astype(np.int32)).cuda()


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("name,target,src", SC.CASES, ids=SC.CASE_IDS)
@pytest.mark.parametrize("unpre", [False, True], ids=["plain", "unpre"])
def test_sample_equals_the_restatement(name, target, src, unpre):
    ds, ref = dev_scene(name), reference(name, target, src)
    n_kp = ds.n_keypoints(target)
    got = ds.sample(target, src, perm=perm_tensor(name, target) if n_kp else None, unpreprocess=unpre)
    assert set(got) == (set(ref) - {"_ref_proj_inv"} - (set() if unpre else {"images_unpre"}))
    V = 1 + len(src)
    assert got["rays_depth"].shape == (1, min(n_kp, 1024), 3, 3) and got["images"].shape == (1, V, 3, ds.H, ds.W)
    for key in ("images", "depths_h", "dpt", "sparse_depths", "sparse_depths_weight", "rays_depth", "w2cs", "c2ws", "near_fars", "intrinsics",
                "view_ids", "affine_mat", "affine_mat_inv", "scan") + (("images_unpre",) if unpre else ()):
        assert got[key].is_cuda and same_bits(got[key], ref[key]), key
    for key in ("sparse_depths_ms", "weight_ms"):
        assert set(got[key]) == {"stage1", "stage2", "stage3"}
        for lvl in got[key]:
            assert same_bits(got[key][lvl], ref[key][lvl]), (key, lvl)
    # proj_mats: identity rows for the target; elsewhere a four-term float32 dot product against the float64 product of the same float32 inputs
    pm = got["proj_mats"].cpu()
    assert pm.shape == (1, V, 3, 4) and torch.equal(pm[0, 0], torch.eye(4)[:3])
    a = ref["affine_mat"][0, :, 2].double()                                   # [V,4,4]
    b = ref["_ref_proj_inv"].double()
    exact = (a @ b)[:, :3]
    bound = 4 * 2.0 ** -24 * (a.abs() @ b.abs())[:, :3]
    err = (pm[0].double() - exact).abs()
    print("proj_mats: max error %.3e, max error / bound %.3f" % (err[1:].max().item() if V > 1 else 0.0,
                                                                  (err[1:] / bound[1:]).max().item() if V > 1 else 0.0))
    assert (err[1:] <= bound[1:]).all()
    # ... and the restatement's own torch.matmul sits inside the same bound (the two differ by summation order only)
    assert ((ref["proj_mats"][0, 1:].double() - exact[1:]).abs() <= bound[1:]).all()


def test_default_perm_is_a_permutation_of_the_full_list():
    ds, sc = dev_scene("b10x14"), SC.scene("b10x14")
    n = len(sc["sparse"][0]["depth"])
    assert n == 1030
    # all 1030 rows of the list (the restatement cuts at 1024: the last six come from a second call); random depths make them distinct
    rows = torch.cat([SC.reference_sample(sc, 0, [1])["rays_depth"][0], SC.reference_sample(sc, 0, [1], perm=np.arange(1024, n))["rays_depth"][0]])
    rows = rows.reshape(n, 9)
    assert torch.unique(rows, dim=0).shape[0] == n
    torch.manual_seed(0)
    a = ds.sample(0, [1])["rays_depth"].cpu().reshape(-1, 9)
    b = ds.sample(0, [1])["rays_depth"].cpu().reshape(-1, 9)
    assert a.shape == (1024, 9) and not torch.equal(a, b)
    for got in (a, b):
        hit = (got[:, None, :] == rows[None]).all(-1)                             # [1024,1030]: drawn row i is list row j
        assert (hit.sum(1) == 1).all() and torch.unique(hit.int().argmax(1)).numel() == 1024
    small = ds.sample(1, [0])["rays_depth"]                                       # 3 keypoints, equal weights: NaN, still one row per keypoint
    assert small.shape == (1, 3, 3, 3) and sorted(small[0, :, 2, :2].cpu().tolist()) == sorted(sc["sparse"][1]["coord"].astype(float).tolist())
    assert ds.sample(2, [0])["rays_depth"].shape == (1, 0, 3, 3)


def test_two_samples_of_one_scene_do_not_disturb_each_other():
    ds = dev_scene("a8x12")
    first = ds.sample(1, [2], perm=perm_tensor("a8x12", 1), unpreprocess=True)
    keep = {k: v.clone() for k, v in first.items() if torch.is_tensor(v)}
    second = ds.sample(3, [0, 1, 2, 3, 0, 1, 2, 3], perm=perm_tensor("a8x12", 3), unpreprocess=True)
    torch.cuda.synchronize()
    assert all(torch.equal(torch.nan_to_num(first[k]), torch.nan_to_num(keep[k])) for k in keep)
    ref = reference("a8x12", 3, [0, 1, 2, 3, 0, 1, 2, 3])
    assert same_bits(second["images"], ref["images"]) and same_bits(second["rays_depth"], ref["rays_depth"])
    assert second["images"].data_ptr() != first["images"].data_ptr()


def test_documented_views_alias_the_resident_storage():
    ds = dev_scene("a8x12")
    s = ds.sample(1, [2], perm=perm_tensor("a8x12", 1))
    hw = ds.H * ds.W * 4
    assert s["dpt"].data_ptr() == ds.dpt.data_ptr() + hw and s["depths_h"].data_ptr() == ds.depths_h.data_ptr() + hw
    assert s["sparse_depths"].data_ptr() == ds.depth_img.data_ptr() + hw == s["sparse_depths_ms"]["stage3"].data_ptr()
    assert s["sparse_depths_weight"].data_ptr() == ds.weight_img.data_ptr() + hw == s["weight_ms"]["stage3"].data_ptr()
    assert s["scan"].data_ptr() == ds.scan.data_ptr()
    lo, hi = ds.frames.data_ptr(), ds.frames.data_ptr() + ds.frames.numel()
    assert not lo <= s["images"].data_ptr() < hi and s["sparse_depths_ms"]["stage1"].data_ptr() != ds.depth_img.data_ptr()


def test_sample_goes_through_the_training_steps_indexing_on_the_device():
    """utils.sub_selete_data and train.py:110-134's indexing on a sample: every tensor stays on the device, shapes as the step expects."""
    from uc_nerf_amd.utils.utils import sub_selete_data
    ds = dev_scene("b10x14")
    batch = ds.sample(3, [0, 1, 2], perm=perm_tensor("b10x14", 3))
    depth_sparse_ms, weight_ms = batch["sparse_depths_ms"], batch["weight_ms"]
    for k in ("scan", "sparse_depths_ms", "weight_ms"):
        batch.pop(k)
    data_mvs = sub_selete_data(batch, batch["images"].device, None, filtKey=[])
    pose_ref = {k: data_mvs[k].squeeze() for k in ("w2cs", "intrinsics", "c2ws", "near_fars")}
    imgs, near_fars = data_mvs["images"], pose_ref["near_fars"]
    batch_depth = torch.transpose(data_mvs["rays_depth"].squeeze(0), 0, 1)
    target_depths, target_weights, depth_coord = batch_depth[0, :, 0], batch_depth[1, :, 0], batch_depth[2, :, 0:2]
    affine_mat, affine_mat_inv = data_mvs["affine_mat"][0], data_mvs["affine_mat_inv"][0]
    imgs_input = imgs[:, 1:]
    every = [imgs, near_fars, data_mvs["dpt"], data_mvs["sparse_depths"], data_mvs["sparse_depths_weight"], target_depths, target_weights, depth_coord,
             affine_mat, affine_mat_inv, imgs_input, *pose_ref.values(), *depth_sparse_ms.values(), *weight_ms.values()]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in every)
    assert imgs_input.shape == (1, 3, 3, 10, 14) and near_fars.shape == (4, 2) and pose_ref["w2cs"].shape == (4, 4, 4) and affine_mat.shape == (4, 3, 4, 4)
    assert target_depths.shape == (1024,) and depth_coord.shape == (1024, 2) and depth_sparse_ms["stage1"].shape == (1, 2, 3)
    ref = reference("b10x14", 3, [0, 1, 2, 3])
    assert torch.equal(target_depths.cpu(), ref["rays_depth"][0, :, 0, 0]) and torch.equal(depth_coord.cpu(), ref["rays_depth"][0, :, 2, :2])
