"""Free-camera rendering on the device: ucnerf_novel_assemble through `DeviceScene.sample_pose` against the float64 restatement of
tests/novel_cases.py (pinned to the reference's route by tests/test_novel_host.py), against `DeviceScene.sample` where the pose is a dataset
frame's, its source-view selection, its padding and error codes; then `UCNeRFSystem.render_path` on the tiny system of tests/system_cases.py.

No case here provokes a fault.  Read in csrc/novel.hip: every candidate id is clamped into 0 .. N-1 before it indexes a resident array, the
dwords of a frame are read only below 3 H W (inside frame_stride), cand is read below n_cand <= 4096 (the LDS array's size), poses at
pose_index < P (checked on the host), and every store is bounded by V, H W and the segment sizes the wrapper carves.

Bars.  Copies are bit-exact.  A k-term float32 dot product accumulated with fmaf carries at most gamma_k sum|a_i||b_i|, gamma_k = k u / (1 - k u),
u = 2^-24 (fmaf rounds once a term, so k roundings).  affine_mat[0] is checked twice: against the float64 product of the float32 operands the
kernel multiplies (K_s and its own w2cs[0]; bar gamma_3 sum|a||b|) and against the whole float64 chain from the pose (that bar plus |K_s| times
the bar of w2c's translation).  affine_mat_inv[0] and proj_mats[v > 0] have no bar fixed in advance: the error of the reference's own float32
route (`frame_matrices`: torch.inverse, np.linalg.inv, torch's matmul) against the same float64 values is measured on the same poses here, and
the kernel is allowed four times the largest.  Measured figures: profiles/novel_path.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import novel_cases as NC
import system_cases as YC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
POISON = 0x7FC0DEAD       # a NaN with a payload, as int32
_cache = {}


def dev_scene(name):
    if name not in _cache:
        _cache[name] = NC.device_scene(name, DEV)
    return _cache[name]


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def centres_of(ds):
    return ds.c2w.cpu().numpy().reshape(-1, 4, 4)[:, :3, 3]


# ------------------------------------------------------------------------------------------------ 1. matrices
@pytest.mark.parametrize("name,V,own_K", [("n15x21", 3, False), ("n15x21", 9, True), ("n16x20", 3, True)], ids=["n15x21-V3", "n15x21-V9-K", "n16x20-V3-K"])
def test_target_matrices_against_the_float64_restatement(name, V, own_K):
    from uc_nerf_amd.data.scene import frame_matrices
    ds, sc = dev_scene(name), NC.scene(name)
    W, H = sc["img_wh"]
    # an intrinsic of its own in the form frame_matrices can state: focal (fx, fy), principal point (w / 2, h / 2)
    focal, wh = ((1.3 * W, 0.8 * H), (W + 3, H - 1)) if own_K else (sc["focal"], (W, H))
    K = np.array([[focal[0], 0, wh[0] / 2], [0, focal[1], wh[1] / 2], [0, 0, 1]], dtype=np.float32)
    poses = NC.free_poses(4, 17)
    cand = np.arange(ds.N)[1::2]
    poses_d, cand_d, K_d = up(poses, np.float32), up(cand, np.int32), up(K, np.float32)
    centres = centres_of(ds)
    worst = {"w2c_t": 0.0, "affine": 0.0, "affine_chain": 0.0}
    kernel_err, route_err = {"affine_inv": 0.0, "proj": 0.0}, {"affine_inv": 0.0, "proj": 0.0}
    g3 = NC.gamma(3)
    for i, pose in enumerate(poses):
        out = ds.sample_pose(poses_d, i, V, candidates=cand_d, intrinsic=K_d if own_K else None)
        ref = NC.novel_matrices(pose, K)
        got = {k: out[k][0].cpu().numpy() for k in ("c2ws", "w2cs", "intrinsics", "affine_mat", "affine_mat_inv", "proj_mats")}
        # copies
        assert np.array_equal(got["c2ws"][0], ref["c2w"].astype(np.float32)) and np.array_equal(got["intrinsics"][0], K)
        assert np.array_equal(got["proj_mats"][0], np.eye(4, dtype=np.float32)[:3])
        w2c = got["w2cs"][0]
        assert np.array_equal(w2c[:3, :3], pose[:, :3].T) and np.array_equal(w2c[3], [0, 0, 0, 1])
        # the translation: three terms
        R64, t64 = pose[:, :3].astype(np.float64), pose[:, 3].astype(np.float64)
        bar_t = g3 * (np.abs(R64.T) @ np.abs(t64))
        err_t = np.abs(w2c[:3, 3] - ref["w2c"][:3, 3])
        worst["w2c_t"] = max(worst["w2c_t"], (err_t / bar_t).max())
        assert (err_t <= bar_t).all(), (i, err_t, bar_t)
        for s in range(3):
            Ks = K.astype(np.float64).copy()
            Ks[:2] /= 2 ** (2 - s)
            a = got["affine_mat"][0, s]
            assert np.array_equal(a[3], [0, 0, 0, 1])
            w64 = w2c[:3].astype(np.float64)                                       # the float32 operand the kernel multiplies
            bar = g3 * (np.abs(Ks) @ np.abs(w64))
            err = np.abs(a[:3] - Ks @ w64)
            worst["affine"] = max(worst["affine"], (err / np.maximum(bar, 1e-300)).max())
            assert (err <= bar).all(), (i, s, err.max())
            bar_chain = bar + np.abs(Ks) @ np.concatenate([np.zeros((3, 3)), bar_t[:, None]], 1)      # + |K_s| times what the operand itself may be off by
            err_chain = np.abs(a[:3] - ref["affine"][s][:3])
            worst["affine_chain"] = max(worst["affine_chain"], (err_chain / np.maximum(bar_chain, 1e-300)).max())
            assert (err_chain <= bar_chain).all(), (i, s, err_chain.max())
        # the reference's float32 route on the same pose, against the same float64 values
        fm = frame_matrices(pose.astype(np.float64), focal, wh)
        assert np.array_equal(fm[2], K)
        kernel_err["affine_inv"] = max(kernel_err["affine_inv"], np.abs(got["affine_mat_inv"][0] - ref["affine_inv"]).max())
        route_err["affine_inv"] = max(route_err["affine_inv"], np.abs(fm[4] - ref["affine_inv"]).max())
        src, d = NC.select(pose[:, 3], centres, cand, V - 1)
        assert NC.well_separated(d)
        assert out["view_ids"][0].cpu().tolist() == [-1] + src.tolist()
        aff_src = ds.affine.cpu().numpy().reshape(-1, 3, 4, 4)[src, 2]             # the resident float32 stage-3 matrices of the sources
        exact = (aff_src.astype(np.float64) @ ref["affine_inv"][2])[:, :3]
        route = (torch.from_numpy(aff_src) @ torch.from_numpy(fm[5])).numpy()[:, :3]        # proj_mat_l @ ref_proj_inv, torch's float32 matmul
        kernel_err["proj"] = max(kernel_err["proj"], np.abs(got["proj_mats"][1:] - exact).max())
        route_err["proj"] = max(route_err["proj"], np.abs(route - exact).max())
    print("largest error / derived bar: %s" % worst)
    print("affine_mat_inv[0]: kernel %.3e, the reference's float32 route %.3e;  proj_mats[v>0]: kernel %.3e, route %.3e  (max abs error against float64)"
          % (kernel_err["affine_inv"], route_err["affine_inv"], kernel_err["proj"], route_err["proj"]))
    assert kernel_err["affine_inv"] <= 4 * route_err["affine_inv"]
    assert kernel_err["proj"] <= 4 * route_err["proj"]


# ------------------------------------------------------------------------------------------------ 2. a pose that is a dataset frame's
@pytest.mark.parametrize("name,V", [("n15x21", 3), ("n15x21", 9), ("n16x20", 3), ("n40x52", 3)])
def test_pose_of_a_dataset_frame_gives_the_samples_source_slots(name, V):
    """The candidates are f's sources from metas("val") at V + 1 views: V frames, the least the entry point takes (n_cand >= V); their V - 1
    nearest are f's sources at V views, which `sample` is called with."""
    ds, sc = dev_scene(name), NC.scene(name)
    poses_d = up(sc["poses"].astype(np.float32), np.float32)
    metas, wide = ds.metas("val", V), ds.metas("val", V + 1)
    for (f, src), (f2, cand) in list(zip(metas, wide))[:3]:
        assert f == f2 and len(cand) == V and len(src) == V - 1 and cand[:V - 1] == src
        assert NC.well_separated(NC.distances(sc["poses"][f][:, 3], centres_of(ds), cand))
        got = ds.sample_pose(poses_d, f, V, candidates=cand, unpreprocess=True)
        want = ds.sample(f, src, perm=torch.arange(ds.n_keypoints(f), dtype=torch.int32, device=DEV), unpreprocess=True)
        assert got["view_ids"][0, 1:].cpu().tolist() == src and int(got["view_ids"][0, 0]) == -1
        for key in ("images", "images_unpre", "c2ws", "w2cs", "intrinsics", "affine_mat", "affine_mat_inv", "near_fars"):
            assert got[key].shape == want[key].shape and same_bits(got[key][:, :, 1:] if key == "near_fars" else got[key][:, 1:],
                                                                   want[key][:, :, 1:] if key == "near_fars" else want[key][:, 1:]), key
        assert same_bits(got["near_fars"], want["near_fars"]) and same_bits(got["c2ws"][:, 0], want["c2ws"][:, 0])
        assert got["scan"].data_ptr() == ds.scan.data_ptr()
        assert set(got) == {"images", "images_unpre", "c2ws", "w2cs", "intrinsics", "affine_mat", "affine_mat_inv", "proj_mats", "near_fars", "view_ids", "scan"}
        assert not bool(got["images"][:, 0].any()) and not bool(got["images_unpre"][:, 0].any())
        plain = ds.sample_pose(poses_d, f, V, candidates=cand)
        assert "images_unpre" not in plain and same_bits(plain["images"], got["images"])


# ------------------------------------------------------------------------------------------------ 3. selection
def _ids(ds, poses_d, i, V, cand):
    return ds.sample_pose(poses_d, i, V, candidates=cand)["view_ids"][0].cpu().tolist()


def test_selection_is_the_stable_argsort_of_the_float64_distances():
    ds = dev_scene("n15x21")
    centres = centres_of(ds)
    poses = NC.free_poses(6, 23)
    poses_d = up(poses, np.float32)
    rs = np.random.RandomState(3)
    lists = {"train": np.arange(ds.N)[1::2], "all-but-a-twin": np.array([k for k in range(ds.N) if k != 12]),
             "descending": np.array([k for k in range(ds.N) if k != 12])[::-1], "shuffled": rs.permutation(np.arange(ds.N)[:11])}
    for label, cand in lists.items():
        cand_d = up(cand, np.int32)
        for i, pose in enumerate(poses):
            for V in (2, 3, 9):
                want, d = NC.select(pose[:, 3], centres, cand, V - 1)
                assert NC.well_separated(d), (label, i)                            # a condition on the inputs: float32 rounding cannot reorder them
                assert _ids(ds, poses_d, i, V, cand_d) == [-1] + want.tolist(), (label, i, V)


def test_selection_edge_cases():
    ds, sc = dev_scene("n15x21"), NC.scene("n15x21")
    centres = centres_of(ds)
    assert np.array_equal(centres[4], centres[12])
    poses = np.concatenate([sc["poses"][4:5].astype(np.float32), NC.free_poses(2, 29)])
    poses_d = up(poses, np.float32)
    # two candidates with the identical pose (distance 0 from pose 0): the lower position first, whichever frame id sits there
    for cand in ([1, 12, 3, 4, 5], [1, 4, 3, 12, 5]):
        want, d = NC.select(poses[0][:, 3], centres, cand, 2)
        assert want.tolist() == [cand[1], cand[3]] and NC.well_separated(d)
        assert _ids(ds, poses_d, 0, 3, cand) == [-1] + want.tolist()
    # n_cand == V
    cand = [9, 2, 17]
    want, d = NC.select(poses[1][:, 3], centres, cand, 2)
    assert NC.well_separated(d) and _ids(ds, poses_d, 1, 3, cand) == [-1] + want.tolist()
    # n_cand = 4096 with repeated ids: the cap; equal distances resolve by position, so the first occurrences win
    cand = np.resize(np.array([k for k in range(ds.N) if k != 12])[::-1], 4096)
    want, d = NC.select(poses[2][:, 3], centres, cand, 8)
    assert NC.well_separated(d) and len(set(want.tolist())) == 1                    # the nearest frame, eight times over
    assert _ids(ds, poses_d, 2, 9, cand) == [-1] + want.tolist()
    want3, _ = NC.select(poses[2][:, 3], centres, cand[:19], 8)
    assert len(set(want3.tolist())) == 8 and _ids(ds, poses_d, 2, 9, cand[:19]) == [-1] + want3.tolist()
    # a candidate whose centre is NaN sorts last: never picked while a number is left, picked (by position) when none is
    twin = NC.device_scene("n15x21", DEV)                                           # (a scene of its own: the resident c2w is written)
    twin.c2w[7, 0, 3] = float("nan")
    twin.c2w[9, 2, 3] = float("nan")
    cen = centres_of(twin)
    cand = [9, 7, 1, 3, 9]                                                          # three NaN positions, two numbers
    want, d = NC.select(poses[1][:, 3], cen, cand, 2)
    assert np.isnan(d[:2]).all() and NC.well_separated(d) and not {7, 9} & set(want.tolist())
    assert _ids(twin, poses_d, 1, 3, cand) == [-1] + want.tolist()
    want, d = NC.select(poses[1][:, 3], cen, cand, 4)
    assert want.tolist()[2:] == [9, 7]
    assert _ids(twin, poses_d, 1, 5, cand) == [-1] + want.tolist()
    # an id outside 0 .. N-1 is clamped into the range (documented: the list is on the device)
    assert _ids(ds, poses_d, 1, 3, [-5, 1000, 3])[1:] in ([0, 19], [19, 0], [0, 3], [3, 0], [19, 3], [3, 19])


# ------------------------------------------------------------------------------------------------ 4. padding and error codes
def raw_call(ds, poses_d, index, cand_d, V, unpre=True, guard=64, **over):
    """The entry point on a poisoned allocation of the wrapper's own layout.  -> (return code, message, buffer as int32, offsets, sizes, total)."""
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.ops import data as D
    base = D._novel_params(ds)
    p = L.NovelAssembleParams.from_buffer_copy(base)
    Va = min(max(V, 1), 9)
    HW = ds.H * ds.W
    img = Va * 3 * HW
    sizes = [img, img if unpre else 0, Va * 16, Va * 16, Va * 9, Va * 48, Va * 48, Va * 12, Va * 2, Va * 2]
    offs, total = D._carve(sizes)
    buf = torch.full((total + guard,), POISON, dtype=torch.int32, device=DEV)
    p.V, p.P, p.pose_index, p.n_cand = V, poses_d.shape[0], index, cand_d.numel()
    p.poses, p.cand, p.intrinsic_in = poses_d.data_ptr(), cand_d.data_ptr(), 0
    (p.images, p.images_unpre, p.c2ws, p.w2cs, p.intrinsics, p.affine_mat, p.affine_mat_inv, p.proj_mats, p.near_fars,
     p.view_ids_out) = [buf.data_ptr() + 4 * o if n else 0 for o, n in zip(offs, sizes)]
    for k, v in over.items():
        setattr(p, k, v)
    rc = L.lib().ucnerf_novel_assemble(C.addressof(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = L.lib().ucnerf_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg, buf.cpu(), offs, sizes, total


@pytest.mark.parametrize("name,V,unpre", [("n15x21", 3, True), ("n15x21", 9, False), ("n16x20", 4, True), ("n40x52", 2, True)])
def test_every_element_is_written_and_nothing_else(name, V, unpre):
    ds = dev_scene(name)
    poses_d, cand_d = up(NC.free_poses(2, 31), np.float32), up(np.arange(ds.N), np.int32)
    rc, msg, buf, offs, sizes, total = raw_call(ds, poses_d, 1, cand_d, V, unpre=unpre)
    assert rc == 0, msg
    written = torch.zeros(total + 64, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        written[o:o + n] = True
    assert not bool((buf[written] == POISON).any())                                  # no element of a carved segment keeps the poison
    assert bool((buf[~written] == POISON).all())                                     # the alignment gaps between segments and the guard words after them
    HW = ds.H * ds.W
    assert not bool(buf[:3 * HW].any())                                              # slot 0 of images: 0.0f everywhere (+0.0: all bits clear)
    if unpre:
        assert not bool(buf[offs[1]:offs[1] + 3 * HW].any())
    assert int(buf[offs[9]:offs[9] + 2].view(torch.int64)[0]) == -1


def test_error_codes_launch_nothing():
    ds = dev_scene("n15x21")
    poses_d, cand_d = up(NC.free_poses(2, 31), np.float32), up(np.arange(ds.N), np.int32)
    big = up(np.resize(np.arange(ds.N), 4097), np.int32)
    cases = [(dict(P=0), "P = 0"), (dict(P=-1), "negative"), (dict(pose_index=-1), "pose_index = -1"), (dict(pose_index=2), "pose_index = 2"),
             (dict(n_cand=2), "n_cand = 2 candidates below V = 3"), (dict(n_cand=4097, cand=big.data_ptr()), "n_cand = 4097 candidates above 4096"),
             (dict(V=1), "V = 1 outside 2..9"), (dict(V=10, n_cand=20), "V = 10 outside 2..9"), (dict(V=-3), "negative"), (dict(n_cand=-1), "negative"),
             (dict(N=-1), "negative"), (dict(poses=0), "null poses or cand"), (dict(cand=0), "null poses or cand"), (dict(images=0), "null output")]
    for over, message in cases:
        over = dict(over)
        rc, msg, buf, offs, sizes, total = raw_call(ds, poses_d, 0, cand_d, over.pop("V", 3), **over)
        assert rc == -1 and message in msg, (over, rc, msg)
        assert bool((buf == POISON).all()), over                                     # nothing was launched: the allocation is as it was
    from uc_nerf_amd import ops
    with pytest.raises(RuntimeError, match=r"ucnerf_novel_assemble failed \(-1\).*n_cand = 2 candidates below V = 3"):
        ops.novel_assemble(ds, poses_d, 0, cand_d[:2], 3)
    with pytest.raises(RuntimeError, match=r"ucnerf_novel_assemble failed \(-1\).*pose_index = 2"):
        ds.sample_pose(poses_d, 2, 3)
    with pytest.raises(RuntimeError, match="poses must be"):
        ops.novel_assemble(ds, poses_d.double(), 0, cand_d, 3)
    with pytest.raises(RuntimeError, match="poses must be"):
        ops.novel_assemble(ds, poses_d.cpu(), 0, cand_d, 3)
    with pytest.raises(RuntimeError, match="cand must be"):
        ops.novel_assemble(ds, poses_d, 0, cand_d.long(), 3)
    with pytest.raises(RuntimeError, match="intrinsic must be"):
        ops.novel_assemble(ds, poses_d, 0, cand_d, 3, intrinsic=torch.eye(4, device=DEV))


# ------------------------------------------------------------------------------------------------ 5. render_path
def tiny():
    if "tiny" not in _cache:
        from uc_nerf_amd.system import UCNeRFSystem
        scene = YC.tiny_scene(DEV)
        torch.manual_seed(0)
        _cache["tiny"] = (UCNeRFSystem(YC.tiny_args(DEV), [scene], network_mvs=YC.tiny_mvs()), scene)
    return _cache["tiny"]


def reseed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def test_render_path_frames_are_render_novel_view_and_the_model_is_left_as_found():
    from uc_nerf_amd.data.paths import interp_path
    from uc_nerf_amd.validate import render_novel_view
    system, scene = tiny()
    keys = YC.tiny_scene_arrays()["poses"][[0, 2]]
    poses_d = up(interp_path(keys, 4)[1:3], np.float32)                              # two poses strictly between two frames
    net, mlp = system.Consist_Learner, system.render_kwargs_train["network_fn"]
    net.eval()
    for k, m in enumerate(net.modules()):                                           # a mixed pattern of flags: each one must come back, not just the root's
        m.training = k % 3 == 0
    flags = [m.training for n in (net, mlp) for m in n.modules()]
    before = [{k: v.clone() for k, v in n.state_dict().items()} for n in (net, mlp)]
    assert any(k.endswith("running_mean") for k in before[0]) and any(k.endswith("num_batches_tracked") for k in before[0])
    reseed(7)
    out = system.render_path(scene, poses_d, depth_vis=True)
    assert set(out) == {"rgb", "depth", "depth_vis"} and out["rgb"].shape == (2, 3, YC.H, YC.W) and out["depth"].shape == (2, YC.H, YC.W)
    assert out["depth_vis"].shape == (2, 3, YC.H, YC.W) and all(v.is_cuda for v in out.values())
    assert bool(torch.isfinite(out["rgb"]).all()) and float(out["rgb"].min()) >= 0.0 and float(out["rgb"].max()) <= 1.0
    assert [m.training for n in (net, mlp) for m in n.modules()] == flags
    for n, was in zip((net, mlp), before):
        now = n.state_dict()
        assert set(now) == set(was)
        for k in was:
            assert same_bits(now[k], was[k]) if was[k].dtype == torch.float32 else torch.equal(now[k], was[k]), k
    assert set(system.render_path(scene, poses_d[:1])) == {"rgb", "depth"}
    # frame j is render_novel_view on sample_pose(poses, j), in the mode validation runs the CNNs in
    reseed(7)
    net.train()
    for j in range(2):
        rgb, depth, vis = render_novel_view(system.args, scene.sample_pose(poses_d, j, system.args.view_num, unpreprocess=True), net, system.render_kwargs_train)
        assert rgb.shape == (3, YC.H, YC.W) and depth.shape == (YC.H, YC.W) and vis.shape == (3, YC.H, YC.W)
        assert torch.equal(out["rgb"][j], rgb) and torch.equal(out["depth"][j], depth) and torch.equal(out["depth_vis"][j], vis), j


def _ulp_up(t):
    """Every entry that is neither 0 nor 1 (the structural entries of the matrices) moved one float32 ulp away from zero."""
    moved = torch.nextafter(t, torch.where(t > 0, torch.full_like(t, float("inf")), torch.full_like(t, -float("inf"))))
    return torch.where((t == 0) | (t == 1), t, moved)


def test_render_path_at_a_validation_pose_agrees_with_validation_step():
    """The one input that differs from validation_step's is slot 0's matrices, in their last bits (closed forms against LAPACK's).  The bar is not
    fixed in advance: it is four times the spread between validation_step on the resident matrices and on the same matrices moved by one float32
    ulp.  Measured figures: profiles/novel_path.md."""
    system, scene = tiny()
    f, src = scene.metas("val", YC.V)[1]
    arrays = YC.tiny_scene_arrays()
    train = np.arange(scene.N)[1::2]
    assert NC.well_separated(NC.distances(arrays["poses"][f][:, 3].astype(np.float32), centres_of(scene), train))
    poses_d = up(arrays["poses"][f:f + 1], np.float32)
    assert scene.sample_pose(poses_d, 0, YC.V)["view_ids"][0, 1:].cpu().tolist() == src       # the default candidates: the training index
    reseed(13)
    out = system.render_path(scene, poses_d)
    batch = scene.sample(f, src, unpreprocess=True)
    reseed(13)
    base = system.validation_step(batch, 0)
    moved = dict(batch)
    for k in ("w2cs", "c2ws", "affine_mat", "affine_mat_inv"):
        t = batch[k].clone()
        t[:, 0] = _ulp_up(t[:, 0])
        moved[k] = t
    reseed(13)
    pert = system.validation_step(moved, 1)
    system.validation_step_outputs = []
    for key, mine in (("pred_rgb", out["rgb"][0]), ("pred_depth", out["depth"][0])):
        spread = float((pert[key] - base[key]).abs().max())
        diff = float((mine - base[key]).abs().max())
        print("%s: |render_path - validation_step| max %.3e;  one-ulp spread of validation_step %.3e;  bar %.3e" % (key, diff, spread, 4 * spread))
        assert diff <= 4 * spread, key


def test_render_path_reads_nothing_back():
    system, scene = tiny()
    poses_d = up(NC.free_poses(2, 37), np.float32)
    system.render_path(scene, poses_d, depth_vis=True)                               # warm: the cached candidates, packed weights, tables
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = system.render_path(scene, poses_d, depth_vis=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(out["depth"]).all())
