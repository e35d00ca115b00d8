"""Host-side checks of free-camera rendering: `data.paths.interp_path`, the float64 restatement of tests/novel_cases.py against the reference's
own route (`frame_matrices`: float32 torch.inverse / np.linalg.inv; `formats.get_nearest_pose_ids`) on dataset poses -- this pins the oracle the
kernel is compared with to the reference before the kernel is looked at --, and the surface of `ops.novel_assemble`.  No GPU."""
import ast
import os
import pkgutil

import numpy as np
import pytest

import novel_cases as NC
from uc_nerf_amd.data import paths
from uc_nerf_amd.data.formats import get_nearest_pose_ids
from uc_nerf_amd.data.scene import frame_matrices


def keyframes(K, seed):
    """float64 keyframes whose rotation blocks are orthonormal to float64 rounding (a keyframe is copied as given, so this is the input's job)."""
    import sample_cases as SC
    rs = np.random.RandomState(seed)
    return np.stack([np.concatenate([SC._rotation(rs), rs.uniform(-0.5, 0.5, (3, 1))], 1) for _ in range(K)])


# ------------------------------------------------------------------------------------------------ interp_path
@pytest.mark.parametrize("K,n", [(2, 5), (3, 9), (4, 10), (4, 7), (5, 3)])
def test_interp_path_endpoints_keyframes_and_orthonormal_rotations(K, n):
    keys = keyframes(K, 5 + K)
    out = paths.interp_path(keys, n)
    assert out.shape == (n, 3, 4) and out.dtype == np.float64
    assert np.array_equal(out[0], keys[0]) and np.array_equal(out[-1], keys[-1])
    if (n - 1) % (K - 1) == 0:
        step = (n - 1) // (K - 1)
        assert np.array_equal(out[::step], keys)                                  # every interior keyframe, exactly
    for p in out:
        R = p[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).sum(1).max() <= 1e-12                   # the infinity norm of R^T R - I
    # translations are linear within a segment: pose j of a two-keyframe path
    two = paths.interp_path(keys[:2], 5)
    assert np.allclose(two[:, :, 3], keys[0, :, 3] + np.linspace(0, 1, 5)[:, None] * (keys[1, :, 3] - keys[0, :, 3]), rtol=0, atol=1e-15)


def test_interp_path_takes_the_shorter_arc():
    q = paths.quat_from_matrix(keyframes(1, 3)[0, :, :3])
    for t in (0.0, 0.3, 0.5, 1.0):                                                # q and -q are one rotation: nothing to turn through
        got = paths.slerp(q, -q, t)
        assert np.allclose(got, q, atol=1e-15) or np.allclose(got, -q, atol=1e-15)
    # two keyframes whose quaternions come out of the conversion with opposite signs: rotations about z by -100 degrees (positive trace: w > 0)
    # and by -130 degrees (the pivot branch: z > 0, w < 0).  The shorter arc passes through -115 degrees, the longer one through +65.
    def rz(deg):
        a = np.deg2rad(deg)
        return np.array([[np.cos(a), -np.sin(a), 0, 0.0], [np.sin(a), np.cos(a), 0, 0.0], [0, 0, 1, 0.0]])
    keys = np.stack([rz(-100.0), rz(-130.0)])
    assert np.dot(paths.quat_from_matrix(keys[0][:, :3]), paths.quat_from_matrix(keys[1][:, :3])) < 0
    mid = paths.interp_path(keys, 3)[1]
    assert np.allclose(mid[:, :3], rz(-115.0)[:, :3], atol=1e-12)
    # the same rotation twice, fed to slerp with opposite signs through a path: a constant rotation
    same = paths.interp_path(np.stack([keys[0], keys[0]]), 4)
    assert all(np.allclose(p[:, :3], keys[0][:, :3], atol=1e-12) for p in same)


def test_interp_path_degenerate_sizes():
    keys = keyframes(3, 9)
    one = paths.interp_path(keys, 1)                                              # n = 1: the first keyframe alone
    assert one.shape == (1, 3, 4) and np.array_equal(one[0], keys[0])
    rep = paths.interp_path(keys[:1], 4)                                          # K = 1: n copies of the keyframe
    assert rep.shape == (4, 3, 4) and all(np.array_equal(p, keys[0]) for p in rep)
    assert paths.interp_path(keys[:1], 1).shape == (1, 3, 4)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            paths.interp_path(keys, bad)
    with pytest.raises(ValueError):
        paths.interp_path(np.zeros((0, 3, 4)), 3)
    with pytest.raises(ValueError):
        paths.interp_path(np.zeros((3, 4, 4)), 3)


# ------------------------------------------------------------------------------------------------ the restatement against the reference's route
def _inverse_bar(A64):
    """Forward error bound of a float32 LU inverse with partial pivoting of the n x n matrix A (Higham, Accuracy and Stability, ch. 14:
    |X - A^-1| <~ c n u kappa(A) |A^-1| in norm): 8 n u kappa_inf(A) max|A^-1| with n = 4 and c = 8 for the two triangular solves and the
    rounding of A's own float32 entries."""
    inv = np.linalg.inv(A64)
    kappa = np.abs(A64).sum(1).max() * np.abs(inv).sum(1).max()
    return 8 * 4 * NC.U * kappa * np.abs(inv).max()


@pytest.mark.parametrize("name", sorted(NC.SCENES))
def test_restatement_agrees_with_frame_matrices_on_dataset_poses(name):
    sc = NC.scene(name)
    K = NC.scene_intrinsic(sc)
    worst = {}
    for f, pose in enumerate(sc["poses"]):
        c2w, w2c, intrinsic, aff, aff_inv, ref_proj_inv = frame_matrices(pose, sc["focal"], sc["img_wh"])
        ref = NC.novel_matrices(pose.astype(np.float32), K)
        assert np.array_equal(intrinsic, K) and np.array_equal(c2w.astype(np.float64), ref["c2w"])
        bar = _inverse_bar(ref["c2w"])
        err = np.abs(w2c - ref["w2c"]).max()
        worst["w2c"] = max(worst.get("w2c", 0), err / bar)
        assert err <= bar, (f, err, bar)
        for s in range(3):
            # the reference's stage matrix is a float32 product K_s @ w2c of its float32 (LU) w2c: the product's gamma_3 bound plus |K_s| times w2c's own bar
            Ks = K.astype(np.float64).copy()
            Ks[:2] /= 2 ** (2 - s)
            pbar = NC.gamma(3) * (np.abs(Ks) @ np.abs(ref["w2c"][:3])) + np.abs(Ks).sum(1, keepdims=True) * bar
            perr = np.abs(aff[s][:3] - ref["affine"][s][:3])
            assert (perr <= pbar).all(), (f, s, perr.max())
            ibar = _inverse_bar(ref["affine"][s]) + np.abs(np.linalg.inv(ref["affine"][s])).max() ** 2 * pbar.max() * 4      # + the perturbation of A itself, first order: |A^-1| |dA| |A^-1|
            ierr = np.abs(aff_inv[s] - ref["affine_inv"][s]).max()
            worst["affine_inv"] = max(worst.get("affine_inv", 0), ierr / ibar)
            assert ierr <= ibar, (f, s, ierr, ibar)
            # the restated inverse is c2w . diag(K_s^-1, 1): the EXACT inverse of diag(K_s, 1) . c2w^-1 with c2w's true inverse.  (Against the
            # restated stage matrix, built on the rigid formula, it is off by the float32 pose's distance from orthonormal, about 1e-7.)
            K4 = np.eye(4)
            K4[:3, :3] = Ks
            assert np.allclose(K4 @ np.linalg.inv(ref["c2w"]) @ ref["affine_inv"][s], np.eye(4), rtol=0, atol=1e-12)
            assert np.allclose(ref["affine"][s] @ ref["affine_inv"][s], np.eye(4), rtol=0, atol=1e-5)
    print("largest error / bar of the reference's float32 route against the restatement:", worst)


@pytest.mark.parametrize("name", sorted(NC.SCENES))
def test_restated_selection_is_get_nearest_pose_ids(name):
    sc = NC.scene(name)
    N = len(sc["poses"])
    train = np.arange(N)[1::2]
    centres = sc["poses"][:, :, 3].astype(np.float32)
    for f in range(0, N, 2):
        for n_src in range(1, len(train)):                                       # (get_nearest_pose_ids caps at len - 1)
            want = train[get_nearest_pose_ids(sc["poses"][f], sc["poses"][train], n_src)]
            got, d = NC.select(centres[f], centres, train, n_src)
            assert NC.well_separated(d)
            assert got.tolist() == want.tolist(), (f, n_src)


def test_restated_selection_is_stable_and_sorts_nan_last():
    centres = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0.5, 0, 0], [np.nan, 0, 0]], dtype=np.float32)
    got, d = NC.select(np.zeros(3, np.float32), centres, [5, 2, 1, 3, 4, 0], 6)
    assert got.tolist() == [0, 4, 2, 1, 5, 3] and NC.well_separated(d)
    assert not NC.well_separated(np.array([1.0, 1.00001, 3.0]))


# ------------------------------------------------------------------------------------------------ the surface
def test_novel_assemble_resolves_and_has_one_home():
    from uc_nerf_amd import ops
    assert callable(ops.novel_assemble) and ops.novel_assemble.__module__ == "uc_nerf_amd.ops.data" and ops.novel_assemble is ops.data.novel_assemble
    homes = []
    for m in pkgutil.iter_modules(ops.__path__):
        with open(os.path.join(ops.__path__[0], m.name + ".py")) as f:
            tree = ast.parse(f.read())
        homes += [m.name for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "novel_assemble"]
    assert homes == ["data"]
    from uc_nerf_amd import _lib as L
    assert "ucnerf_novel_assemble" in L.SYMBOLS and L.ADDED_STRUCTS["ucnerf_novel_assemble_params"] is L.NovelAssembleParams
    from uc_nerf_amd.data import DeviceScene
    from uc_nerf_amd.system import UCNeRFSystem
    from uc_nerf_amd.validate import render_novel_view
    assert callable(DeviceScene.sample_pose) and callable(UCNeRFSystem.render_path) and callable(render_novel_view)
