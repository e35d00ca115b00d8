"""Shared builders of the system tests (tests/test_system_host.py, tests/test_hip_step_targets.py, tests/test_hip_system.py).  CPU only: nothing
here touches a device.

`step_targets_ref` restates train.py:166-176 in numpy: sparse_depths[:, r, c] and sparse_weights[:, r, c] over the rays from n_rays on,
dpt[:, r, c] over the patch rays reshaped to [-1, ps, ps, 1], with numpy's advanced indexing (which wraps a negative index as torch does).

The coordinate sets are the smallest that hold every case of the gather: both corners, a duplicate, and the wraps -1, -H and -W, placed so
that both the patch part and the depth part of every n_total see a wrap.  The tiny scene is 32 x 32 (the smallest image the CNNs accept:
CostRegNet halves three times on the quarter-resolution stage; the shape and the ndepths [48, 32, 8] tests/test_hip_feature_views.py's cascade step uses), V = 3, six
frames, about 300 keypoints a frame.
"""
import types

import numpy as np

import sample_cases as SC

# ------------------------------------------------------------------------------------------------ the gather
# (H, W, n_rays, patch_num, patch_size, n_total): the issue's 5 x 7 maps with n_rays = 6 and patches of 2 x 2.  Two patches are 8 points,
# more than n_total = 6 or 7 (that combination is the library's UCNERF_EINVAL, tested as such), so those two run with one patch; 6 == n_rays is
# the empty depth part.  The last case holds 300 depth rays: more than one 256-thread block.
GATHER_CASES = ((5, 7, 6, 1, 2, 6), (5, 7, 6, 1, 2, 7), (5, 7, 6, 2, 2, 15), (5, 7, 6, 0, 2, 15), (37, 41, 20, 3, 2, 320))
GATHER_IDS = ["%dx%d-n%d-p%d" % (c[0], c[1], c[5], c[3]) for c in GATHER_CASES]


def gather_maps(H, W, seed):
    """Three [1,H,W] float32 maps holding NaN, +inf, -inf and -0.0 among random values (copied bit for bit by a gather)."""
    rs = np.random.RandomState(seed)
    maps = rs.randn(3, 1, H, W).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
    for m in maps:
        at = rs.permutation(H * W)[:4]
        m.reshape(-1)[at] = special
    # the corners the coordinate sets always read carry the specials too
    maps[0][0, 0, 0], maps[1][0, H - 1, W - 1], maps[2][0, 0, 0] = np.float32(-0.0), np.float32(np.nan), np.float32(np.inf)
    return maps[0], maps[1], maps[2]


def gather_coords(H, W, n_total, seed):
    """int64 [2, n_total] in-range coordinates (row, col): random, with the fixed ones cycled through every position class: (0, 0),
    (H-1, W-1), a duplicate of the previous column, (-1, -1), (-H, -W), (-H, W-1), (H-1, -W)."""
    rs = np.random.RandomState(seed)
    pix = np.stack([rs.randint(-H, H, n_total), rs.randint(-W, W, n_total)]).astype(np.int64)
    fixed = [(0, 0), (H - 1, W - 1), None, (-1, -1), (-H, -W), (-H, W - 1), (H - 1, -W)]
    for i in range(n_total):
        f = fixed[i % len(fixed)] if (i // len(fixed)) % 2 == 0 else "random"
        if f is None and i > 0:
            pix[:, i] = pix[:, i - 1]
        elif isinstance(f, tuple):
            pix[:, i] = f
    return pix


def step_targets_ref(sparse_depths, sparse_weights, dpt, pixel_coordinates, n_rays, patch_num, patch_size):
    """train.py:166-176 on numpy arrays: maps [1,H,W], pixel_coordinates [2,n_total] of whole numbers (any dtype)."""
    pix = np.asarray(pixel_coordinates).astype(np.int64)
    patch_pts = patch_num * patch_size * patch_size
    target_depths = sparse_depths[:, pix[0, n_rays:], pix[1, n_rays:]]
    target_weights = sparse_weights[:, pix[0, n_rays:], pix[1, n_rays:]]
    patch_dpt = dpt[:, pix[0, :patch_pts], pix[1, :patch_pts]].reshape(-1, patch_size, patch_size, 1)
    return target_depths, target_weights, patch_dpt


# ------------------------------------------------------------------------------------------------ the tiny scene and its args
H, W, V = 32, 32, 3
# six frames: the train index is 1, 3, 5, the test index 0, 2, 4.  About 300 keypoints a frame: the quarter-resolution level of the sparse maps
# (every fourth row and column: 64 pixels) then holds a valid depth in every frame -- a cascade stage without one is NaN (torch's mean of nothing)
KP_COUNTS = (300, 320, 310, 330, 305, 315)
NDEPTHS = [48, 32, 8]                     # that test's: at 32 x 32 the quarter-resolution stage needs D = 48 to leave batch-norm more than one value


def tiny_scene_arrays(seed=41):
    return SC.make_scene(H, W, KP_COUNTS, seed)


def tiny_scene(device, seed=41, scan=0):
    from uc_nerf_amd.data.scene import DeviceScene
    s = tiny_scene_arrays(seed)
    return DeviceScene.from_arrays(s["poses"], s["focal"], s["bounds"], s["sparse"], s["frames"], s["dpt"], s["depths_h"] + 0.5, device=device, scan=scan)


def tiny_args(device, **over):
    """The opt.py fields the loop reads, at the tiny scene's sizes: batch_size = 32 = 2 patches of 4 x 4, so the batch is [32 patch points | no uniform ray |
    the target's keypoints]; N_samples a multiple of 3 (build_rays' three cascade ranges); chunk = 300 does not divide 32 * 32 = 1024."""
    a = dict(multires=10, multires_views=4, i_embed=0, netdepth=6, netwidth=128, net_type="v2", view_num=V, netchunk=1024, perturb=1.0, N_samples=12,
             use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, ckpt=None, device=str(device), img_downscale=1.0, use_color_volume=False,
             chunk=300, pad=0, batch_size=32, patch_num=2, patch_size=4, lrate=5e-4, num_epochs=4, finetune=None, log=False, basedir=".",
             expname="tiny", num_train_samples=3, pts_dim=3, dir_dim=3)
    a.update(over)
    return types.SimpleNamespace(**a)


def tiny_mvs(**kw):
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    return CascadeMVSNet.with_cnns(view_num=V, ndepths=NDEPTHS, **kw)
