"""The whole-image path on the GPU: ucnerf_image_put, ucnerf_depth_minmax, ucnerf_depth_colormap, the visualize_depth mirror and
uc_nerf_amd.validate.render_validation_image against the numpy restatement of tests/image_cases.py and the reference's host ops.

Everything is compared bit for bit (the arithmetic is two subtractions, two divisions and a product in float32, each correctly rounded on
both sides), except the sign of a zero minimum / maximum, which numpy does not define either.  The saturation values (NaN -> 0, below 0 -> 0,
above 255 -> 255) are asserted as include/ucnerf_hip.h documents them, not against numpy, which leaves them undefined."""
import types

import numpy as np
import pytest
import torch

import image_cases as IC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32 = np.float32
GROUP = IC.GROUP_PIXELS


def ops():
    from uc_nerf_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: the cached cases are read-only)


# ------------------------------------------------------------------------------------------------ assembly
def _put(order, capacity=0, with_cell=True):
    """The 5 x 7 case put chunk by chunk (`order`: list of (first, n)) into planes with `capacity` pixels to spare behind the image."""
    o = ops()
    H, W = 5, 7
    rgb, depth = IC.put_case()
    pixels = H * W + capacity
    rgb_chw = torch.full((3, pixels), -7.0, device=DEV)
    depth_hw = torch.full((pixels,), -7.0, device=DEV)
    cell = o.minmax_reset(device=DEV) if with_cell else None
    for first, n in order:
        o.image_put(dev(rgb[first:first + n]), dev(depth[first:first + n]), first, rgb_chw, depth_hw, cell)
    return rgb_chw.cpu().numpy(), depth_hw.cpu().numpy(), cell


@pytest.mark.parametrize("name,order,capacity", [
    ("chunks_of_4", [(f, min(4, 35 - f)) for f in range(0, 35, 4)], 0),            # a partial last chunk of 3
    ("one_chunk_of_35", [(0, 35)], 0),
    ("capacity_to_spare", [(0, 35)], 13),
    ("out_of_order", [(f, min(4, 35 - f)) for f in (32, 8, 0, 28, 4, 16, 24, 12, 20)], 0),
])
def test_image_put_equals_the_host_ops_bit_for_bit(name, order, capacity):
    assert order[0][1] in (4, 35, 3) and sum(n for _, n in order) == 35
    rgb, depth = IC.put_case()
    want_rgb, want_depth = IC.assemble_reference(rgb, depth, 5, 7)
    got_rgb, got_depth, cell = _put(order, capacity)
    assert IC.same_bits(got_rgb[:, :35].reshape(3, 5, 7), want_rgb), name
    assert IC.same_bits(got_depth[:35].reshape(5, 7), want_depth), name
    assert (got_rgb[:, 35:] == -7.0).all() and (got_depth[35:] == -7.0).all()      # nothing behind the image is touched
    # NaN stays NaN, -0.0 stays -0.0 (torch.clamp's semantics), spelled out
    src = rgb.reshape(5, 7, 3).transpose(2, 0, 1)
    assert np.isnan(got_rgb[:, :35].reshape(3, 5, 7)[np.isnan(src)]).all()
    assert (IC.bits(got_rgb[:, :35].reshape(3, 5, 7))[IC.bits(src) == 0x80000000] == 0x80000000).all()
    # the range accumulated over the chunks is the whole map's
    assert IC.same_values(ops().minmax_value(cell).cpu().numpy(), np.array(IC.minmax_reference(depth), F32)), name


def test_image_put_refuses_an_overrun_and_launches_nothing():
    o = ops()
    from uc_nerf_amd import _lib as L
    rgb, depth = IC.put_case()
    rgb_chw = torch.full((3, 5, 7), -7.0, device=DEV)
    depth_hw = torch.full((5, 7), -7.0, device=DEV)
    cell = o.minmax_reset(device=DEV)
    with pytest.raises(RuntimeError, match="overrun"):
        o.image_put(dev(rgb[:4]), dev(depth[:4]), 32, rgb_chw, depth_hw, cell)
    p = L.ImagePutParams()
    p.n, p.first_pixel, p.pixels = 4, 32, 35
    p.rgb, p.depth, p.rgb_chw, p.depth_hw, p.minmax = dev(rgb[:4]).data_ptr(), dev(depth[:4]).data_ptr(), rgb_chw.data_ptr(), depth_hw.data_ptr(), cell.data_ptr()
    import ctypes as C
    assert L.lib().ucnerf_image_put(C.addressof(p), None) == -1                    # UCNERF_EINVAL
    torch.cuda.synchronize()
    assert (rgb_chw == -7.0).all() and (depth_hw == -7.0).all()
    assert np.isnan(o.minmax_value(cell).cpu().numpy()).all()                       # the cell is still empty: (NaN, NaN)
    o.image_put(dev(rgb[:0]), dev(depth[:0]), 35, rgb_chw, depth_hw, cell)          # an empty chunk at the end: fine, nothing written
    assert (depth_hw == -7.0).all()


# ------------------------------------------------------------------------------------------------ min / max
@pytest.mark.parametrize("kind", IC.MINMAX_KINDS)
@pytest.mark.parametrize("count", IC.MINMAX_COUNTS)
def test_depth_minmax_equals_numpy(count, kind):
    x = IC.minmax_data(count, kind)
    got = ops().depth_minmax(dev(x)).cpu().numpy()
    want = np.array(IC.minmax_reference(x), F32)
    assert got.dtype == F32 and got.shape == (2,)
    assert IC.same_values(got, want), (count, kind, got, want)                      # +-0 compare equal; everything else has one bit pattern
    assert np.array_equal(IC.bits(got)[want != 0], IC.bits(want)[want != 0])


def test_minmax_cell_accumulates_and_resets():
    o = ops()
    a, b = IC.minmax_data(GROUP + 1, "tame"), IC.minmax_data(65, "negative")
    cell = o.minmax_reset(device=DEV)
    assert cell.dtype == torch.int32 and np.isnan(o.minmax_value(cell).cpu().numpy()).all()
    o.depth_minmax(dev(b), cell)
    got = o.depth_minmax(dev(a), cell).cpu().numpy()
    assert IC.same_values(got, np.array(IC.minmax_reference(np.concatenate([a, b])), F32))
    o.minmax_reset(cell)
    assert IC.same_values(o.depth_minmax(dev(b), cell).cpu().numpy(), np.array(IC.minmax_reference(b), F32))
    assert o.image_group_pixels() == GROUP


# ------------------------------------------------------------------------------------------------ index map and colour
@pytest.mark.parametrize("name", IC.DEPTH_NAMES)
def test_index_map_equals_the_restatement_bit_for_bit(name):
    case = IC.depth_case(name)
    want = IC.index_reference(case["depth"], case["minmax"])
    idx, color = ops().depth_colormap(dev(case["depth"]), minmax=case["minmax"], want_color=False)
    assert color is None and idx.dtype == torch.uint8 and tuple(idx.shape) == case["depth"].shape
    got = idx.cpu().numpy()
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    x = case["depth"]
    if name == "constant":
        assert (got == 0).all()
    if name == "two_valued":
        assert set(np.unique(got).tolist()) == {0, 255}       # fl(1.5 + 1e-8) = 1.5: t = 1 exactly at the upper value
    if name == "lattice":
        assert np.array_equal(got.reshape(-1), np.arange(256))
    if name == "given_range":                                 # documented saturation, not numpy's
        assert (got[x < 2.0] == 0).all() and (got[x > 5.0] == 255).all()
    if name == "nonfinite_given":
        assert (got[np.isnan(x)] == 0).all() and (got[x == np.inf] == 255).all() and (got[x == -np.inf] == 0).all()
    if name == "nonfinite":
        assert (got == 0).all()                               # range +-FLT_MAX: d = inf, t = 0 or NaN


def test_index_map_from_a_cell_equals_the_maps_own_range():
    o = ops()
    case = IC.depth_case("random")
    d = dev(case["depth"])
    cell = o.minmax_reset(device=DEV)
    o.depth_minmax(d, cell)
    a = o.depth_colormap(d, minmax=cell, want_color=False)[0]
    b = o.depth_colormap(d, want_color=False)[0]
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), IC.index_reference(case["depth"]))
    empty = o.minmax_reset(device=DEV)                        # an empty cell is (NaN, NaN): index 0 everywhere
    assert (o.depth_colormap(d, minmax=empty, want_color=False)[0] == 0).all()


@pytest.mark.parametrize("table_name", ["random", "jet"])
@pytest.mark.parametrize("name", ["random", "given_range", "two_valued"])
def test_colour_equals_table_over_255_bit_for_bit(name, table_name):
    from uc_nerf_amd.utils import colormaps
    o = ops()
    table = IC.random_table() if table_name == "random" else colormaps.jet_lut()
    case = IC.depth_case(name)
    idx, color = o.depth_colormap(dev(case["depth"]), o.colormap_table(table, DEV), minmax=case["minmax"])
    assert color.dtype == torch.float32 and tuple(color.shape) == (3,) + case["depth"].shape
    want_idx = IC.index_reference(case["depth"], case["minmax"])
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert IC.same_bits(color.cpu().numpy(), IC.color_reference(want_idx, table)), (name, table_name)
    only = o.depth_colormap(dev(case["depth"]), o.colormap_table(table, DEV), minmax=case["minmax"], want_index=False)
    assert only[0] is None and torch.equal(only[1], color)


@pytest.mark.parametrize("name", IC.DEPTH_NAMES)
def test_visualize_depth_device_and_cpu_are_bit_identical(name):
    from uc_nerf_amd.utils.utils import visualize_depth
    case = IC.depth_case(name)
    table = IC.random_table()
    on_dev = visualize_depth(dev(case["depth"]), case["minmax"], table)
    on_cpu = visualize_depth(torch.from_numpy(case["depth"].copy()), case["minmax"], table)
    assert on_dev.is_cuda and not on_cpu.is_cuda and on_dev.shape == on_cpu.shape
    assert IC.same_bits(on_dev.cpu().numpy(), on_cpu.numpy()), name
    if name == "random":                                      # the default table, and a table handed over as a device tensor
        assert IC.same_bits(visualize_depth(dev(case["depth"])).cpu().numpy(), visualize_depth(case["depth"]).numpy())
        assert torch.equal(visualize_depth(dev(case["depth"]), cmap=dev(table)), on_dev)


# ------------------------------------------------------------------------------------------------ whole image
_WHOLE = {}


def _whole_setup():
    """12 x 20 synthetic scene, the network and what train.py hands to the loop; built once."""
    if _WHOLE:
        return _WHOLE
    import uc_nerf_amd
    uc_nerf_amd.install_dropin()
    import network.models as models
    from uc_nerf_amd.synthetic import cascade_outputs, init_ucnerf_state_dict, make_scene, scene_to
    H, W = 12, 20
    scene = scene_to(make_scene(seed=1, H=H, W=W, small_volumes=True), DEV)
    a = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=6, netwidth=128, feat_dim=97, net_type="v2", view_num=7, netchunk=1024,
                              perturb=1.0, N_samples=90, use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, ckpt=None, device=str(DEV),
                              img_downscale=1.0, use_color_volume=False, chunk=64, pad=0)
    kw, _, _, _ = models.create_ucnerf(a, dir_embedder=True, pts_embedder=True)          # as train.py:36-37
    kw["network_fn"].load_state_dict(init_ucnerf_state_dict(seed=0, n_src=6, sigma_scale=0.05, sigma_bias=0.05))
    outputs = cascade_outputs(scene)
    outputs["stage3"]["img_feats"] = scene["img_feat"]
    near_fars = torch.tensor([[scene["near"], scene["far"]]] * 7, device=DEV)
    depth_gt = torch.rand(H, W, generator=torch.Generator().manual_seed(3)) * 3
    depth_gt[2:4] = 0.0                                       # a band without ground truth
    _WHOLE.update(H=H, W=W, scene=scene, args=a, kw=kw, outputs=outputs, near_fars=near_fars, depth_gt=depth_gt,
                  gt_rgb=torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)))
    return _WHOLE


def _pose(scene):
    return {"w2cs": scene["w2cs"].clone(), "intrinsics": scene["intrinsics"].clone(), "c2ws": scene["c2w"].unsqueeze(0).clone()}


def _reference_loop(s, chunk):
    """train.py:251-279, literally: build_rays_test + rendering per chunk, .cpu(), cat, clamp, reshape, permute."""
    import network.renderer as renderer
    import utils.utils as U
    H, W, scene, a, kw, outputs, near_fars = s["H"], s["W"], s["scene"], s["args"], s["kw"], s["outputs"], s["near_fars"]
    pose_ref = _pose(scene)
    world_to_ref, tgt_to_world, intrinsic = pose_ref["w2cs"][0], pose_ref["c2ws"][0], pose_ref["intrinsics"][0]
    rgbs, depth_preds = [], []
    with torch.no_grad():
        for chunk_idx in range(H * W // chunk + int(H * W % chunk > 0)):
            rays_pts, rays_dir, rays_NDC, depth_candidates, rays_o, ndc_parameters = U.build_rays_test(
                H, W, tgt_to_world, world_to_ref, intrinsic, near_fars, near_fars[-1], a.N_samples, pad=a.pad, chunk=chunk, idx=chunk_idx, outputs=outputs)
            rgb, depth_pred = renderer.rendering(a, pose_ref, rays_pts, rays_NDC, depth_candidates, rays_dir, outputs, scene["imgs"], near_fars=near_fars[0],
                                                 img_feat=outputs["stage3"]["img_feats"], confidence=scene["confidence"], ndc_parameters=ndc_parameters, **kw)
            rgbs.append(rgb.cpu())
            depth_preds.append(depth_pred.cpu())
    return torch.clamp(torch.cat(rgbs).reshape(H, W, 3).permute(2, 0, 1), 0, 1), torch.cat(depth_preds).reshape(H, W), len(rgbs), pose_ref


def _driver(s, chunk, **kw):
    from uc_nerf_amd.validate import render_validation_image
    a = types.SimpleNamespace(**dict(vars(s["args"]), chunk=chunk))
    pose_ref = _pose(s["scene"])
    log = render_validation_image(a, pose_ref, s["outputs"], s["scene"]["imgs"], s["scene"]["confidence"], s["H"], s["W"], s["near_fars"], s["kw"], **kw)
    return log, pose_ref


@pytest.mark.parametrize("chunk", [64, 240])
def test_whole_image_equals_the_reference_style_loop(chunk):
    from uc_nerf_amd.utils.utils import visualize_depth
    s = _whole_setup()
    H, W = s["H"], s["W"]
    torch.manual_seed(21)                                     # build_rays_test draws its jitter from torch's generator
    want_rgb, want_depth, n_chunks, pose_after = _reference_loop(s, chunk)
    assert n_chunks == (4 if chunk == 64 else 1) and (chunk != 64 or H * W - 3 * 64 == 48)
    torch.manual_seed(21)
    table = IC.random_table()
    log, pose_ref = _driver(s, chunk, depth_gt=s["depth_gt"], gt_rgb=s["gt_rgb"], cmap=table)
    assert set(log) == {"pred_rgb", "pred_depth", "gt_rgb", "gt_depth", "mask", "pred_depth_vis", "gt_depth_vis", "uncertainty"}
    assert all(v.is_cuda for v in log.values())
    assert tuple(log["pred_rgb"].shape) == (3, H, W) and tuple(log["pred_depth"].shape) == (H, W)
    assert IC.same_bits(log["pred_rgb"].cpu().numpy(), want_rgb.numpy())
    assert IC.same_bits(log["pred_depth"].cpu().numpy(), want_depth.numpy())
    assert pose_ref["w2cs"].shape[0] == pose_after["w2cs"].shape[0] == 6          # rendering's in-place trim, as in the reference's loop
    assert torch.equal(log["uncertainty"].cpu(), (1 - s["scene"]["confidence"].cpu()).reshape(H, W))
    assert torch.equal(log["mask"].cpu(), s["depth_gt"] > 0) and torch.equal(log["gt_depth"].cpu(), s["depth_gt"]) and torch.equal(log["gt_rgb"].cpu(), s["gt_rgb"])
    assert IC.same_bits(log["pred_depth_vis"].cpu().numpy(), visualize_depth(log["pred_depth"].cpu(), cmap=table).numpy())
    assert IC.same_bits(log["gt_depth_vis"].cpu().numpy(), visualize_depth(s["depth_gt"], cmap=table).numpy())
    # the results feed the metrics directly
    from uc_nerf_amd.utils.evaluation import depth_evaluation, rgb_evaluation
    psnr, ssim, _ = rgb_evaluation(log["gt_rgb"][None], log["pred_rgb"][None], None)
    assert np.isfinite(psnr) and np.isfinite(ssim)
    assert np.isfinite(depth_evaluation(log["gt_depth"][None], log["pred_depth"][None])).all()
    # without ground truth: the reference's two keys and the three added ones that need none
    torch.manual_seed(21)
    log2, _ = _driver(s, chunk)
    assert set(log2) == {"pred_rgb", "pred_depth", "pred_depth_vis", "uncertainty"} and torch.equal(log2["pred_rgb"], log["pred_rgb"])


def test_whole_image_driver_makes_no_synchronising_call():
    """Under torch's sync debug mode "error" a synchronising torch call raises.  Whether this torch build honours the mode is established first with
    a plain .item(); if it does not, the assertion is skipped.  (The mode does not see ctypes calls: that the new entry points themselves do not
    synchronise is a matter of reading csrc/image.hip, which contains no synchronising or copying runtime call -- tests/test_image_cases_host.py.)"""
    s = _whole_setup()
    depth_gt, gt_rgb = s["depth_gt"].to(DEV), s["gt_rgb"].to(DEV)
    _driver(s, 64, depth_gt=depth_gt, gt_rgb=gt_rgb)          # warm: one-time uploads (the colour table, cached constants)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    log = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            log, _ = _driver(s, 64, depth_gt=depth_gt, gt_rgb=gt_rgb)      # raises where a torch call inside the driver synchronises
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error'): the driver's freedom from synchronising calls "
                    "cannot be asserted this way here")
    assert log["pred_rgb"].is_cuda and len(log) == 8
