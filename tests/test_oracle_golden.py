"""T1: the CPU oracle reproduces the golden vectors captured from the reference (tests/golden/*.npz)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, state_dict_from
from oracle import ucnerf_oracle as O

torch.set_num_threads(4)


@pytest.fixture(autouse=True)
def capture_host_rounding():
    """The golden vectors hold the reference's float32 camera products as MKL rounded them on the capture host (fused multiply-adds)."""
    with O.fused_camera_products():
        yield


def close(a, b, atol=1e-6, rtol=1e-6):
    torch.testing.assert_close(a, b, atol=atol, rtol=rtol)


def test_g1_ray_generation():
    g = load_golden("g1_raygen")
    H, W, K, c2w = g["H"], g["W"], g["K"], g["c2w"]
    dirs = O.get_ray_directions(H, W, K)
    assert torch.equal(dirs, g["dirs"])
    ro, rd = O.get_rays(dirs, c2w[:3, :4])
    close(rd, g["rays_d"]); assert torch.equal(ro, g["rays_o"])
    mo, md, pix = O.get_rays_mvs_grid(H, W, K, c2w, chunk=64, idx=2)
    close(md, g["mvs_d"]); assert torch.equal(pix, g["mvs_pix"]); assert torch.equal(mo, g["mvs_o"])
    _, fd, fpix = O.get_rays_mvs_grid(H, W, K, c2w)
    close(fd, g["mvs_full_d"]); assert torch.equal(fpix, g["mvs_full_pix"])
    ho, hd = O.get_rays_opengl(H, W, g["gl_focal"], c2w[:3, :4])
    close(hd, g["gl_d"]); close(ho, g["gl_o"])
    d4 = O.get_ray_directions(400, 400, g["K400"])
    o4, r4 = O.get_rays(d4, c2w[:3, :4])
    close(r4[g["sel400"]], g["d400"]); close(o4[g["sel400"]], g["o400"])


def test_g2_ndc_rays():
    g = load_golden("g2_ndc_rays")
    o, d = O.get_ndc_rays(g["H"], g["W"], g["focal2"].tolist(), g["near"], g["rays_o"], g["rays_d"])
    close(o, g["o_ru"], 1e-5, 1e-5); close(d, g["d_ru"], 1e-5, 1e-5)
    o, d = O.ndc_rays(g["H"], g["W"], g["focal"], g["near"], g["rays_o"], g["rays_d"])
    close(o, g["o_h"], 1e-5, 1e-5); close(d, g["d_h"], 1e-5, 1e-5)


def test_g3_sampling():
    g = load_golden("g3_sampling")
    rays, S = g["rays"], g["S"]
    pts, _, _, z = O.ray_marcher(rays, S)
    assert torch.equal(z, g["z_det"]); close(pts, g["pts_det"])
    _, _, _, zl = O.ray_marcher(rays, S, lindisp=True)
    close(zl, g["z_lindisp"])
    pts, _, _, z = O.ray_marcher(rays, S, perturb=1.0, noise=g["noise"])
    close(z, g["z_p1"]); close(pts, g["pts_p1"])
    _, _, _, z = O.ray_marcher(rays, S, perturb=0.5, noise=g["noise"])
    close(z, g["z_p05"])
    # live cascade sampler as driven by build_rays_test (chunk 32, idx 1 of an 8x12 image)
    H, W, NS = g["bt_H"], g["bt_W"], g["bt_NS"]
    ro, rd, pix = O.get_rays_mvs_grid(H, W, g["bt_K"], g["bt_c2w"], chunk=32, idx=1)
    close(rd, g["bt_dir"])
    p = pix.long()
    nf = {}
    for k, d in (("1", 4), ("2", 2), ("3", 1)):
        dv = g["bt_dv" + k]
        pr, pc = torch.div(p[0], d, rounding_mode="trunc"), torch.div(p[1], d, rounding_mode="trunc")
        nf["near_" + k], nf["far_" + k] = dv[0, 0, pr, pc].unsqueeze(1), dv[0, -1, pr, pc].unsqueeze(1)
    z = O.cascade_depth_candidates(nf["near_1"], nf["far_1"], nf["near_2"], nf["far_2"], nf["near_3"], nf["far_3"], NS,
                                   g["bt_t_rand"])
    close(z, g["bt_z"])
    pts = ro.reshape(1, 1, 3) + z.unsqueeze(-1) * rd.unsqueeze(1)
    close(pts, g["bt_pts"])
    nfe = {k: v.expand(-1, NS).unsqueeze(-1) for k, v in nf.items()}
    nfe["near"], nfe["far"] = g["bt_near_fars"][0, 0], g["bt_near_fars"][0, 1]
    ndc = O.get_ndc_coordinate(g["bt_w2c"], g["bt_K"], pts, torch.tensor([W - 1, H - 1]), nfe)
    for k, name in (("stage1", "bt_ndc1"), ("stage2", "bt_ndc2"), ("stage3", "bt_ndc3"), ("ndc", "bt_ndc")):
        close(ndc[k], g[name], 1e-5, 1e-5)


def test_g4_ndc_coordinate_with_clamp_rows():
    g = load_golden("g4_ndc_coord")
    nf = {k: g[k] for k in ("near_1", "far_1", "near_2", "far_2", "near_3", "far_3")}
    nf["near"], nf["far"] = torch.tensor(g["near"]), torch.tensor(g["far"])
    out = O.get_ndc_coordinate(g["w2c"], g["K"], g["pts"], g["inv_scale"], nf)
    for k in ("stage1", "stage2", "stage3", "ndc"):
        # clamp rows divide by 1e-4: compare relatively
        close(out[k], g["out_" + k], 1e-5, 2e-5)
    close(O.get_ndc_coordinate(g["w2c"], g["K"], g["pts"], g["inv_scale"], sample_2d=True), g["q2d"], 1e-5, 2e-5)


def test_g5_embedders():
    g = load_golden("g5_embed")
    x = g["x"]
    assert g["d10"] == 63 and g["d4"] == 27
    # 2^k x is exact; sin/cos come from the same libm on CPU -> expect equality up to an ulp
    close(O.embed_live(x, 10), g["live10"], 1e-6, 0)
    close(O.embed_live(x, 4), g["live4"], 1e-6, 0)
    close(O.embed_live(x.reshape(8, 8, 3), 10), g["live10_3d"], 1e-6, 0)
    close(O.embed_interleaved(x, 10), g["inter10"], 1e-6, 0)
    close(O.embed_interleaved(x, 4), g["inter4"], 1e-6, 0)
    # the two layouts are permutations of each other
    perm = [0, 1, 2] + [3 + 3 * k + c for k in range(10) for c in range(3)]
    assert not torch.equal(g["live10"], g["inter10"])
    assert torch.equal(g["live10"][:, 3:33].reshape(-1, 10, 3), g["inter10"][:, 3:].reshape(-1, 10, 2, 3)[:, :, 0])


@pytest.mark.parametrize("tag", ["v7", "v4"])
def test_g6_mlp_forward_and_grads(tag, sd_v7):
    g = load_golden("g6_mlp_" + tag)
    V = g["V"]
    sd = sd_v7 if tag == "v7" else state_dict_from(g)
    names = [n for n, _ in O.ucnerf_param_shapes(n_src=V - 1)]
    assert names == list(sd.keys())
    for n, shp in O.ucnerf_param_shapes(n_src=V - 1):
        assert tuple(sd[n].shape) == shp, n
    assert sum(v.numel() for v in sd.values()) == (181642 if V == 7 else sum(v.numel() for v in sd.values()))
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = g["x"].clone().requires_grad_(True)
    out = O.ucnerf_mlp(p, x, n_src=V - 1)
    scale = g["out"].abs().max().item()
    close(out, g["out"], 2e-5 * max(1.0, scale), 1e-4)
    (out * g["r"]).sum().backward()
    gs = g["grad_x"].abs().max().item()
    close(x.grad, g["grad_x"], 1e-4 * gs, 1e-3)
    if tag == "v7":
        no_grad = set(g["no_grad_names"].tolist())
        assert no_grad == {"nerf.pts_bias_confidence_1.weight", "nerf.pts_bias_confidence_1.bias",
                           "nerf.feature_linear_1.weight", "nerf.feature_linear_1.bias",
                           "nerf.confi_linear.weight", "nerf.confi_linear.bias"}
        for k in names:
            if k in no_grad:
                assert p[k].grad is None
            else:
                ref = g["grad." + k]
                close(p[k].grad, ref, 1e-4 * ref.abs().max().item(), 1e-3)


def _ndc_dict(g):
    return {"stage1": g["ndc1"], "stage2": g["ndc2"], "stage3": g["ndc3"], "ndc": g["ndc"]}


def test_g7_feature_gather_and_grads():
    g = load_golden("g7_gather")
    V = g["V"]
    vols = [g["vol1"].clone().requires_grad_(True), g["vol2"].clone().requires_grad_(True),
            g["vol3"].clone().requires_grad_(True)]
    img_feat = g["img_feat"].clone().requires_grad_(True)
    conf = g["conf"].clone().requires_grad_(True)
    ndc = _ndc_dict(g)
    rf, cs = O.index_point_feature(vols, conf, ndc)
    close(rf, g["ray_feats"], 1e-5, 1e-5); close(cs, g["conf_sampled"], 1e-6, 1e-5)
    w2cs, Ks = g["w2cs"][1:], g["K"].repeat(V - 1, 1, 1)
    cv = O.build_color_volume(g["pts"], w2cs, Ks, g["imgs"], img_feat)
    close(cv, g["color_volume"], 2e-5, 1e-5)
    feats = O.gen_pts_feats(g["imgs"], vols, g["pts"], w2cs, Ks, ndc, img_feat, conf)
    assert feats.shape[-1] == 24 + 12 * (V - 1) + 1
    close(feats, g["feats"], 2e-5, 1e-5)
    (feats * g["r"]).sum().backward()
    for t, name in zip(vols + [img_feat, conf], ("g_vol1", "g_vol2", "g_vol3", "g_img_feat", "g_conf")):
        close(t.grad, g[name], 2e-5, 1e-4)


def test_g8_rowsum_and_cumsum_bit_patterns():
    g = load_golden("g8_rowsum")
    for n in list(range(1, 71)) + [127, 128, 190, 191]:
        x = g["x%d" % n]
        assert np.array_equal(O.torch_cpu_rowsum_f32(x.numpy()), g["s%d" % n].numpy()), n
        assert np.array_equal(O.torch_cpu_cumsum_f32(x.numpy()), g["c%d" % n].numpy()), n


def test_g8_sample_pdf_indices_bit_exact():
    g = load_golden("g8_sample_pdf")
    bins, w, M = g["bins"], g["weights"], g["M"]
    N = bins.shape[0]
    u_det = torch.linspace(0., 1., M).expand(N, M).contiguous()
    s, inds, cdf = O.sample_pdf(bins, w, u_det)
    assert torch.equal(cdf, g["cdf"])                    # bit-exact cdf => bit-exact indices
    assert torch.equal(inds, g["inds_det"])
    assert torch.equal(s, g["samples_det"]) and torch.equal(s, g["samples_det_helpers"])
    s, inds, _ = O.sample_pdf(bins, w, g["u"])
    assert torch.equal(inds, g["inds_u"])
    assert torch.equal(s, g["samples_u"])
    s, _, _ = O.sample_pdf(bins[:16], w[:16], g["u_pytest"])
    assert torch.equal(s, g["samples_pytest"])
    assert inds.dtype == torch.int64 and int(inds.max()) <= bins.shape[1]


@pytest.mark.parametrize("S", [64, 90, 192])
def test_g9_compositing(S):
    g = load_golden("g9_composite")
    raw = g["S%d_raw" % S].clone().requires_grad_(True)
    z = g["S%d_z" % S]
    for wb in (False, True):
        res = O.raw2outputs_live(raw, z, wb)
        tag = "S%d_wb%d_" % (S, wb)
        for name, t in zip(("rgb", "disp", "acc", "weights", "depth", "alpha", "var"), res):
            torch.testing.assert_close(t, g[tag + name], atol=2e-6, rtol=1e-5, equal_nan=True)
    res = O.raw2outputs_live(raw, z, False)
    ((res[0] * g["S%d_r3" % S]).sum() + (res[4] * g["S%d_r1" % S]).sum()).backward()
    close(raw.grad, g["S%d_graw" % S], 1e-5, 1e-4)
    resh = O.raw2outputs_helpers(g["S%d_h_raw" % S], z, g["S%d_h_rays_d" % S])
    for name, t in zip(("rgb", "disp", "acc", "weights", "depth"), resh):
        torch.testing.assert_close(t, g["S%d_h_" % S + name], atol=2e-6, rtol=1e-5, equal_nan=True)
    close(O.raw2outputs_helpers(g["S%d_h_raw" % S], z, g["S%d_h_rays_d" % S], white_bkgd=True)[0],
          g["S%d_h_rgb_wb" % S], 2e-6, 1e-5)
    close(O.depth2dist(z, g["S%d_h_rays_d" % S].norm(dim=-1)), g["S%d_dists" % S], 1e-6, 1e-6)


def test_g10_rendering_first_and_second_call(sd_v7):
    g = load_golden("g10_rendering")
    V = g["V"]
    vols = [g["vol1"], g["vol2"], g["vol3"]]
    pose = {"w2cs": g["w2cs"].clone(), "intrinsics": g["K"].repeat(V, 1, 1)}
    args = (g["pts"], _ndc_dict(g), g["z"], g["rays_d"], vols, g["imgs"], g["img_feat"], g["conf"], V)
    rgb1, d1 = O.rendering(sd_v7, pose, *args)
    assert pose["w2cs"].shape[0] == g["n_w2cs_after_first"] == V - 1     # in-place trim (renderer.py:241-243)
    rgb2, d2 = O.rendering(sd_v7, pose, *args)
    close(rgb1, g["rgb_first"], 2e-5, 1e-4); close(d1, g["depth_first"], 5e-5, 1e-4)
    close(rgb2, g["rgb_second"], 2e-5, 1e-4); close(d2, g["depth_second"], 5e-5, 1e-4)
    assert (g["rgb_first"] - g["rgb_second"]).abs().max() > 1e-4          # the quirk is observable
    pose = {"w2cs": g["w2cs"].clone(), "intrinsics": g["K"].repeat(V, 1, 1)}
    rgbw, _ = O.rendering(sd_v7, pose, *args, white_bkgd=True)
    close(rgbw, g["rgb_white"], 2e-5, 1e-4)


def scene_from_golden(g, dtype=torch.float32):
    V = g["V"]
    return dict(K=g["K"].to(dtype), c2w=torch.eye(4, dtype=dtype), w2cs=g["w2cs"].to(dtype),
                intrinsics=g["K"].to(dtype).repeat(V, 1, 1), near=g["near"], far=g["far"],
                vols=[g["vol1"].to(dtype), g["vol2"].to(dtype), g["vol3"].to(dtype)], imgs=g["imgs"].to(dtype),
                img_feat=g["img_feat"].to(dtype), confidence=g["conf"].to(dtype))


def scaled_sd(sd, s, b=0.0):
    sd = {k: v.clone() for k, v in sd.items()}
    for n in ("nerf.alpha_linear", "nerf.alpha_linear_1"):
        sd[n + ".weight"] *= s
        sd[n + ".bias"] += b
    return sd


def test_g11_coarse_fine_composition(sd_v7):
    """64 coarse + 128 fine.  The fine depths come from searchsorted over coarse weights that carry fp32
    rounding noise and the synthetic volumes are white noise, so the free-running composition is only
    statistically comparable; the pinned checks are stage-wise with the reference's own intermediate
    tensors fed in (teacher forcing)."""
    g = load_golden("g11_coarse_fine")
    sd = scaled_sd(sd_v7, g["sigma_head_scale"], g["sigma_head_bias"])
    scene = scene_from_golden(g)
    out = O.render_coarse_fine(sd, scene, g["xs"], g["ys"], 64, 128)
    assert torch.equal(out["z_coarse"], g["z_coarse"])
    close(out["coarse"]["rgb"], g["c_rgb"], 2e-5, 1e-4)
    close(out["coarse"]["depth"], g["c_depth"], 5e-5, 1e-4)
    close(out["coarse"]["weights"], g["c_weights"], 2e-5, 1e-3)
    # stage 2, teacher-forced: reference coarse weights -> bit-exact fine depths
    zc = g["z_coarse"]
    u = torch.linspace(0., 1., 128).expand(zc.shape[0], 128).contiguous()
    z_s, _, _ = O.sample_pdf(.5 * (zc[:, :-1] + zc[:, 1:]), g["c_weights"][:, 1:-1].contiguous(), u)
    assert torch.equal(z_s, g["z_samples"])
    assert torch.equal(O.merge_sorted(z_s, zc), g["z_fine"])
    # stage 3, teacher-forced: reference z_fine -> final render within 1e-4
    fine = O.render_coarse_fine(sd, scene, g["xs"], g["ys"], 64, 128, z_fine_override=g["z_fine"])
    close(fine["rgb"], g["f_rgb"], 1e-4, 0); close(fine["depth"], g["f_depth"], 1e-4, 0)
    close(fine["acc"], g["f_acc"], 1e-4, 0); close(fine["var"], g["f_var"], 1e-5, 1e-3)
    close(fine["weights"], g["f_weights"], 2e-5, 1e-3)
    # free-running: almost every ray still lands within 1e-4 (a flipped searchsorted bin moves one sample)
    err = (out["rgb"] - g["f_rgb"]).abs().max(-1)[0]
    assert (err < 1e-4).float().mean() > 0.9 and err.median() < 1e-5


# ---------------------------------------------------------------------------------------------- f2: the step in front
@pytest.mark.parametrize("tag", ["a", "b"])
def test_g12_cost_volume_variance(tag):
    """homo_warp (utils/utils.py:1105-1172) and the variance volume DepthNet hands to the regularisation net
    (network/mvs_models.py:599-626), captured from the reference."""
    from oracle import mvs_oracle as M
    g = load_golden("g12_cost_volume")
    f = lambda k: g[tag + "_" + k]                                       # noqa: E731
    H, W, D, pad = int(f("H")), int(f("W")), int(f("D")), int(f("pad"))
    grid = M.homo_warp_grid(f("proj")[0], f("depth_values"), H, W, pad)
    assert torch.equal(grid, f("grid0"))
    warped = M.sample_nearest_border(f("feats")[0], grid).reshape(f("warped0").shape)
    assert torch.equal(warped, f("warped0"))
    feats = f("feats").clone().requires_grad_(True)
    var, _ = M.cost_volume_variance(feats, f("proj"), f("depth_values"), pad)
    assert torch.equal(var.detach(), f("variance"))
    (var * f("r_var")).sum().backward()                                  # what autograd sends into the feature maps
    close(feats.grad, f("g_feats"), 1e-6, 1e-5)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g13_depth_regression_and_confidence(tag):
    """softmax over depth, expected depth, 4-tap photometric confidence (network/mvs_models.py:629-646)."""
    from oracle import mvs_oracle as M
    g = load_golden("g13_depth_regress")
    f = lambda k: g[tag + "_" + k]                                       # noqa: E731
    init = f("prob_init") if f("prob_init").numel() else None
    x = f("prob_pre").clone().requires_grad_(True)
    p, depth, conf = M.depth_regress(x, f("depth_values"), init, int(f("pad")))
    close(p.detach(), f("prob_volume"), 1e-7, 1e-6)
    close(depth.detach(), f("depth"), 1e-6, 1e-6)
    close(conf.detach(), f("confidence"), 1e-6, 1e-6)
    ((depth * f("r_depth")).sum() + (conf * f("r_conf")).sum()).backward()   # gradient at the regularisation net's logits
    close(x.grad, f("g_prob_pre"), 1e-6, 1e-5)


def sd_v4_for_g16(g):
    """The V = 4 network of G16: G6 v4's state dict with the sigma heads rescaled as the fixture records."""
    return scaled_sd(state_dict_from(load_golden("g6_mlp_v4")), g["sigma_head_scale"], g["sigma_head_bias"])


def test_g16_rendering_hamlyn_view_count_with_everything_the_body_computes():
    """configs[3]: 3 source views (view_num 4, feat_dim 61), per-ray cascade ranges, first and second call, the
    discarded intermediates, and the gradients into the network and the gather sources."""
    g = load_golden("g16_rendering_v4")
    V = g["V"]
    sd = {k: v.clone().requires_grad_(True) for k, v in sd_v4_for_g16(g).items()}
    vols = [g["vol%d" % k].clone().requires_grad_(True) for k in (1, 2, 3)]
    img_feat, conf = g["img_feat"].clone().requires_grad_(True), g["conf"].clone().requires_grad_(True)
    pose = {"w2cs": g["w2cs"].clone(), "intrinsics": g["K"].repeat(V, 1, 1)}
    args = (g["pts"], _ndc_dict(g), g["z"], g["rays_d"], vols, g["imgs"], img_feat, conf, V)
    out = O.rendering(sd, pose, *args, full=True)
    assert pose["w2cs"].shape[0] == g["n_w2cs_after_first"] == V - 1
    close(out["feats"], g["feats"], 2e-5, 1e-5)
    close(out["raw"], g["raw"], 2e-5, 1e-4)
    close(out["rgb"], g["rgb_first"], 2e-5, 1e-4); close(out["depth"], g["depth_first"], 5e-5, 1e-4)
    close(out["acc"], g["acc"], 2e-5, 1e-4); close(out["weights"], g["weights"], 1e-5, 1e-4); close(out["var"], g["var"], 1e-6, 1e-3)
    close(out["u_sampled"], g["u_sampled"], 1e-6, 0); close(out["wu"], g["wu"], 2e-5, 1e-4)
    ((out["rgb"] * g["r3"]).sum() + (out["depth"] * g["r1"]).sum()).backward()
    for got, name in zip(vols + [img_feat, conf], ("g_vol1", "g_vol2", "g_vol3", "g_img_feat", "g_conf")):
        w = g[name]
        torch.testing.assert_close(got.grad, w, atol=2e-4 * w.abs().max().item() + 1e-8, rtol=2e-3)
    n_checked = 0
    for k, p in sd.items():
        if ("grad." + k) in g:
            w = g["grad." + k]
            torch.testing.assert_close(p.grad, w, atol=2e-4 * w.abs().max().item() + 1e-8, rtol=2e-3, msg=lambda s: k + ": " + s)
            n_checked += 1
    assert n_checked == 30                                                  # 30 of 36 tensors receive gradients
    with torch.no_grad():
        rgb2, d2 = O.rendering({k: v.detach() for k, v in sd.items()}, pose, g["pts"], _ndc_dict(g), g["z"], g["rays_d"],
                               [v.detach() for v in vols], g["imgs"], img_feat.detach(), conf.detach(), V)
    close(rgb2, g["rgb_second"], 2e-5, 1e-4); close(d2, g["depth_second"], 5e-5, 1e-4)


def test_g17_uncertainty_outputs_on_the_g10_and_g11_scenes(sd_v7):
    u17 = load_golden("g17_uncertainty")
    g = load_golden("g10_rendering")
    V = g["V"]
    out = O.rendering(sd_v7, {"w2cs": g["w2cs"].clone(), "intrinsics": g["K"].repeat(V, 1, 1)}, g["pts"], _ndc_dict(g), g["z"],
                      g["rays_d"], [g["vol1"], g["vol2"], g["vol3"]], g["imgs"], g["img_feat"], g["conf"], V, full=True)
    close(out["u_sampled"], u17["g10_u"], 1e-6, 0); close(out["wu"], u17["g10_wu"], 2e-5, 1e-4)
    close(out["weights"], u17["g10_weights"], 1e-5, 1e-4); close(out["acc"], u17["g10_acc"], 2e-5, 1e-4)
    close(out["var"], u17["g10_var"], 1e-6, 1e-3)
    g = load_golden("g11_coarse_fine")
    sd = scaled_sd(sd_v7, g["sigma_head_scale"], g["sigma_head_bias"])
    ref = O.render_coarse_fine(sd, scene_from_golden(g), g["xs"], g["ys"], 64, 128, z_fine_override=g["z_fine"])
    close(ref["coarse"]["u_sampled"], u17["g11_c_u"], 1e-6, 0); close(ref["u_sampled"], u17["g11_f_u"], 1e-6, 0)
    ok = (g["ys"] > 0) & (g["ys"] < g["H"] - 1)          # rows 0 / H-1 sit on the in-mask discontinuity (see test_g11)
    close(ref["coarse"]["wu"][ok], u17["g11_c_wu"][ok], 2e-5, 1e-4); close(ref["wu"][ok], u17["g11_f_wu"][ok], 2e-5, 1e-4)


def test_g18_training_ray_builder_downstream_of_the_pixel_picks():
    """G18 = the reference's build_rays (utils/utils.py:400-597) with every random draw recorded.  Given the pixels it picked and its jitter draws, the
    oracle's pieces reproduce its rays, colours, cascade depths, points and normalised coordinates -- and the picks themselves follow from the
    recorded draws (patch cells from the multinomial picks, shifts from numpy, uniform pixels from randint, sparse-depth pixels last)."""
    g = load_golden("g18_build_rays")
    H, W, NS, ps, patch_num = g["H"], g["W"], g["NS"], g["patch_size"], g["patch_num"]
    draws = [g["draw_%03d" % i] for i in range(g["n_draws"])]
    # the pixel list from the draws
    rows, cols, k = [], [], 0
    for half in range(2):
        sel = draws[k]; k += 1
        for j in range(patch_num // 2):
            cr = min(max(int(sel[j]) // W // ps, 0), H // ps - 2)
            cc = min(max(int(sel[j]) % W // ps, 0), W // ps - 2)
            r0, c0 = cr * ps + int(draws[k]), cc * ps + int(draws[k + 1]); k += 2
            rr, cc_ = torch.arange(r0, min(r0 + ps, H)), torch.arange(c0, min(c0 + ps, W))
            rows.append(rr.repeat_interleave(cc_.numel())); cols.append(cc_.repeat(rr.numel()))
    xs_u, ys_u = draws[k], draws[k + 1]
    rows += [ys_u, g["coords"][:, 0].long()]; cols += [xs_u, g["coords"][:, 1].long()]
    pix = torch.stack([torch.cat(rows), torch.cat(cols)])
    assert torch.equal(pix, g["pix"])
    t_rand = draws[k + 2]
    _, rd, _ = O.get_rays_mvs_pixels(pix[1].float(), pix[0].float(), g["K"], g["c2ws"][0])
    close(rd, g["rays_d"])
    assert torch.equal(g["imgs"][0, 0][:, pix[0], pix[1]].t(), g["colors"])
    nf = {}
    for kk, d in (("1", 4), ("2", 2), ("3", 1)):
        dv = g["stage%s_depth_values" % kk]
        pr, pc = torch.div(pix[0], d, rounding_mode="trunc"), torch.div(pix[1], d, rounding_mode="trunc")
        nf["near_" + kk], nf["far_" + kk] = dv[0, 0, pr, pc].unsqueeze(1), dv[0, -1, pr, pc].unsqueeze(1)
    z = O.cascade_depth_candidates(nf["near_1"], nf["far_1"], nf["near_2"], nf["far_2"], nf["near_3"], nf["far_3"], NS, t_rand)
    close(z, g["z"])
    pts = g["c2ws"][0][:3, 3].reshape(1, 1, 3) + z.unsqueeze(-1) * rd.unsqueeze(1)
    close(pts, g["pts"])
    nfe = {k_: v.expand(-1, NS).unsqueeze(-1) for k_, v in nf.items()}
    nfe["near"], nfe["far"] = g["near_fars"][0, 0], g["near_fars"][0, 1]
    ndc = O.get_ndc_coordinate(g["w2cs"][0], g["K"], pts, torch.tensor([W - 1, H - 1]), nfe)
    for k_, name in (("stage1", "ndc1"), ("stage2", "ndc2"), ("stage3", "ndc3"), ("ndc", "ndc")):
        close(ndc[k_], g[name], 1e-5, 1e-5)
