"""The cascade link on the GPU: ucnerf_depth_hypotheses against the torch restatement of the reference's op chain (tests/cascade_stubs.py, pinned
to fixture G19 by tests/test_cascade_host.py), the get_*depth_range_samples mirrors against G19, and the CascadeMVSNet mirror end to end.

Bar for every hypothesis value: |got - want| <= 16 * 2^-23 * far, absolute, no element excluded (cascade_stubs.bar).
Run on the GPU box:  python -m pytest tests/test_hip_cascade.py -m gpu -q -s   (prints the measured maxima)
"""
import pytest
import torch

import cascade_stubs as S
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEAR, FAR = 2.0, 11.0

# cur_depth, intermediate (H, W), output (h, w), D, ratio (interval_pixel = ratio * (far - near) / 48), pad
MAP_CASES = {
    "stage2_shape": ((8, 10), (32, 40), (16, 20), 32, 2, 0),
    "stage3_shape_identity_pad2": ((16, 20), (32, 40), (32, 40), 8, 1, 2),
    "no_multiple_of_anything": ((5, 7), (20, 28), (10, 14), 4, 1, 0),
    "rows_narrower_than_a_wave": ((6, 6), (24, 24), (6, 6), 48, 4, 0),
    "non_integer_ratio": ((9, 11), (32, 40), (8, 10), 5, 3, 1),
}
CLAMPS_MUST_BE_PARTIAL = ("stage2_shape", "stage3_shape_identity_pad2")


def ops():
    from uc_nerf_amd import ops as _ops
    return _ops


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_cascade")


@pytest.fixture(scope="module")
def map_refs():
    """Inputs and the CPU reference of every map-mode case, computed once."""
    near, far = torch.tensor(NEAR), torch.tensor(FAR)
    refs = {}
    for i, (name, (hw0, HW, hw, D, ratio, pad)) in enumerate(MAP_CASES.items()):
        cur = NEAR + (FAR - NEAR) * torch.rand(*hw0, generator=torch.Generator().manual_seed(190 + i))
        want, (lo, hi, c) = S.hypotheses_chain(cur, near, far, ratio * ((far - near) / 48), D, HW, hw, pad)
        half = D / 2 * ratio * ((FAR - NEAR) / 48)
        refs[name] = (cur, want, (c - half < NEAR).float().mean().item(), (c + half > FAR).float().mean().item())
    return refs


@pytest.mark.parametrize("name", list(MAP_CASES))
def test_map_mode_against_the_restated_chain(name, map_refs):
    hw0, HW, hw, D, ratio, pad = MAP_CASES[name]
    cur, want, lo_share, hi_share = map_refs[name]
    if name in CLAMPS_MUST_BE_PARTIAL:                    # each clamp active on more than none and fewer than all pixels
        assert 0.0 < lo_share < 1.0 and 0.0 < hi_share < 1.0, (lo_share, hi_share)
    nf = torch.tensor([NEAR, FAR], device=DEV)
    got = ops().depth_hypotheses(D, hw, cur_depth=dev(cur), near_far=nf, k=ratio / 48.0, full_hw=HW, pad=pad)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (D, hw[0] + 2 * pad, hw[1] + 2 * pad)
    err = (got.cpu() - want).abs().max().item()
    print("\n%s: max |err| = %.3e = %.2f * 2^-23 * far (bar 16); clamp shares near %.3f far %.3f" % (name, err, err / (2.0 ** -23 * FAR), lo_share, hi_share))
    assert err <= S.bar(FAR)
    if pad:                                               # the border repeats the edge value, bit for bit
        inner = got[:, pad:-pad, pad:-pad]
        assert torch.equal(got, torch.nn.functional.pad(inner.unsqueeze(0), (pad,) * 4, "replicate")[0])
    again = ops().depth_hypotheses(D, hw, cur_depth=dev(cur), near_far=nf, k=ratio / 48.0, full_hw=HW, pad=pad)
    assert torch.equal(got, again)                        # repeatability: two launches are bit-identical


@pytest.mark.parametrize("pad", [0, 1])
def test_row_mode(pad):
    row = torch.linspace(NEAR, FAR, 48)
    want = S.row_chain(row, 48, (8, 10), pad)
    got = ops().depth_hypotheses(48, (8, 10), row=dev(row), pad=pad)
    assert got.shape == want.shape == (48, 8 + 2 * pad, 10 + 2 * pad)
    err = (got.cpu() - want).abs().max().item()
    print("\nrow mode pad %d: max |err| = %.3e" % (pad, err))
    assert err <= S.bar(FAR)
    assert torch.equal(got, ops().depth_hypotheses(48, (8, 10), row=dev(row), pad=pad))
    # a row of another length than D: only its two ends count
    got2 = ops().depth_hypotheses(48, (8, 10), row=torch.tensor([NEAR, FAR], device=DEV), pad=pad)
    assert torch.equal(got2, got)


def test_empty_output_and_bad_arguments():
    nf = torch.tensor([NEAR, FAR], device=DEV)
    cur = torch.rand(4, 5, device=DEV)
    assert ops().depth_hypotheses(8, (0, 5), cur_depth=cur, near_far=nf, k=1 / 48, full_hw=(8, 10)).shape == (8, 0, 5)
    with pytest.raises(RuntimeError, match="D = 1"):
        ops().depth_hypotheses(1, (4, 5), cur_depth=cur, near_far=nf, k=1 / 48)
    with pytest.raises(RuntimeError, match="must cover"):
        ops().depth_hypotheses(8, (9, 10), cur_depth=cur, near_far=nf, k=1 / 48, full_hw=(8, 10))


def test_full_resolution_mirrors_match_the_reference_fixture(g19):
    from uc_nerf_amd.network import mvs_models as M
    g = g19
    cur = dev(g["map_cur_depth"])
    got = M.get_depth_range_samples(cur, g["map_ndepth"], g["map_interval"], cur.device, cur.dtype, list(cur.shape), max_depth=g["map_far"], min_depth=g["map_near"])
    direct = M.get_cur_depth_range_samples(cur, g["map_ndepth"], dev(torch.tensor(g["map_interval"])), list(cur.shape), dev(torch.tensor(g["map_far"])),
                                           dev(torch.tensor(g["map_near"])))            # (scalars as device tensors, as CascadeMVSNet.forward hands them over)
    assert got.shape == g["map_samples"].shape and torch.equal(got, direct)
    e_map = (got.cpu() - g["map_samples"]).abs().max().item()
    row = dev(g["row_in"])
    got_row = M.get_depth_range_samples(row, g["row_ndepth"], g["map_interval"], row.device, row.dtype, [1] + list(g["row_samples"].shape[2:]))
    assert got_row.shape == g["row_samples"].shape
    e_row = (got_row.cpu() - g["row_samples"]).abs().max().item()
    print("\nfull-resolution mirrors against G19: max |err| map %.3e, row %.3e (bar %.3e)" % (e_map, e_row, S.bar(g["map_far"])))
    assert e_map <= S.bar(g["map_far"]) and e_row <= S.bar(g["map_far"])


@pytest.fixture(scope="module")
def cascade_run(g19):
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    g = g19
    feature, regs = S.make_stubs(g["V"], g["H"], g["W"], [g["logits%d" % k] for k in (1, 2, 3)], seed=g["feature_seed"])
    net = CascadeMVSNet(feature=feature, cost_regularization=regs).to(DEV)
    with torch.no_grad():
        result = net(dev(g["imgs"]), dev(g["affine_mat"]), dev(g["affine_mat_inv"]), dev(g["near_far"]), pad=g["pad"])
    torch.cuda.synchronize()
    return result


def test_cascade_mirror_end_to_end_against_the_reference_fixture(g19, cascade_run):
    g = g19
    vol, conf, depth, outputs = cascade_run
    far = g["near_far"][1].item()
    bar = S.bar(far)
    for k in (1, 2, 3):
        o = outputs["stage%d" % k]
        e_dv = (o["depth_values"][0].cpu() - g["depth_values%d" % k]).abs().max().item()
        e_d = (o["depth"][0].cpu() - g["depth%d" % k]).abs().max().item()
        bad = ((o["photometric_confidence"][0].cpu() - g["confidence%d" % k]).abs() > 2e-6).float().mean().item()
        print("\nstage %d: max |err| depth_values %.3e (bar %.3e), depth %.3e, confidence differs on %.4f of the pixels" % (k, e_dv, bar, e_d, bad))
        assert e_dv <= bar
        # depth is a convex combination of the hypotheses: their bar plus the depth regression's own tolerance (G13: 2e-6 absolute and relative)
        torch.testing.assert_close(o["depth"][0].cpu(), g["depth%d" % k], atol=bar + 2e-6, rtol=2e-6)
        # the confidence reads the 4-tap window at floor(E[d]): an expectation within rounding of an integer may take either (as G13 allows)
        assert bad < 5e-3
    assert S.outputs_listing(outputs) == list(g["outputs_listing"])
    s3 = outputs["stage3"]
    assert vol is s3["volume_feature_no_ref"] and conf is s3["photometric_confidence"] and depth is s3["depth"]
    assert outputs["depth_values"] is s3["depth_values"] and outputs["depth"] is depth


def test_cascade_mirror_takes_near_far_from_the_host_too_and_detaches_between_stages(g19, cascade_run):
    """near_far as the CPU tensor / pair of numbers a caller may hold gives the same volumes; under autograd the regulariser's logits get gradients
    through depth and confidence while the hypotheses themselves carry none."""
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    g = g19
    feature, regs = S.make_stubs(g["V"], g["H"], g["W"], [g["logits%d" % k] for k in (1, 2, 3)], seed=g["feature_seed"])
    net = CascadeMVSNet(feature=feature, cost_regularization=regs).to(DEV)
    lg = torch.nn.Parameter(dev(g["logits3"]).clone())
    net.cost_regularization[2].logits = lg
    _, conf, depth, outputs = net(dev(g["imgs"]), dev(g["affine_mat"]), dev(g["affine_mat_inv"]), (float(g["near_far"][0]), float(g["near_far"][1])), pad=g["pad"])
    for k in (1, 2, 3):
        assert torch.equal(outputs["stage%d" % k]["depth_values"], cascade_run[3]["stage%d" % k]["depth_values"])
        assert not outputs["stage%d" % k]["depth_values"].requires_grad
    (depth.sum() + conf.sum()).backward()
    assert lg.grad is not None and torch.isfinite(lg.grad).all() and lg.grad.abs().sum() > 0


def test_outputs_feed_the_test_time_ray_builder(g19, cascade_run):
    """The padded depth_values have the shapes uc_nerf_amd.utils.utils.build_rays_test expects: one chunk goes through."""
    from uc_nerf_amd.utils import utils as U
    g = g19
    outputs = cascade_run[3]
    H, W, pad, n_samples, chunk = g["H"], g["W"], g["pad"], 9, 256
    K = torch.tensor([[0.9 * W, 0, 0.5 * W], [0, 0.9 * W, 0.5 * H], [0, 0, 1]], device=DEV)
    c2w = torch.eye(4, device=DEV)
    nf = dev(g["near_far"]).view(1, 2)
    pts, rays_dir, ndc, z, rays_o, ndc_parameters = U.build_rays_test(H, W, c2w, torch.eye(4, device=DEV), K, nf, nf[-1], n_samples, pad=pad, chunk=chunk, idx=1,
                                                                      outputs=outputs)
    torch.cuda.synchronize()
    assert pts.shape == (chunk, n_samples, 3) and z.shape == (chunk, n_samples) and rays_dir.shape == (chunk, 3)
    assert set(ndc) == {"stage1", "stage2", "stage3", "ndc"} and all(v.shape == (chunk, n_samples, 3) for v in ndc.values())
    assert torch.isfinite(pts).all() and torch.isfinite(z).all()
