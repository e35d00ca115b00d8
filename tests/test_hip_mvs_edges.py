"""The four kernels of csrc/mvs.hip against the float64 oracle (tests/mvs_cases.py): bit for bit on the lattice cases -- hypotheses landing exactly
on x.5 / y.5, on gx, gy = +-1, past every border and behind the camera; both forward layouts (C <= 16: cost_volume_narrow_kernel, C > 16:
cost_volume_wide_kernel), volumes that end inside a block, a wave and a grid row; runs of equal source pixel at every position of the backward's
8 depth positions; one-, two-, four- and eight-hot depth distributions at every window edge -- and under a bar derived from the float32 oracle's
own error on the continuous cases.  No share of differing elements is allowed anywhere."""
import pytest
import torch

import mvs_cases as G
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


def same(got, want, what):
    got, want = got.detach().cpu(), want.float().reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, reference %r"
                             % (what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


# ------------------------------------------------------------------------------------------------ cost volume, lattice
@pytest.mark.parametrize("name", G.CV_LATTICE_NAMES)
def test_cost_volume_forward_is_exact(name):
    """Variance and count: class P against the float64 oracle, class Q against the float32 oracle (same operations in the same order) -- both bit
    for bit; the call without the count returns the same variance."""
    from uc_nerf_amd import ops
    case, cls, ref, ref32 = G.cv_lattice(name)
    want = ref if cls == "P" else ref32
    feats, proj, dv = f32(case["feats"]), f32(case["proj"]), f32(case["depth_values"])
    var_c, cnt = ops.cost_volume(feats, proj, dv, pad=case["pad"], want_count=True)
    var = ops.cost_volume(feats, proj, dv, pad=case["pad"])
    same(cnt, want[1], name + " count")
    same(var_c, want[0], name + " variance (with the count)")
    same(var, want[0], name + " variance")
    assert torch.equal(var, var_c)


@pytest.mark.parametrize("name", G.CV_LATTICE_NAMES)
def test_cost_volume_backward_is_exact_and_accumulates(name):
    """_CostVolumeFn's backward, twice into the same leaf.  Class P: the float64 gradient bit for bit, then exactly twice that.  Class Q (count =
    1/3, 1/5, ..: the products round): under bar(float32 oracle's distance), once and, against twice the reference, twice."""
    from uc_nerf_amd import ops
    case, cls, ref, ref32 = G.cv_lattice(name)
    feats = f32(case["feats"]).requires_grad_(True)
    proj, dv, g = f32(case["proj"]), f32(case["depth_values"]), f32(case["g_variance"])
    got = []
    for _ in range(2):
        ops.cost_volume(feats, proj, dv, pad=case["pad"]).backward(g)
        got.append(feats.grad.detach().cpu().clone())
    if cls == "P":
        same(got[0], ref[2], name + " g_feats")
        same(got[1], 2 * ref[2], name + " g_feats after a second backward")
        return
    oracle_d = (ref32[2].double() - ref[2]).abs().max().item()
    limit = G.bar(oracle_d, ref[2].abs().max().item())
    d1 = (got[0].double() - ref[2]).abs().max().item()
    d2 = (got[1].double() - 2 * ref[2]).abs().max().item()
    record("mvs_edges/" + name, g_feats=dict(device=d1, device_twice=d2, oracle_f32=oracle_d, bar=limit))
    assert d1 <= limit and d2 <= 2 * limit, "%s g_feats: %.3e (twice: %.3e) > bar %.3e (float32 oracle %.3e)" % (name, d1, d2, limit, oracle_d)


# ------------------------------------------------------------------------------------------------ depth regression, lattice
@pytest.mark.parametrize("name", G.DR_LATTICE_NAMES)
def test_depth_regress_forward_and_backward_are_exact(name):
    """Probabilities, depth, confidence, and the logits' gradient with g_depth alone, g_confidence alone and both -- border pixels of a padded
    plane included; prob_init, where given, receives the same gradient."""
    from uc_nerf_amd import ops
    case, ref = G.dr_lattice(name)
    dv, g_depth, g_conf = f32(case["depth_values"]), f32(case["g_depth"]), f32(case["g_confidence"])
    for mode in G.DR_MODES:
        x = f32(case["prob_pre"]).requires_grad_(True)
        init = f32(case["prob_init"])
        if init is not None:
            init.requires_grad_(True)
        prob, depth, conf = ops.depth_regress(x, dv, init, pad=case["pad"])
        want = ref[mode]
        same(prob, want[0], "%s prob_volume" % name)
        same(depth, want[1], "%s depth" % name)
        same(conf, want[2], "%s confidence" % name)
        loss = 0
        if mode in ("both", "depth"):
            loss = loss + (depth * g_depth).sum()
        if mode in ("both", "confidence"):
            loss = loss + (conf * g_conf).sum()
        loss.backward()
        same(x.grad, want[3], "%s g_prob_pre (%s)" % (name, mode))
        if init is not None:
            same(init.grad, want[4], "%s g_prob_init (%s)" % (name, mode))
            assert torch.equal(init.grad, x.grad)


# ------------------------------------------------------------------------------------------------ continuous cases
@pytest.mark.parametrize("name", G.CONTINUOUS_NAMES)
def test_continuous_case_within_four_times_the_float32_oracle(name):
    from uc_nerf_amd import ops
    case, ref, oracle_d, scale = G.continuous(name)
    got = {}
    feats = f32(case["feats"]).requires_grad_(True)
    proj, dv = f32(case["proj"]), f32(case["depth_values"])
    var_c, got["count"] = ops.cost_volume(feats, proj, dv, pad=case["pad"], want_count=True)
    got["variance"] = ops.cost_volume(feats, proj, dv, pad=case["pad"])
    assert torch.equal(got["variance"], var_c)
    got["variance"].backward(f32(case["g_variance"]))
    got["g_feats"] = feats.grad
    x = f32(case["prob_pre"]).requires_grad_(True)
    got["prob_volume"], got["depth"], got["confidence"] = ops.depth_regress(x, dv, f32(case["prob_init"]), pad=case["pad"])
    ((got["depth"] * f32(case["g_depth"])).sum() + (got["confidence"] * f32(case["g_confidence"])).sum()).backward()
    got["g_prob_pre"] = x.grad
    got = {k: v.detach().cpu() for k, v in got.items()}
    dist = G.distances(case, ref, got)
    rows = {k: dict(device=dist[k], oracle_f32=oracle_d[k], bar=G.bar(oracle_d[k], scale[k]), ratio=dist[k] / G.bar(oracle_d[k], scale[k])) for k in dist}
    # count off the excluded voxels: the float32 oracle's, bit for bit (1 / msum in float32; the host test ties its msum to the float64 one)
    keep = ~case["skip_voxel"]
    var32, count32, _ = G.cv_reference(case, G.F32)
    count_flips = int((got["count"] != count32)[keep].sum())
    # every voxel, the excluded ones included: where the device's variance is not the float32 oracle's beyond the bar, it picked another pixel
    index_differs = int(((got["variance"].double() - var32.double()).abs() > rows["variance"]["bar"]).any(0).sum())
    record("mvs_edges/" + name, excluded_voxels=case["excluded_voxels"], excluded_pixels=case["excluded_pixels"], count_flips=count_flips,
           voxels_off_the_float32_oracle=index_differs, **rows)
    fails = ["%s %s: %.3e > bar %.3e (float32 oracle %.3e)" % (name, k, r["device"], r["bar"], r["oracle_f32"]) for k, r in rows.items()
             if not r["device"] <= r["bar"]]
    if count_flips:
        fails.append("%s: %d counts differ outside the excluded set" % (name, count_flips))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ refusals
def test_sizes_the_kernels_do_not_serve_are_refused():
    """The host checks of mvs.hip answer before any launch: 129 hypotheses (the LDS copy holds 128), 9 views (registers and LDS for 8), a map
    one pixel wide (W - 1 = 0 divides the normalised coordinate)."""
    from uc_nerf_amd import ops
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    with pytest.raises(RuntimeError, match=r"depth_regress: bad sizes D=129 \(max 128\)"):
        ops.depth_regress(z(129, 3, 4), z(129, 3, 4) + 1)
    with pytest.raises(RuntimeError, match=r"cost_volume: V = 9 outside 1\.\.8"):
        ops.cost_volume(z(9, 2, 3, 4), z(9, 3, 4), z(2, 3, 4) + 1)
    with pytest.raises(RuntimeError, match=r"cost_volume: bad sizes C=2 H=3 W=1 D=2 pad=0"):
        ops.cost_volume(z(1, 2, 3, 1), z(1, 3, 4), z(2, 3, 1) + 1)
    torch.cuda.synchronize()
    # the sizes next to them are served
    assert ops.depth_regress(z(128, 3, 4), z(128, 3, 4) + 1)[0].shape == (128, 3, 4)
    assert ops.cost_volume(z(8, 2, 3, 2), torch.eye(3, 4, device=DEV).repeat(8, 1, 1), z(2, 3, 2) + 1).shape == (2, 2, 3, 2)
    torch.cuda.synchronize()
