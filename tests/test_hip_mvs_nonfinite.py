"""The five kernels of csrc/mvs.hip on non-finite depths, logits, features and upstream gradients (tests/mvs_nonfinite_cases.py; its host test
proves the cases): NaN, +inf and -inf land exactly where torch's float32 ops put them on the CPU; every element outside the set predicted from the
geometry keeps the bits of the same call on the clean input (g_feats, an unordered sum of atomics: the existing bar of mvs_cases, exact on the
lattice); finite values inside the set are held to float64 under mvs_cases.bar; a second call into dirty buffers gives the same bits; and one stage
in one piece -- hypotheses, cost volume, a pointwise regulariser, regression -- keeps a NaN and a -inf of the incoming depth map to their pixels."""
import pytest
import torch

import cascade_edge_cases as E
import cascade_stubs as S
import mvs_cases as G
import mvs_nonfinite_cases as N
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_pattern(got, want32, what):
    a, b = N.classes(got), N.classes(want32.reshape(got.shape))
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError("%s: %d of %d entries are not of torch's class (0 finite, 1 NaN, 2 +inf, 3 -inf), first at %s: device %r (class %d), torch %r"
                             % (what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), a[tuple(bad[0])].item(), want32.reshape(got.shape)[tuple(bad[0])].item()))


def same_bits_outside(got, clean, inside, what):
    moved = (bits(got) != bits(clean)) & ~inside.reshape(got.shape)
    assert not moved.any(), "%s: %d elements outside the predicted set are not the clean call's, first at %s" % (what, int(moved.sum()), moved.nonzero()[0].tolist())


def held_inside(name, key, got, r64, r32, inside, rows):
    """Finite values of the predicted set against float64 under mvs_cases.bar (4 x the float32 restatement's own distance + 1e-6 of the scale)."""
    limit, own, keep = N.finite_bar(r64, r32, inside.reshape(r64.shape))
    if not keep.any():
        return
    d = (got.double().reshape(r64.shape) - r64)[keep].abs().max().item()
    rows[key] = dict(device=d, oracle_f32=own, bar=limit, ratio=d / limit, elements=int(keep.sum()))
    assert d <= limit, "%s %s: %.3e > bar %.3e on %d finite elements of the poisoned set (float32 restatement %.3e)" % (name, key, d, limit, int(keep.sum()), own)


# ------------------------------------------------------------------------------------------------ cost volume
def run_cv(case):
    """variance, count (one launch with the count, one without) and g_feats of one backward -> CPU tensors."""
    from uc_nerf_amd import ops
    feats = dev(case["feats"]).requires_grad_(True)
    proj, dv = dev(case["proj"]), dev(case["depth_values"])
    var_c, cnt = ops.cost_volume(feats, proj, dv, pad=case["pad"], want_count=True)
    var = ops.cost_volume(feats, proj, dv, pad=case["pad"])
    assert torch.equal(bits(var), bits(var_c))
    var.backward(dev(case["g_variance"]))
    return dict(variance=var.detach().cpu(), count=cnt.cpu(), g_feats=feats.grad.cpu())


_CV_CLEAN = {}


def cv_clean_run(case):
    base = case["clean"]
    if base["name"] not in _CV_CLEAN:
        _CV_CLEAN[base["name"]] = run_cv(base)
    return _CV_CLEAN[base["name"]]


@pytest.mark.parametrize("name", N.CV_NAMES)
def test_cost_volume_forward_and_backward_on_a_poisoned_case(name):
    case, r64, r32, predicted = N.cv_case(name)
    got, clean = run_cv(case), cv_clean_run(case)
    rows = {}
    for k in G.CV_OUTPUTS:
        same_pattern(got[k], r32[k], "%s %s" % (name, k))
    for k in ("variance", "count"):
        same_bits_outside(got[k], clean[k], predicted[k], "%s %s" % (name, k))
        held_inside(name, k, got[k], r64[k], r32[k], predicted[k], rows)
    # g_feats: atomics in an unordered sum.  Outside the predicted cells: exact where the float32 restatement is the float64 one (the lattice's
    # class P), under the bar of test_hip_mvs_edges elsewhere; inside: the finite cells under the same rule
    out = ~predicted["g_feats"]
    assert torch.isfinite(got["g_feats"][out]).all()
    if torch.equal(r32["g_feats"][out].double(), r64["g_feats"][out]):
        assert torch.equal(got["g_feats"][out].double(), r64["g_feats"][out]), "%s g_feats outside the predicted cells is not the exact gradient" % name
        rows["g_feats_outside"] = "exact"
    else:
        own = (r32["g_feats"].double() - r64["g_feats"])[out].abs().max().item()
        limit = G.bar(own, r64["g_feats"][torch.isfinite(r64["g_feats"])].abs().max().item())
        d = (got["g_feats"].double() - r64["g_feats"])[out].abs().max().item()
        rows["g_feats_outside"] = dict(device=d, oracle_f32=own, bar=limit, ratio=d / limit)
        assert d <= limit, "%s g_feats outside the predicted cells: %.3e > bar %.3e" % (name, d, limit)
    held_inside(name, "g_feats", got["g_feats"], r64["g_feats"], r32["g_feats"], predicted["g_feats"], rows)
    record("mvs_nonfinite/" + name, **rows)


def test_maps_one_pixel_wide_or_high_are_refused():
    """sx = (W - 1) / 2 = 0 would make every gx +-inf or NaN: the entry point answers before any launch."""
    from uc_nerf_amd import ops
    for (H, W), text in N.REFUSED_SIZES.values():
        with pytest.raises(RuntimeError, match=text):
            ops.cost_volume(torch.zeros(1, 3, H, W, device=DEV), torch.zeros(1, 3, 4, device=DEV), torch.full((9, H, W), float("nan"), device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ depth regression
def run_dr(case):
    """The five outputs through ops.depth_regress and autograd (ucnerf_depth_regress, _bwd, _bwd_values) -> CPU tensors."""
    from uc_nerf_amd import ops
    x, dv, init = dev(case["prob_pre"]).requires_grad_(True), dev(case["depth_values"]).requires_grad_(True), dev(case["prob_init"])
    if init is not None:
        init.requires_grad_(True)
    prob, depth, conf = ops.depth_regress(x, dv, init, pad=case["pad"])
    torch.autograd.backward([depth, conf], [dev(case["g_depth"]), dev(case["g_confidence"])])
    if init is not None:
        assert torch.equal(bits(init.grad), bits(x.grad))
    return dict(prob_volume=prob.detach().cpu(), depth=depth.detach().cpu(), confidence=conf.detach().cpu(), g_prob_pre=x.grad.cpu(), g_depth_values=dv.grad.cpu())


_DR_CLEAN = {}


def dr_clean_run(case):
    base = case["clean"]
    if base["name"] not in _DR_CLEAN:
        _DR_CLEAN[base["name"]] = run_dr(base)
    return _DR_CLEAN[base["name"]]


@pytest.mark.parametrize("name", N.DR_NAMES)
def test_depth_regress_forward_and_backward_on_a_poisoned_case(name):
    case, r64, r32, predicted = N.dr_case(name)
    got, clean = run_dr(case), dr_clean_run(case)
    rows = {}
    for k in N.DR_OUTPUTS:
        same_pattern(got[k], r32[k], "%s %s" % (name, k))
    for k in N.DR_OUTPUTS:
        same_bits_outside(got[k], clean[k], predicted[k], "%s %s" % (name, k))
        held_inside(name, k, got[k], r64[k], r32[k], predicted[k], rows)
    record("mvs_nonfinite/" + name, **rows)


# ------------------------------------------------------------------------------------------------ nothing kept between calls
@pytest.mark.parametrize("name", ("cv/narrow_v3_pad1/depth_nan/last_voxel", "cv/wide_v8_pad1/depth_+0/border_voxel", "cv/wide_v3_pad0/feats_+inf/pixel0",
                                  "cv/narrow_v1_pad1/g_variance_+inf"))
def test_second_cost_volume_call_into_the_same_dirty_buffers_gives_the_same_bits(name):
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.ops import mvs as OM
    assert name in N.CV_NAMES
    case = N.cv_case(name)[0]
    fresh = run_cv(case)
    feats, proj, dv, g = dev(case["feats"]), dev(case["proj"]), dev(case["depth_values"]), dev(case["g_variance"])
    var, cnt = torch.full(tuple(g.shape), 7.0, device=DEV), torch.full(tuple(dv.shape), 7.0, device=DEV)
    p = OM._cost_volume_params(feats, proj, dv, case["pad"])
    p.variance, p.count = var.data_ptr(), cnt.data_ptr()
    for i in range(2):
        OM._launch("ucnerf_cost_volume", p, feats.device)
        assert torch.equal(bits(var.cpu()), bits(fresh["variance"])) and torch.equal(bits(cnt.cpu()), bits(fresh["count"])), "%s, call %d" % (name, i)
        var.add_(1.0)                                                        # (stale values of another call in every output, NaN slots included)
        cnt.add_(1.0)
    bp = L.CostVolumeBwdParams()
    bp.fwd = OM._cost_volume_params(feats, proj, dv, case["pad"])
    g_feats = torch.zeros_like(feats)
    bp.g_variance, bp.g_feats = g.data_ptr(), g_feats.data_ptr()
    for i in range(2):                                                       # accumulated into: the same classes after one call and after two
        OM._launch("ucnerf_cost_volume_bwd", bp, feats.device)
        assert torch.equal(N.classes(g_feats.cpu()), N.classes(fresh["g_feats"])), "%s g_feats, call %d" % (name, i)


@pytest.mark.parametrize("name", ("dr/d4_pad0/prob_pre_nan/d0/pixel0", "dr/d17_pad1/depth_values_+inf", "dr/d9_pad1/g_confidence_-inf", "dr/d17_pad1/g_depth_nan"))
def test_second_regression_call_into_the_same_dirty_buffers_gives_the_same_bits(name):
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.ops import mvs as OM
    assert name in N.DR_NAMES
    case = N.dr_case(name)[0]
    fresh = run_dr(case)
    x, dv, init = dev(case["prob_pre"]), dev(case["depth_values"]), dev(case["prob_init"])
    g_depth, g_conf = dev(case["g_depth"]), dev(case["g_confidence"])
    out = {k: torch.full(tuple(fresh[k].shape), 7.0, device=DEV) for k in N.DR_OUTPUTS}
    p = OM._depth_regress_params(x, init, dv, case["pad"])
    p.prob_volume, p.depth, p.confidence = (out[k].data_ptr() for k in N.DR_FWD)
    bp = L.DepthRegressBwdParams()
    prob = dev(fresh["prob_volume"])
    bp.fwd = OM._depth_regress_params(prob, None, dv, case["pad"])
    bp.fwd.prob_volume = prob.data_ptr()
    bp.g_depth, bp.g_confidence, bp.g_prob_pre = g_depth.data_ptr(), g_conf.data_ptr(), out["g_prob_pre"].data_ptr()
    vp = L.DepthRegressBwdValuesParams()
    vp.D, vp.Hp, vp.Wp, vp.pad = case["D"], case["Hp"], case["Wp"], case["pad"]
    vp.prob_volume, vp.g_depth, vp.g_depth_values = prob.data_ptr(), g_depth.data_ptr(), out["g_depth_values"].data_ptr()
    for i in range(2):
        OM._launch("ucnerf_depth_regress", p, x.device)
        OM._launch("ucnerf_depth_regress_bwd", bp, x.device)
        OM._launch("ucnerf_depth_regress_bwd_values", vp, x.device)
        for k, v in out.items():
            assert torch.equal(bits(v.cpu()), bits(fresh[k])), "%s %s, call %d into the caller's buffers" % (name, k, i)
            v.add_(1.0)


# ------------------------------------------------------------------------------------------------ a stage in one piece
def test_one_stage_keeps_a_nan_and_a_minus_inf_of_the_incoming_depth_to_their_pixels():
    """ucnerf_depth_hypotheses -> ucnerf_cost_volume -> cascade_stubs.RegStub's rule (fixed logits + 0.0 * variance channel 0) ->
    ucnerf_depth_regress against the same chain in torch on the CPU (cascade_stubs.hypotheses_chain, mvs_nonfinite_cases.cv_restatement,
    oracle depth_regress): depth, confidence and prob_volume are non-finite at exactly torch's pixels, every other pixel has the clean run's bits."""
    from uc_nerf_amd import ops
    hw0, HW, hw, D, pad, ratio = E.NONFINITE["integer_ratio_pad1"]
    gen = torch.Generator().manual_seed(7500)
    near, far, k = E.C_NEAR, E.C_FAR, ratio / 48.0
    clean_cur = near + (far - near) * torch.rand(*hw0, generator=gen)
    cur = clean_cur.clone()
    cur[1, 2], cur[4, 6] = float("nan"), float("-inf")
    V, C = 3, 8
    feats = torch.randn(V, C, *hw, generator=gen)
    proj = G.lattice_proj([0, 1, 2], *hw).float()
    logits = torch.randn(D, hw[0] + 2 * pad, hw[1] + 2 * pad, generator=gen)

    def on_cpu(c):
        dv = S.hypotheses_chain(c, torch.tensor(near), torch.tensor(far), torch.tensor(k) * (torch.tensor(far) - torch.tensor(near)), D, HW, hw, pad)[0]
        case = dict(feats=feats, proj=proj, depth_values=dv, pad=pad, g_variance=torch.zeros(C, *dv.shape))
        var = N.cv_restatement(case, N.F32)["variance"]
        return N.M.depth_regress(logits + 0.0 * var[0], dv, None, pad)

    def on_device(c):
        dv = ops.depth_hypotheses(D, hw, cur_depth=c.to(DEV), near_far=torch.tensor([near, far], device=DEV), k=k, full_hw=HW, pad=pad)
        var = ops.cost_volume(feats.to(DEV), proj.to(DEV), dv, pad=pad)
        return [t.detach().cpu() for t in ops.depth_regress(logits.to(DEV) + 0.0 * var[0], dv, None, pad=pad)]

    want, got, clean = on_cpu(cur), on_device(cur), on_device(clean_cur)
    touched = 0
    for k_, w, g, c in zip(N.DR_FWD, want, got, clean):
        same_pattern(g, w, "stage " + k_)
        bad = N.classes(w) != 0
        touched += int(bad.sum())
        assert torch.equal(bits(g)[~bad], bits(c)[~bad]), "stage %s: a pixel torch keeps finite is not the clean run's" % k_
    assert touched and torch.isfinite(torch.stack([t.sum() for t in clean])).all()
