"""The non-finite cases of tests/mvs_nonfinite_cases.py are what they claim -- on the CPU, before any kernel sees them: the float32 and the float64
restatement put NaN, +inf and -inf at the same positions (a case where they do not has no single right answer and is listed in N.REMOVED), the
poison is visible, it stays inside the set predicted from the geometry, and every (kind, site) pair of the lists survives the removal rule."""
import pytest
import torch

import mvs_cases as G
import mvs_nonfinite_cases as N


def _pixels(mask):
    return mask.reshape(-1, *mask.shape[-2:]).any(0) if mask.dim() > 2 else mask


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("layout", N.CV_LAYOUTS)
@pytest.mark.parametrize("pad", (0, 1))
def test_grid_sample_restatement_is_the_pinned_oracle_on_clean_inputs(layout, pad):
    """cv_restatement (F.grid_sample) == oracle.mvs_oracle.cost_volume_variance (index arithmetic, pinned by fixture g12) == cv_explicit, bit for bit."""
    case = N.cv_clean(layout, pad)
    for dtype in (N.F64, N.F32):
        want = dict(zip(G.CV_OUTPUTS, G.cv_reference(case, dtype)))
        got, explicit = N.cv_restatement(case, dtype), N.cv_explicit(case, dtype)
        for k in G.CV_OUTPUTS:
            assert torch.equal(got[k], want[k].reshape(got[k].shape)), (layout, pad, dtype, k)
        assert torch.equal(explicit["variance"], got["variance"]) and torch.equal(explicit["count"], got["count"])


def test_the_padded_volume_ends_inside_a_block_of_both_layouts():
    total = N.CV_D * (N.HW[0] + 2) * (N.HW[1] + 2)
    assert total == 693 and total % 32 and total % 256 and (N.CV_D * N.HW[0] * N.HW[1]) % 32


# ------------------------------------------------------------------------------------------------ cost volume
@pytest.mark.parametrize("name", list(N.CV_SPECS))
def test_cost_volume_case(name):
    removed = name in N.REMOVED
    fn, args = N.CV_SPECS[name]
    case = fn(*args)
    r64, r32, predicted = N.cv_restatement(case, N.F64), N.cv_restatement(case, N.F32), N.cv_predicted(case)
    assert (N.patterns_agree(r64, r32) != []) == removed, "%s: float32 and float64 patterns differ on %s" % (name, N.patterns_agree(r64, r32))
    if removed:
        return
    c64, c32 = N.cv_clean_reference(case)
    for ref, clean, dtype in ((r64, c64, N.F64), (r32, c32, N.F32)):
        # the geometry's own prediction of the forward: index arithmetic with NaN -> 0, a plain gather
        explicit = N.cv_explicit(case, dtype)
        for k in ("variance", "count"):
            assert not N.changed(ref[k], explicit[k]).any(), "%s %s: grid_sample and the index rule differ" % (name, k)
        moved = {k: N.changed(ref[k], clean[k]) for k in G.CV_OUTPUTS}
        for k in G.CV_OUTPUTS:                          # contained
            assert not (moved[k] & ~predicted[k]).any(), "%s %s: %d elements outside the predicted set changed" % (name, k, int((moved[k] & ~predicted[k]).sum()))
        assert any(bool(m.any()) for m in moved.values()), "%s: the poison is not visible" % name
        if case["poison"][0] == "feats":                # NaN / inf - inf = NaN on every voxel that lands on the pixel; count untouched
            assert torch.equal(moved["variance"], predicted["variance"]) and torch.isnan(ref["variance"][predicted["variance"]]).all()
            assert not moved["count"].any()
        if case["poison"][0] == "g_variance":
            assert not moved["variance"].any() and not moved["count"].any() and moved["g_feats"].any()
            assert (N.classes(ref["g_feats"])[moved["g_feats"]] != 0).all()
    assert torch.isfinite(r32["count"]).all()
    if case["poison"][0] == "depth":                    # a poisoned depth moves a lookup, it never makes a value non-finite
        assert all(torch.isfinite(r32[k]).all() for k in G.CV_OUTPUTS)


def test_every_cost_volume_kind_and_site_survives():
    alive = [N.CV_SPECS[n][1] for n in N.CV_NAMES if N.CV_SPECS[n][0] is N.cv_depth_case]
    for kind in N.CV_KINDS:
        for site in N.CV_SITES:
            for family in ("narrow", "wide"):
                assert any(a[2] == kind and a[3] == site and a[0].startswith(family) for a in alive), (kind, site, family)
    for layout in N.CV_LAYOUTS:
        assert {a[1] for a in alive if a[0] == layout} == {0, 1}, layout
    feats = [N.CV_SPECS[n][1] for n in N.CV_NAMES if N.CV_SPECS[n][0] is N.cv_feat_case]
    assert {(a[0], a[2], a[3]) for a in feats} == {(lay, k, p) for lay in N.CV_LAYOUTS for k in N.FEAT_KINDS for p in N.FEAT_PIXELS}
    grads = [N.CV_SPECS[n][1] for n in N.CV_NAMES if N.CV_SPECS[n][0] is N.cv_grad_case]
    assert {(a[0], a[2]) for a in grads} == {(lay, k) for lay in N.CV_LAYOUTS for k in ("nan", "+inf")}


def test_zero_over_zero_occurs():
    """View 6 of the lattice has T = 0 in every row: at a depth of 0 its T / depth is 0 / 0 in all three."""
    names = [n for n in N.CV_NAMES if N.CV_SPECS[n][0] is N.cv_depth_case and N.CV_SPECS[n][1][2] in ("+0", "-0") and 6 in N.CV_LAYOUTS[N.CV_SPECS[n][1][0]]["views"]]
    assert names
    case = N.cv_case(names[0])[0]
    v = N.CV_LAYOUTS[N.CV_SPECS[names[0]][1][0]]["views"].index(6)
    assert (case["proj"][v, :, 3] == 0).all() and (case["depth_values"] == 0).any()
    q = case["proj"][v, :, 3:].float() / case["depth_values"].float().reshape(1, -1)
    assert torch.isnan(q).all(0).any()


def test_a_nan_coordinate_lands_on_pixel_0_and_inf_on_the_clamped_ends():
    for name in N.CV_NAMES:
        fn, args = N.CV_SPECS[name]
        if fn is N.cv_depth_case and args[2] in ("nan", "+0", "-0"):
            case = N.cv_case(name)[0]
            idx, inside = N.cv_index(case, N.F32)
            hit = case["voxels"].reshape(-1)
            assert (idx[:, hit] == 0).all() and not inside[:, hit].any(), name


# ------------------------------------------------------------------------------------------------ depth regression
@pytest.mark.parametrize("name", list(N.DR_SPECS))
def test_depth_regress_case(name):
    removed = name in N.REMOVED
    fn, args = N.DR_SPECS[name]
    case = fn(*args)
    r64, r32, predicted = N.dr_restatement(case, N.F64), N.dr_restatement(case, N.F32), N.dr_predicted(case)
    assert (N.patterns_agree(r64, r32) != []) == removed, "%s: float32 and float64 patterns differ on %s" % (name, N.patterns_agree(r64, r32))
    if removed:
        return
    shape = name.split("/")[1]
    for ref, clean in zip((r64, r32), N.dr_clean_reference(shape)):
        moved = {k: N.changed(ref[k], clean[k]) for k in N.DR_OUTPUTS}
        for k in N.DR_OUTPUTS:
            assert not (moved[k] & ~predicted[k]).any(), "%s %s: %d elements outside the predicted set changed" % (name, k, int((moved[k] & ~predicted[k]).sum()))
        assert any(bool(m.any()) for m in moved.values()), "%s: the poison is not visible" % name
        what = case["poison"][0]
        if what == "logits":                            # the whole row is renormalised (or NaN)
            assert torch.equal(moved["prob_volume"], predicted["prob_volume"])
            assert torch.equal(moved["depth"], predicted["depth"])
        if what == "depth_values":
            assert torch.equal(moved["depth"], predicted["depth"]) and not torch.isfinite(ref["depth"][predicted["depth"]]).any()
        if what == "g_confidence":                      # the clamp passes the gradient by a margin no rounding crosses
            assert (ref["confidence"][predicted["g_prob_pre"][0][case["pad"]:case["Hp"] - case["pad"], case["pad"]:case["Wp"] - case["pad"]]] < 1 - 1e-3).all()
        if what in ("g_depth", "g_confidence"):
            assert moved["g_prob_pre"].any() and (N.classes(ref["g_prob_pre"])[moved["g_prob_pre"]] != 0).all()
    # the window decision of the finite pixels inside the poisoned set is not next to an integer (float64)
    p = r64["prob_volume"]
    e = (p * torch.arange(case["D"], dtype=N.F64).view(-1, 1, 1)).sum(0)[case["pixels"]]
    e = e[torch.isfinite(e)]
    assert ((e - e.round()).abs() > 1e-4).all(), name


def test_every_regression_kind_and_site_survives():
    alive = [N.DR_SPECS[n][1] for n in N.DR_NAMES if N.DR_SPECS[n][0] is N.dr_logit_case]        # (shape, kind, depth_site, pixel_site, target)
    for kind in N.DR_KINDS:
        for site in N.DR_PIXEL_SITES:
            assert any(a[1] == kind and a[3] == site for a in alive), (kind, site)
        if kind != "-inf_all":
            for site in N.DR_DEPTH_SITES:
                assert any(a[1] == kind and a[2] == site for a in alive), (kind, site)
        assert any(a[1] == kind and a[4] == "prob_init" for a in alive) and any(a[1] == kind and a[4] == "prob_pre" for a in alive), kind
        assert {N.DR_SHAPES[a[0]][0] for a in alive if a[1] == kind} == {4, 9, 17}, kind
    names = set(N.DR_NAMES)
    assert {"dr/%s/depth_values_%s" % (s, k) for s in ("d9_pad0", "d17_pad1") for k in N.DV_KINDS} <= names
    assert {"dr/d17_pad1/g_depth_nan", "dr/d9_pad0/g_depth_+inf", "dr/d4_pad0/g_confidence_nan", "dr/d9_pad1/g_confidence_+inf"} <= names


def test_the_last_block_of_every_plane_is_partial():
    for shape in N.DR_SHAPES:
        base = N.dr_clean(shape)
        plane = base["Hp"] * base["Wp"]
        assert 32 < plane < 96 and plane % 32
        y, x = N.dr_pixel("last_live_pixel", base["pad"])
        assert y * base["Wp"] + x == plane - 1
