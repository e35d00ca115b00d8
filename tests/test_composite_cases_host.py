"""No GPU: the cases of tests/composite_cases.py are what they claim to be.

  * every exact case builds and meets the exactness conditions (composite_cases.check_exact ran inside the builder: the structure, the closed-form
    weights, the float32 oracle against the float64 one), so the device tests may compare with torch.equal;
  * the closed-form gradients of the exact backward agree with the float64 autograd;
  * the hit sweep puts an opaque sample on every position of every lane split, on both sides of every split boundary, and leaves the last 4-ray
    block ragged in every way;
  * the merged-row cases cover empty and one-row halves and put the opaque row in both halves;
  * the continuous cases leave at most one ray in seven out of the disp comparison, and the float32 oracle passes every bar."""
import pytest
import torch

import composite_cases as CC


def test_case_names_are_unique():
    names = CC.EXACT_NAMES + CC.CONT_NAMES + tuple("merged_S%d_na%d_%s" % s for s in CC.merged_specs())
    assert len(set(names)) == len(names)
    assert len(CC.LIVE_EXACT_NAMES) == 3 * len(CC.HIT_S) - 2 + 5 and len(CC.HELPERS_EXACT_NAMES) == 5


@pytest.mark.parametrize("name", CC.EXACT_NAMES)
def test_exact_case_is_exact(name):
    case, want = CC.exact(name)                      # (check_exact ran inside)
    n, S = case["n"], case["S"]
    hits = case["opaque"].long().sum(-1)
    assert int(hits.max()) <= 2
    for white in (False, True):
        w = want[white]
        assert tuple(w["weights"].shape) == (n, S) and tuple(w["rgb"].shape) == (n, 3)
        empty = hits == 0
        assert bool((w["acc"][empty] == 0).all()) and bool((w["depth"][empty] == 0).all()) and bool((w["disp"][empty] != w["disp"][empty]).all())
        assert bool((w["weights"][empty] == 0).all()) and bool((w["rgb"][empty] == (1.0 if white else 0.0)).all())
        assert bool((w["acc"][~empty] == 1).all()) and bool(torch.isfinite(w["disp"][~empty]).all())
    if S <= CC.DRIFT_FREE:
        assert case["confirmable_rays"] == n


def test_hit_sweep_covers_every_lane_split_and_block_remainder():
    lane_samples = lambda S: (lambda e: e if e <= 4 else 8 if e <= 8 else 16)(max(1, (S + 63) // 64))      # noqa: E731  (composite_lane_samples)
    assert {lane_samples(S) for S in CC.HIT_S} == {1, 2, 3, 4, 8, 16}
    for a, b in ((64, 65), (128, 129), (192, 193), (256, 257), (512, 513)):
        assert a in CC.HIT_S and b in CC.HIT_S and lane_samples(a) != lane_samples(b)
    assert {S % 4 for S in CC.HIT_S} == {0, 1, 2, 3}                   # n = S rays: the last block holds 4, 1, 2 and 3 rays
    for S in CC.HIT_S:
        case, _ = CC.exact("hit_S%d_one" % S)
        assert case["n"] == S and torch.equal(case["opaque"], torch.eye(S, dtype=torch.bool))      # every position of every lane, once
        assert bool((case["raw"][..., 3] == 0).sum() == S * S - S)
    case, _ = CC.exact("hit_S65_last")
    assert bool(case["opaque"][:, 64].all()) and int(case["opaque"].sum()) == 2 * 65 - 1
    case, _ = CC.exact("hit_S65_adjacent")
    assert bool(case["opaque"].diagonal(1).all()) and int(case["opaque"].sum()) == 2 * 65 - 1
    sig = CC.exact("hit_S65_one")[0]["raw"][..., 3]
    assert bool(torch.signbit(sig[sig == 0]).any()) and not bool(torch.signbit(sig[sig == 0]).all())      # -0.0 and 0.0 both present
    assert {CC.exact(n)[0]["n"] for n in CC.LIVE_EXACT_NAMES if n.startswith("n")} == {1, 3, 4, 5}
    hits = CC.exact("empty_S65")[0]["opaque"].long().sum(-1).tolist()
    assert hits == [1, 0, 1, 0, 1, 0]                                  # empty rays between opaque ones, in a full block and in the ragged one


def test_helpers_cases_hold_the_listed_situations():
    for name in CC.HELPERS_EXACT_NAMES:
        case, want = CC.exact(name)
        S, sig, noise, z = case["S"], case["raw"][..., 3], case["noise"], case["z"]
        assert {tuple(d) for d in case["rays_d"].tolist()} == {(0.0, 0.0, 1.0), (3.0, 4.0, 0.0)}
        assert set(sig.unique().tolist()) <= {-5.0, 0.0, 1.0, 200.0}
        assert bool(((sig == 200) & ~case["opaque"] & (noise < 0)).any())               # an opaque density switched off by the noise
        assert bool((sig == 1)[:, -1].any()) and bool(case["opaque"][sig[:, -1] == 1, -1].all())      # density 1 is opaque through 1e10
        assert bool(((sig[:, -1] == 0) & (noise[:, -1] == 0) & ~case["opaque"][:, -1]).any())       # 0 * 1e10 = 0
        if S > 2:
            assert bool(((sig == 0) & case["opaque"] & (noise == 200)).any())             # a transparent one switched on
            assert bool(((sig + noise) < 0).any())
            flat = (z[:, 1:] == z[:, :-1]) & (sig[:, :-1] == 200)
            assert bool(flat.any()) and not bool(case["opaque"][:, :-1][flat].any())        # dist 0 under an opaque density: alpha 0
        assert bool((want[False]["disp"] != want[False]["disp"]).any())                     # an empty ray


@pytest.mark.parametrize("name", [n for n in CC.LIVE_EXACT_NAMES])
def test_exact_backward_closed_form_agrees_with_the_float64_autograd(name):
    """Every upstream-gradient combination and both backgrounds up to S = 257; beyond, all four together on a white background (the float64
    autograd over 1024 x 1024 samples is what takes the time; the closed form is the same code at every S)."""
    case, _ = CC.exact(name)
    if case["S"] <= 257:
        CC.check_exact_backward(case)
    else:
        CC.check_exact_backward(case, whites=(True,), combos=(CC.TARGETS,))
    g, mask, _ = CC.expected_g_raw(case, True, CC.TARGETS)
    assert bool(mask.all()) and bool((g[..., 3][case["opaque"]] == 0).all())
    if name.endswith("_one") and case["S"] > 1:      # the one-hit form: gw_i - gw_h in front of the hit (recomputed here from the inputs)
        n, S = case["n"], case["S"]
        ga = case["g_acc"] - case["g_rgb"].sum(-1)
        gw = (case["raw"][..., :3] * case["g_rgb"][:, None]).sum(-1) + case["g_depth"][:, None] * case["z"] + ga[:, None] + case["g_weights"]
        front = torch.tril(torch.ones(S, S, dtype=torch.bool), -1)        # ray r, samples i < r
        assert torch.equal(g[..., 3][front], (gw - gw.diagonal()[:, None])[front])
        assert torch.equal(g[..., 3][front.T], (gw * CC.TINY)[front.T])


def test_merged_cases_cover_the_degenerate_splits_and_both_halves():
    specs = CC.merged_specs()
    for S in CC.MERGED_S:
        nas = {na for s, na, _ in specs if s == S}
        assert {0, 1, S - 1, S} <= nas
        assert {k for s, _, k in specs if s == S} == set(CC.RANK_KINDS)
    for S, na, kind in specs:
        if S > 257 and kind != "random":
            continue
        m, _ = CC.merged_case(S, na, kind)
        assert m["rank"].dtype == torch.int32 and m["raw_a"].shape[1] == na and m["raw_b"].shape[1] == S - na
        assert m["hit_in_a"] + m["hit_in_b"] == S
        if 1 < na < S - 1 or (0 < na < S and kind == "identity"):        # (a one-row half holds the opaque row of a ray only where the rank puts it)
            assert m["hit_in_a"] > 0 and m["hit_in_b"] > 0, m["name"]


@pytest.mark.parametrize("name", CC.CONT_NAMES)
def test_continuous_case_and_the_float32_oracle_under_the_bars(name):
    case, ref, dist, gref, gdist = CC.continuous(name)
    assert case["n"] == 7
    for white in (False, True):
        keep = CC.disp_keep(ref[white])
        assert int((~keep).sum()) <= 1 and not bool(keep[4])            # the deliberately empty ray, and nothing else
        assert bool((ref[white]["disp"][4] != ref[white]["disp"][4]))   # its disp is NaN
        assert not CC.over_the_bar(dist[white], name)
    for d in gdist.values():
        assert not CC.over_the_bar(d, name)
    if case["variant"] == 0:
        assert len(gref) == 2 * len(CC.COMBOS) == 10
        sig = case["raw"][..., 3]
        assert bool((sig[4] == 0).all()) and sig[6, 0] == 200 and (case["S"] < 10 or 0.15 < (sig[5] == 200).float().mean() < 0.45)
        if case["S"] >= 65:                                              # transmittance through the denormals to 0 mid-ray
            T = torch.cumprod(1.0 - (1.0 - torch.exp(-sig[5])) + 1e-10, 0)
            assert bool(((T > 0) & (T < 1.17e-38)).any()) and T[-1] == 0
        rgb = case["raw"][..., :3]
        assert rgb.min() < -0.5 and rgb.max() > 1.5


def test_bars_come_from_the_oracles():
    b = CC.bars()
    assert set(b) == set(CC.BAR_NAMES)
    for k, v in b.items():
        assert 0 < v < 2e-5, (k, v)                                        # float32 rounding of values of order 1 .. 10, nothing else
