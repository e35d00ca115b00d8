"""No GPU: the cases of tests/mvs_cases.py are what they claim to be.

  * every cost-volume lattice case has float32 coordinates == float64 coordinates; class P has float32 oracle == float64 oracle on variance, count
    and g_feats and meets the 2^24 bound on every partial sum of the atomics (mvs_cases.check_cv_lattice, run by the builder);
  * every depth-regression lattice case has float32 oracle == float64 oracle on every output and every backward mode (check_dr_lattice);
  * the census, taken from float64 coordinates, holds every spot the kernels can get wrong;
  * every continuous case excludes at most 2 % of its voxels and pixels, and the float32 oracle passes every bar it defines;
  * the builders are deterministic."""
import pytest
import torch

import mvs_cases as G


@pytest.mark.parametrize("name", G.CV_LATTICE_NAMES)
def test_cost_volume_lattice_case_is_exact(name):
    case, cls, ref, f32 = G.cv_lattice(name)                     # (check_cv_lattice ran inside)
    C, D, Hp, Wp = case["C"], case["D"], case["H"] + 2 * case["pad"], case["W"] + 2 * case["pad"]
    assert ref[0].shape == (C, D, Hp, Wp) and ref[1].shape == (D, Hp, Wp) and ref[2].shape == case["feats"].shape
    msum = torch.round(1 / ref[1])
    assert bool((msum >= 1).all()) and bool((msum <= 1 + case["V"]).all())
    if cls == "P":
        assert set(msum.unique().tolist()) <= {1.0, 2.0, 4.0, 8.0}
    else:
        assert set(msum.unique().tolist()) & {3.0, 5.0, 6.0, 7.0, 9.0}          # a count that rounds


def test_cost_volume_lattice_set_contains_what_it_claims():
    cases = [G.cv_lattice(n) for n in G.CV_LATTICE_NAMES]
    total, runs, p_total, p_runs = {}, set(), {}, set()
    for case, cls, _, _ in cases:
        c = G.cv_census(case)
        r = c.pop("runs")
        runs |= r
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        if cls == "P":
            p_runs |= r
            for k, v in c.items():
                p_total[k] = p_total.get(k, 0) + v
    items = ("half_x_even", "half_x_odd", "half_y_even", "half_y_odd",         # exactly on x.5 / y.5 above an even and an odd neighbour
             "edge_x_lo", "edge_x_hi", "edge_y_lo", "edge_y_hi",               # exactly on gx = -1, gx = 1, gy = -1, gy = 1 (the other axis inside)
             "out_x_lo", "out_x_hi", "out_y_lo", "out_y_hi",                   # past all four borders: the clamp
             "behind", "in_view",
             "run_crossing_a_wave", "a_b_a", "wave_of_8_different_columns", "one_pixel_for_every_voxel")
    for k in items:
        assert total.get(k, 0) >= 1, k
        assert p_total.get(k, 0) >= 1, "class P: " + k                         # (the bit-for-bit backward meets every one of them as well)
    want_runs = {(s, n) for s in G.RUN_STARTS for n in G.RUN_LENGTHS}
    assert want_runs <= runs and want_runs <= p_runs
    assert {(0, 40), (0, 17)} <= p_runs                                         # a run of length D: over two grid rows, and ending in a wave's first position
    assert {len(c["views"]) for c, _, _, _ in cases} >= {1, 2, 3, 7, 8}
    assert {c["C"] for c, _, _, _ in cases} >= {1, 3, 16, 17, 24, 33}
    assert {c["pad"] for c, _, _, _ in cases} >= {0, 1, 3}
    assert {c["D"] for c, _, _, _ in cases} >= {1, 2, 5, 7, 8, 9, 16, 17, 31, 32, 33, 40}
    assert {c[k] - 1 for c, _, _, _ in cases for k in ("H", "W")} >= {1, 2, 4, 8, 16, 32}
    assert {float(c) for case, _, _, _ in cases for c in case["proj"][:, 2, 2].tolist()} == {1.0, 2.0, 0.5, -1.0}
    planes = [((c["H"] + 2 * c["pad"]) * (c["W"] + 2 * c["pad"]), c["D"]) for c, _, _, _ in cases]
    assert any(p % 8 and (p * d) % 32 and (p * d) % 256 for p, d in planes)    # tails in the narrow, the wide and the backward grid
    assert any(p < 8 for p, d in planes)
    # both forward layouts and the backward's second grid row in both classes
    for cls in "PQ":
        mine = [c for c, k, _, _ in cases if k == cls]
        assert any(c["C"] > 16 for c in mine) and any(c["C"] <= 16 for c in mine) and any(c["D"] > 32 for c in mine)


@pytest.mark.parametrize("name", G.DR_LATTICE_NAMES)
def test_depth_regression_lattice_case_is_exact(name):
    case, ref = G.dr_lattice(name)                               # (check_dr_lattice ran inside)
    prob, depth, conf, g_pre, g_init = ref["both"]
    assert set(prob.unique().tolist()) <= {0.0, 0.125, 0.25, 0.5, 1.0}
    assert (g_init is not None) == (case["prob_init"] is not None)
    assert bool((conf * 8 == torch.floor(conf * 8)).all()) and bool((conf <= 1).all())
    for mode in G.DR_MODES:
        assert ref[mode][3].shape == prob.shape
    pad, Hp, Wp = case["pad"], case["Hp"], case["Wp"]
    if pad:                                                      # the border pixels: probabilities as everywhere, gradient exactly 0
        inner = torch.zeros(Hp, Wp, dtype=torch.bool)
        inner[pad:Hp - pad, pad:Wp - pad] = True
        assert bool((prob[:, ~inner].sum(0) == 1).all()) and bool((g_pre[:, ~inner] == 0).all())
    assert bool((g_pre != 0).any()) or case["D"] == 1


def test_depth_regression_lattice_set_contains_what_it_claims():
    cases = [G.dr_lattice(n)[0] for n in G.DR_LATTICE_NAMES]
    total = {}
    for case in cases:
        for k, v in G.dr_census(case).items():
            total[k] = total.get(k, 0) + v
    for k in ("e_integer_two_hot", "e_half", "window_0", "window_d_minus_2", "window_d_minus_1", "window_sum_1", "window_sum_below_1",
              "hot_in_one_lane", "hot_in_different_lanes", "border_pixels"):
        assert total.get(k, 0) >= 1, k
    assert {c["D"] for c in cases} == {1, 2, 3, 7, 8, 9, 16, 17, 127, 128}
    assert {c["pad"] for c in cases} >= {0, 1, 3}
    assert {c["Hp"] * c["Wp"] for c in cases} >= {1, 31, 32, 33}
    assert any(c["pad"] > 0 and (c["Hp"] * c["Wp"]) % 32 for c in cases)
    assert {len(s) for c in cases for s in c["hot"]} == {1, 2, 4, 8}
    assert {c["prob_init"] is not None for c in cases} == {True, False}
    # the window edges are met at the largest D too (the LDS copy's last rows)
    big = G.dr_census(G.dr_lattice("d128_pad1_plane99")[0])
    assert big["window_d_minus_1"] and big["window_d_minus_2"] and big["window_0"]


@pytest.mark.parametrize("name", G.CONTINUOUS_NAMES)
def test_continuous_case_keeps_98_percent_and_the_float32_oracle_passes_its_bars(name):
    case, ref, oracle_d, scale = G.continuous(name)
    print("\n%s: float32 oracle's coordinate error %s pixels, E[d] error %.3g; excluded %.3f %% of the voxels, %.3f %% of the pixels"
          % (name, {k: "%.3g" % v for k, v in case["coord_error"].items()}, case["e_error"], 100 * case["excluded_voxels"], 100 * case["excluded_pixels"]))
    print("%s: float32 oracle's distances %s" % (name, {k: "%.3g" % v for k, v in oracle_d.items()}))
    assert case["excluded_voxels"] <= G.EXCLUDED_CAP and case["excluded_pixels"] <= G.EXCLUDED_CAP
    assert case["H"] <= 24 and case["W"] <= 40 and case["D"] <= 12
    assert 0 < max(case["coord_error"].values()) < 1e-4 and 0 < case["e_error"] < 1e-5
    assert case["census"]["in_view"] > 0 and case["census"]["outside"] > 0 and case["census"]["clamped"] > 0
    assert bool((case["g_variance"][:, case["skip_voxel"]] == 0).all()) and bool((case["g_confidence"][case["skip_pixel"]] == 0).all())
    # off the excluded voxels the two oracles pick the same pixels and count the same views: the float32 oracle's distance is rounding
    f32_count = G.cv_reference(case, G.F32)[1]
    keep = ~case["skip_voxel"]
    assert torch.equal(torch.round(1 / f32_count.double())[keep], torch.round(1 / ref["count"])[keep])
    for k, v in oracle_d.items():
        assert v <= G.bar(v, scale[k])
        assert v < 2e-6 * max(1.0, scale[k]), (k, v, scale[k])


def test_case_builders_are_deterministic():
    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    for n in ("q_v3_c17_d9", "p_runs_v3_c3_d40"):
        same(G.cv_lattice_case(n, seed=G.CV_LATTICE_NAMES.index(n), **G.CV_LATTICE_SPECS[n]), G.cv_lattice(n)[0])
    n = "d17_pad1_plane45"
    same(G.dr_lattice_case(n, seed=G.DR_LATTICE_NAMES.index(n), **G.DR_LATTICE_SPECS[n]), G.dr_lattice(n)[0])
    n = "cont_far_v8_c8_pad3"
    same(G.continuous_case(n, seed=2000 + G.CONTINUOUS_NAMES.index(n), **G.CONTINUOUS_SPECS[n]), G.continuous(n)[0])
