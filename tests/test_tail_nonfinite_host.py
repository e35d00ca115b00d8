"""CPU checks of tests/tail_nonfinite_cases.py: the table holds what it claims, each size lands in the instantiation it names, the two CPU
references agree where both apply, and the restatements of the device's search and merge see the defects the cases were written for."""
import pytest
import torch

import tail_nonfinite_cases as TN

PDF_NAMES, COMP_CANDIDATES = TN.pdf_names(), TN.comp_candidates()


# ------------------------------------------------------------------------------------------------ the table
def test_every_poison_kind_sits_at_every_position_class():
    assert len(PDF_NAMES) == 4 * (len(TN.PDF_L) + len(TN.PDF_S)) * len(TN.PDF_M)
    want = {"weights": ({"w_nan", "w_inf", "w_nan_zeros"}, 13, 3), "depths": ({"z_nan"}, 5, 5), "draws": ({"u_nan"}, 10, 4), "shared": ({"w_nan"}, 4, 4)}
    for name in PDF_NAMES:
        case = TN.pdf_case(name)
        everywhere, n_poisoned, n_clean = want[case["group"]]
        assert case["n"] <= 16 and int(case["poisoned"].sum()) == n_poisoned == len(case["rays"]) and case["n"] - n_poisoned == n_clean
        pairs = {(r["kind"], r["cls"]) for r in case["rays"]}
        assert {(k, c) for k in everywhere for c in TN.POSITIONS} <= pairs
        if case["group"] == "weights":
            assert ("w_all_nan", None) in pairs
        if case["group"] == "depths":
            assert ("z_inf_last", "last") in pairs
        if case["group"] == "draws":
            assert {(k, c) for k in ("u_one", "u_above", "u_below") for c in ("first", "last")} <= pairs
        assert case["shared"] == (case["u"].dim() == 1)
    for name in COMP_CANDIDATES:
        case = TN.comp_case(name)
        kinds = {"sigma": {"sigma_nan", "sigma_inf"}, "colour_nan": {"colour_nan"}, "colour_inf": {"colour_inf_zero_weight"},
                 "geometry": {"zero_interval_inf_sigma"}}[case["group"]]
        pairs = {(r["kind"], r["cls"]) for r in case["rays"]}
        assert {(k, c) for k in kinds for c in TN.POSITIONS} <= pairs and (case["group"] != "geometry" or ("rays_d_nan", None) in pairs)
        assert case["n"] <= 16 and case["n"] - int(case["poisoned"].sum()) == 4
    assert {TN.comp_case(n)["variant"] for n in COMP_CANDIDATES} == {0, 1}


def test_the_poison_is_in_the_poisoned_rays_and_nowhere_else():
    for name in PDF_NAMES:
        case = TN.pdf_case(name)
        for r in range(case["n"]):
            same = all(TN.same_bits(case[k][r], case["clean"][k][r]) for k in ("w", "z") + (() if case["shared"] else ("u",)))
            assert same != bool(case["poisoned"][r]), (name, r)
    for name in COMP_CANDIDATES:
        case = TN.comp_case(name)
        for r in range(case["n"]):
            same = all(TN.same_bits(case[k][r], case["clean"][k][r]) for k in case["clean"])
            assert same != bool(case["poisoned"][r]), (name, r)
        for ray in case["rays"]:
            if ray["kind"] == "colour_inf_zero_weight" and case["variant"] == 0:
                assert float(TN.comp_reference(name, False)[1]["weights"][ray["ray"], ray["index"]]) == 0.0


def test_positions_fall_where_their_class_says():
    for S, E in zip(TN.COMP_S, (1, 2, 8, 16)):
        assert TN.composite_lane_samples(S) == E and (S % E != 0 or S in (3, 1024))  # 65 and 257 end in a ragged lane, 1024 fills all 64
        b, i = TN.position(S, "boundary", E), TN.position(S, "inside", E)
        assert b % E == 0 and 0 < b < S - 1 or S == 3
        assert (i % E == 1 or E == 1) and 0 < i <= S - 1
    assert TN.position(65, "boundary") == 64 and TN.position(130, "boundary") == 64 and TN.position(7, "boundary") == 3


def test_each_size_lands_in_the_instantiation_it_names():
    assert [TN.sum_path(L - 1) for L in TN.PDF_L] == ["scalar", "lanes8", "lanes8", "lanes8"]
    assert [(L - 1 + 63) // 64 for L in TN.PDF_L] == [1, 1, 2, 3]                  # scan chunks of the cdf
    for L in TN.PDF_L:
        for M in TN.PDF_M:
            assert TN.pdf_instantiation(L, TN.N_MERGE_BINS, M) == ((128, 512) if L <= 128 else (1024, 2048))
    for S, want in zip(TN.PDF_S, ((128, 512), (128, 512), (1024, 2048))):
        assert TN.pdf_instantiation(S - 1, S, 7) == want
    assert TN.pdf_instantiation(128, 384, 128) == (128, 512) and TN.pdf_instantiation(128, 385, 128) == (1024, 2048)
    assert TN.pdf_instantiation(129, 0, 1) == (1024, 2048)
    assert [TN.composite_lane_samples(S) for S in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 3, 4, 8, 8, 16, 16]


# ------------------------------------------------------------------------------------------------ re-sampling references
@pytest.mark.parametrize("name", PDF_NAMES)
def test_the_two_references_agree_on_every_clean_ray(name):
    case, ref = TN.pdf_case(name), TN.pdf_reference(name)
    samples, inds, cdf = TN.oracle_pdf(name)
    keep = ~case["poisoned"]
    assert int(keep.sum()) >= 3
    assert TN.same_bits(cdf[keep], ref["cdf"][keep]) and torch.equal(inds[keep], ref["inds"][keep]) and TN.same_bits(samples[keep], ref["samples"][keep])
    assert bool(torch.isfinite(ref["samples"][keep]).all())
    # ... and a clean ray's reference does not depend on the other rays of its batch
    clean = TN.pdf_reference(name, "clean")
    for k in ("samples", "inds", "cdf", "z_sorted"):
        assert TN.same_bits(ref[k][keep], clean[k][keep]), k


@pytest.mark.parametrize("name", PDF_NAMES)
def test_fixed_search_is_torch_searchsorted_and_the_old_form_is_not_under_nan(name):
    case, ref = TN.pdf_case(name), TN.pdf_reference(name)
    u = TN.pdf_inputs(case)[2]
    assert torch.equal(TN.search_restated(ref["cdf"], u, fixed=True), ref["inds"])
    old = TN.search_restated(ref["cdf"], u, fixed=False)
    nan_rows = torch.isnan(ref["cdf"]).any(-1) | torch.isnan(u).any(-1)
    assert torch.equal(old[~nan_rows], ref["inds"][~nan_rows])
    if bool(nan_rows.any()):
        assert not torch.equal(old, ref["inds"]), "the <= form agrees with torch on a case with NaN in cdf or u"
        assert case["group"] in ("weights", "draws", "shared")
    assert int(ref["inds"].min()) >= 0 and int(ref["inds"].max()) <= case["L"]


@pytest.mark.parametrize("name", PDF_NAMES)
def test_fixed_merge_is_a_permutation_that_sorts_and_the_old_rule_is_not_under_nan(name):
    case, ref = TN.pdf_case(name), TN.pdf_reference(name)
    for cat, M, want in ((ref["cat"], case["M"], ref["z_sorted"]), (ref["samples"], case["M"], torch.sort(ref["samples"], -1)[0])):
        rank = TN.merge_rank_restated(cat, M, fixed=True)
        assert TN.is_permutation(rank), name
        assert TN.same_bits(TN.placed(cat, rank), want), TN.first_difference(TN.placed(cat, rank), want)
        old = TN.merge_rank_restated(cat, M, fixed=False)
        nan_rows = torch.isnan(cat).any(-1)
        assert torch.equal(old[~nan_rows], rank[~nan_rows])
        for r in nan_rows.nonzero().flatten().tolist():
            assert not TN.is_permutation(old[r:r + 1]), (name, r)
    # (a NaN or +inf bin edge reaches the concatenation only through a draw that lands next to it: not required of the `bins` form)
    if case["group"] != "depths" or case["from_coarse"]:
        assert bool(torch.isnan(ref["cat"]).any()), "a case without a NaN in the concatenation"


def test_nan_row_of_the_issue_ranks_as_stated():
    row = torch.tensor([[TN.NAN, 1.0, TN.NAN, 0.5, TN.INF, -TN.INF, 2.0]])
    assert TN.merge_rank_restated(row, 3, fixed=False)[0].tolist() == [0, 2, 0, 1, 4, 0, 3]
    assert TN.merge_rank_restated(row, 3, fixed=True)[0].tolist() == [5, 2, 6, 1, 4, 0, 3]
    # a one-element list with a NaN escapes the sortedness test of the old rule through the pair across the two lists
    for row, M in ((torch.tensor([[TN.NAN, 1.0, 2.0, 3.0]]), 1), (torch.tensor([[1.0, 2.0, 3.0, TN.NAN]]), 3)):
        assert not TN.is_permutation(TN.merge_rank_restated(row, M, fixed=False))
        assert TN.is_permutation(TN.merge_rank_restated(row, M, fixed=True))
    cdf = torch.tensor([[0.0, 0.2, TN.NAN, 0.7, 1.0]])
    assert int(torch.searchsorted(cdf, torch.tensor([[0.1]]), right=True)) == 3 == int(TN.search_restated(cdf, torch.tensor([[0.1]]))[0, 0])
    assert int(TN.search_restated(cdf, torch.tensor([[0.1]]), fixed=False)[0, 0]) == 1


# ------------------------------------------------------------------------------------------------ compositing references
@pytest.mark.parametrize("name", COMP_CANDIDATES)
def test_float32_and_float64_oracles_put_their_non_finite_values_on_the_same_elements(name):
    bad = TN.oracle_disagreements(name)
    if name in TN.DROPPED:
        assert bad, "%s is listed as dropped, but the two oracles agree on it" % name
    else:
        assert not bad, "%s: the oracles disagree on %s" % (name, ", ".join(bad))
    case = TN.comp_case(name)
    clean = TN.clean_of(case)
    for white in (False, True):
        f64 = TN.comp_reference(name, white)[0]
        ref_clean = TN.CC.forward(clean, TN.F64, white)
        keep = ~case["poisoned"]
        for k in f64:                                                        # a clean ray's reference does not depend on the other rays
            assert TN.same_bits(f64[k][keep], ref_clean[k][keep]) and bool(torch.isfinite(f64[k][keep]).all()), (name, k)
        poisoned_seen = torch.zeros(case["n"], dtype=torch.bool)
        for k in f64:
            poisoned_seen |= ~torch.isfinite(f64[k].reshape(case["n"], -1)).all(-1)
        assert not bool((poisoned_seen & keep).any())
    if case["group"] != "colour_inf" or case["variant"] == 0:
        assert bool(poisoned_seen[case["poisoned"]].any()), name + ": no poison reaches an output"


def test_the_float32_oracle_on_these_rows_is_inside_the_bars():
    """The bars come from composite_cases' continuous cases; the finite elements of the float32 oracle on the rows here sit under them too."""
    for name in TN.comp_names():
        for white in (False, True):
            f64, f32, g64, g32 = TN.comp_reference(name, white)
            fails = TN.comp_fwd_failures(f32, name, white, "float32 oracle")
            if g32 is not None:
                fails += TN.comp_bwd_failures(g32, name, white, "float32 oracle")
            assert not fails, "\n".join(fails)
