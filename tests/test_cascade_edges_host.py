"""Host-side checks of the forward edge cases of the cascade link (tests/cascade_edge_cases.py): no GPU.  The cases are what they claim -- the
lattice cases are exact in float32 at every intermediate, their clamps are partial, they cover the shapes the GPU tests rely on; the float64 chain
and the float32 torch op chain (cascade_stubs.hypotheses_chain, pinned to fixture G19 by tests/test_cascade_host.py) agree within
cascade_stubs.bar(far); the one-hot footprints partition unity; the non-finite cases have a non-trivial NaN set -- and the refusals of
ops.depth_hypotheses and of the entry point that tests/test_cascade_host.py does not reach yet."""
import ctypes as C

import pytest
import torch

import cascade_edge_cases as E
import cascade_stubs as S


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", list(E.LATTICE))
def test_lattice_cases_are_exact_in_float32(name):
    c = E.lattice_case(name)
    assert E.inexact_parts(c) == []
    ref = E.reference(c)
    assert torch.isfinite(ref["out"]).all()
    # the float32 torch op chain gives the very same bits: two restatements, one answer
    assert torch.equal(E.stub_chain(c).double(), ref["out"])
    lo_share, hi_share = E.clamp_shares(ref, c["near"], c["far"])
    if name in E.LATTICE_CLAMPS_PARTIAL:
        assert 0.0 < lo_share < 1.0 and 0.0 < hi_share < 1.0, (lo_share, hi_share)


def test_a_case_off_the_lattice_is_rejected():
    c = E.lattice_case("up4_down2_D5")
    assert "device half" in E.inexact_parts(dict(c, k=1 / 48, interval=None))          # k = 1 / 48 is no dyadic number
    off = dict(c, cur=c["cur"] + 2.0 ** -20)                                           # x4 up, x2 down, D - 1 = 4: 2^-20 needs 30 fraction bits
    assert E.inexact_parts(off)
    assert E.inexact_parts(dict(c, D=4))                                               # D - 1 = 3: the step is no dyadic number


def test_lattice_cases_cover_what_the_gpu_tests_rely_on():
    cases = E.LATTICE.values()
    pads = {c[4] for c in cases}
    assert {0, 1, 3} <= pads and any(c[4] > c[2][0] for c in cases)                    # pad larger than h
    assert any(c[2] == c[1] and c[0] != c[1] for c in cases)                           # up-sampling only
    assert any(c[0] == c[1] and c[2] != c[1] for c in cases)                           # down-sampling only
    assert any(c[0] == c[1] == c[2] for c in cases)                                    # neither
    assert any(c[0] != c[1] and c[2] != c[1] for c in cases)                           # both
    for axis in (0, 1):
        assert any(c[0][axis] == 1 for c in cases) and any(c[2][axis] == 1 for c in cases)      # a 1-pixel axis in h0, w0, h, w
    planes = [(c[2][0] + 2 * c[4]) * (c[2][1] + 2 * c[4]) for c in cases]
    assert any(p > 256 and p % 256 for p in planes)                                    # more than one block, the last one ragged
    assert {2, 3, 5, 9, 17} <= {c[3] for c in cases}                                   # D - 1 a power of two; 9 and 17: ragged depth chunks
    for name in E.CHUNK_LATTICE + E.GUARD_CASES:
        assert E.LATTICE[name][3] in (9, 17)
    assert all(E.LATTICE[name][4] == 1 for name in E.GUARD_CASES) and {E.LATTICE[name][3] for name in E.GUARD_CASES} == {9, 17}
    for name in E.CHUNK_LATTICE:                                                       # the line through planes 0 and D - 1 IS the volume, exactly
        out = E.reference(E.lattice_case(name))["out"]
        assert torch.equal(E.line_through_the_ends(out.float()), out)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", list(E.FOOTPRINT))
def test_footprints_partition_unity_and_both_tap_rules_agree_on_them(name):
    hw0, HW, hw, D, pad = E.FOOTPRINT[name]
    total = 0
    for i in range(hw0[0]):
        for j in range(hw0[1]):
            c = E.footprint_case(name, (i, j))
            ref = E.reference(c)
            assert float(ref["half"]) == 0 and torch.equal(ref["lo"], ref["c"]) and torch.equal(ref["hi"], ref["c"])       # no clamp binds
            out = ref["out"]
            assert 0 < int((out[0] != 0).sum()) < out[0].numel()
            assert all(torch.equal(out[d], out[0]) for d in range(D))
            # no source index lies on an integer: the float32 rule has the same footprint as the float64 one
            assert torch.equal(E.stub_chain(c) != 0, out != 0)
            total = total + out
    assert (total - 1).abs().max().item() <= 1e-12
    assert (E.reference(E.footprint_case(name))["out"] - 1).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------------ C, D, F
def _share(c, **over):
    ref = E.reference(c, **over)["out"]
    return (E.stub_chain(c, **over).double() - ref).abs().max().item() / S.bar(c["far"])


@pytest.mark.parametrize("name", E.CONTINUOUS)
def test_the_two_restatements_agree_on_the_continuous_cases(name):
    c = E.continuous_case(name)
    share = _share(c)
    print("%s: float32 op chain against the float64 chain: %.3f of the bar" % (name, share))
    assert share <= 1.0
    ref = E.reference(c)
    lo_share, hi_share = E.clamp_shares(ref, c["near"], c["far"])
    if name == "both_clamps_everywhere":
        assert lo_share == hi_share == 1.0 and float(ref["half"]) > c["far"] - c["near"]
    if name == "step_edge":
        rows = c["cur"].shape[0]
        jump = c["cur"][rows // 2:].min() - c["cur"][:rows // 2].max()
        assert jump > 0.8 * (c["far"] - c["near"]) / 2 and 0.0 < lo_share < 1.0 and 0.0 < hi_share < 1.0


@pytest.mark.parametrize("D", E.CHUNK_DEPTHS)
def test_the_two_restatements_agree_on_the_chunk_cases(D):
    c = E.chunk_case(D)
    assert _share(c) <= 1.0
    for factor in (0.5, 2.0):                                              # part D's other intervals: they move the output by more than the bar
        iv = factor * (c["far"] - c["near"])
        assert _share(c, interval=iv) <= 1.0
        moved = (E.reference(c, interval=iv)["out"] - E.reference(c)["out"]).abs().max().item()
        assert moved > 100 * S.bar(c["far"])


def test_row_chain_agrees_with_the_stub():
    row = torch.linspace(2.0, 11.0, 48)
    for D in (2, 9, 48):
        assert (E.row_chain(row, D, (3, 5), 1) - S.row_chain(row, D, (3, 5), 1).double()).abs().max().item() <= S.bar(11.0)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("name", list(E.NONFINITE))
def test_nonfinite_cases_have_a_non_trivial_nan_set(name):
    cases = [E.nonfinite_case(name, kind, spot) for kind in E.NONFINITE_KINDS for spot in E.NONFINITE_SPOTS] + [E.nonfinite_all_three(name)]
    for c in cases:
        want = E.classes(E.stub_chain(c))
        n_nan = int((want == 1).sum())
        assert 0 < n_nan < want.numel(), (c["name"], n_nan)
        # the float64 chain has the same classes, and agrees with the op chain wherever both are finite
        ref = E.reference(c)["out"]
        assert torch.equal(E.classes(ref), want), c["name"]
        finite = want == 0
        assert (E.stub_chain(c).double() - ref)[finite].abs().max().item() <= S.bar(c["far"])
        # torch's clamp backward lets nothing through a NaN: the gradient of a finite g_out is finite everywhere
        g = E.chain_grad64(c, torch.ones_like(ref))
        assert torch.isfinite(g).all(), c["name"]


# ------------------------------------------------------------------------------------------------ refusals
def test_the_wrapper_refuses_both_inputs_before_it_looks_at_a_device():
    from uc_nerf_amd import ops
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.depth_hypotheses(8, (4, 5), cur_depth=torch.rand(4, 5), row=torch.rand(48), near_far=torch.tensor([1.0, 2.0]), k=1 / 48)
    with pytest.raises(RuntimeError, match="exactly one"):
        ops.depth_hypotheses(8, (4, 5), near_far=torch.tensor([1.0, 2.0]), k=1 / 48)


def test_the_launch_path_turns_the_entry_points_refusals_into_errors():
    """The wrapper's own checks past `exactly one` need device tensors (tests/test_hip_cascade_edges.py); what it leaves to the entry point is
    refused there before any pointer is read or anything is launched, and _lib.call -- the path the wrapper launches through -- raises with the
    entry point's message.  (The return codes themselves: tests/cascade_probe.py.)"""
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib as L

    def params(mode="map", **kw):
        p = L.DepthHypothesesParams()
        p.D, p.h, p.w, p.pad, p.H, p.W, p.h0, p.w0, p.D_in, p.k = 8, 16, 20, 1, 32, 40, 8, 10, 0, 1.0 / 48
        p.near_far = p.out = 64                                           # stands for a device address: never dereferenced
        if mode == "map":
            p.cur_depth = 64
        else:
            p.row, p.D_in = 64, 48
        for key, v in kw.items():
            setattr(p, key, v)
        return p

    for what, p, needle in (("h0 > H", params(h0=33), "must cover"), ("w > W", params(w=41), "must cover"), ("negative pad", params(pad=-1), "negative size"),
                            ("negative pad, row mode", params("row", pad=-1), "negative size"), ("D = 1 in row mode", params("row", D=1), "D = 1"),
                            ("both inputs", params(row=64, D_in=48), "exactly one"), ("neither input", params(cur_depth=None), "exactly one")):
        with pytest.raises(RuntimeError, match=needle):
            L.call("ucnerf_depth_hypotheses", p, 0)
        assert C.sizeof(p) == L.lib().ucnerf_sizeof(b"ucnerf_depth_hypotheses_params"), what
