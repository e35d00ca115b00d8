"""Host-side checks of the gradient chain depth regression -> depth_values -> depth hypotheses -> previous depth.  No GPU: the case builder of
tests/cascade_grad_cases.py produces what it claims (its own assertions -- float32 autograd == float64 autograd on the lattice cases, the mass
bound -- run here, and the census of ties, clamp states and border cells is checked), CPU autograd lets a tie of either clamp pass, the library
exports the new entry points with nothing of ABI v6 moved, and they validate their arguments before any pointer is read."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import cascade_grad_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def lattice():
    return {name: G.lattice_case(name) for name in G.LATTICE}          # (the builder's own assertions run here)


def test_the_lattice_set_holds_every_situation_it_must(lattice):
    census = {name: c["census"] for name, c in lattice.items()}
    print("\nlattice census:", json.dumps(census, indent=1))
    total = {k: sum(c[k] for c in census.values()) for k in next(iter(census.values()))}
    assert total["tie_lo"] > 0 and total["tie_hi"] > 0                   # c - half == near and c + half == far, exactly
    assert total["both"] > 0 and total["one"] > 0 and total["none"] > 0   # both clamps active, one, none
    pads = {c["pad"] for c in lattice.values()}
    assert pads == {0, 1, 2}
    for name, c in lattice.items():
        assert c["want"].abs().max() > 0, name                            # a gradient to get wrong
        assert c["D"] in (2, 3, 5, 9, 33)
        if c["pad"]:
            assert c["census"]["border_nonzero"] > 0 and c["census"]["corner_nonzero"] > 0, name
    assert {c["D"] for c in lattice.values()} == {2, 3, 5, 9, 33}
    # the shapes: a 1 x 1 map, a row, a column, all three scales 1, identity down-sampling
    shapes = {tuple(c["cur"].shape) for c in lattice.values()}
    assert (1, 1) in shapes and (1, 7) in shapes and (7, 1) in shapes
    assert any(tuple(c["cur"].shape) == tuple(c["HW"]) == tuple(c["hw"]) for c in lattice.values())
    assert any(tuple(c["HW"]) == tuple(c["hw"]) != tuple(c["cur"].shape) for c in lattice.values())


def test_cpu_autograd_lets_a_tie_pass(lattice):
    """The 1 x 1 map at c = near + half: the lower clamp ties on every pixel and the upper one is idle, so d out / d c = 1 on every sample when
    the tie passes -- the gradient is the sum of all of g_out -- and d / (D - 1) when it does not."""
    c = lattice["one_pixel_D2_pad1"]
    assert c["census"]["tie_lo"] == c["HW"][0] * c["HW"][1] and c["census"]["both"] == c["census"]["one"] == 0
    assert c["want"].shape == (1, 1)
    passes = c["g_out"].double().sum().item()
    blocked = (c["g_out"].double() * torch.arange(c["D"]).double().view(-1, 1, 1) / (c["D"] - 1)).sum().item()
    assert passes != blocked
    assert c["want"].item() == passes
    # and the upper clamp's tie: the same map at far - half
    want, cc = G.chain_grad(torch.full((1, 1), c["far"] - c["D"] / 2 * c["interval"]), c["g_out"], c["near"], c["far"], c["interval"], c["D"],
                            c["HW"], c["hw"], c["pad"], torch.float64)
    half = c["D"] / 2 * c["interval"]
    assert bool((cc + half == c["far"]).all()) and want.item() == passes


@pytest.mark.parametrize("name", list(G.CONTINUOUS))
def test_continuous_cases_exclude_next_to_nothing(name):
    c = G.continuous_case(name)
    print("\n%s: eps %.3e, excluded share %.2e (%d columns zeroed), float32 witness %.3e, bar %.3e, clamp shares %s"
          % (name, c["eps"], c["excluded_share"], c["zeroed_columns"], c["witness"], c["bar"], c["clamp_shares"]))
    assert c["excluded_share"] <= 0.01
    assert c["want"].abs().max() > 0 and c["witness"] <= c["bar"]
    assert 0 < c["eps"] < 16 * 2.0 ** -23 * c["far"]                      # the float32 chain's c is a few ulp of far off, as cascade_stubs.bar says


def test_regress_cases_are_exact_and_cover_the_sizes():
    cases = {name: G.regress_case(name) for name in G.REGRESS}
    assert {c["prob"].shape[0] for c in cases.values()} == {1, 2, 8, 9, 128}
    assert {c["pad"] for c in cases.values()} == {0, 1, 3}
    assert {c["g_depth"].numel() for c in cases.values()} == {1, 33, 99}
    for name, c in cases.items():
        pad = c["pad"]
        want = c["want"]
        full = torch.nn.functional.pad(c["g_depth"].double(), (pad,) * 4)
        assert torch.equal(want, c["prob"].double() * full), name
        if pad:                                                           # the border gets nothing although its probabilities are not 0
            border = torch.ones_like(full, dtype=torch.bool)
            border[pad:-pad, pad:-pad] = False
            assert want[:, border].abs().max() == 0 and c["prob"][:, border].abs().max() > 0, name


def test_the_entry_points_are_exported_and_nothing_of_the_abi_moved(L):
    raw = C.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    for name in ("ucnerf_depth_hypotheses_bwd", "ucnerf_depth_hypotheses_bwd_scratch_floats", "ucnerf_depth_regress_bwd_values"):
        assert hasattr(raw, name), "library does not export " + name
        assert name in L.SYMBOLS and name + "(" in hdr
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    assert "No backward" not in hdr.split("struct ucnerf_depth_hypotheses_params {")[0][-3000:]
    for sname in ("ucnerf_depth_hypotheses_bwd_params", "ucnerf_depth_regress_bwd_values_params"):
        assert sname not in L.STRUCTS and "struct %s {" % sname in hdr
        cls = L.ADDED_STRUCTS[sname]
        assert L.lib().ucnerf_sizeof(sname.encode()) == C.sizeof(cls) > 0
        body = hdr.split("struct %s {" % sname)[1].split("};")[0]
        declared = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines() if ";" in line]
        declared = [n for d in declared for n in d.split(",")]
        fields = [f[0] for f in cls._fields_]
        if sname.endswith("values_params"):
            declared = ["D", "Hp", "Wp", "pad"] + declared[1:]           # (the four sizes share one declaration)
        assert declared == fields, (declared, fields)
    # the forward's struct is embedded whole and first
    assert L.DepthHypothesesBwdParams._fields_[0] == ("fwd", L.DepthHypothesesParams)


def test_argument_errors_are_einval_in_a_child_process(L):
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before any pointer is read or anything launched."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cascade_grad_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 45 and not out["problems"], out["problems"]


def test_the_mirror_class_takes_both_grad_methods_and_refuses_a_misspelt_one():
    import cascade_stubs as S
    from uc_nerf_amd.network import mvs_models as M
    feature, regs = S.make_stubs(3, 32, 40, [torch.zeros(s) for s in S.stage_logit_shapes(32, 40, [48, 32, 8], 2)])
    for method in ("detach", "undetach"):
        assert M.CascadeMVSNet(grad_method=method, feature=feature, cost_regularization=regs).grad_method == method
    for method in ("Detach", "detatch", None):
        with pytest.raises(NotImplementedError, match="undetach"):
            M.CascadeMVSNet(grad_method=method, feature=feature, cost_regularization=regs)
