"""No GPU: the cases of tests/gather_cases.py are what they claim to be, and ExactDiv divides exactly where it runs.

  * every lattice case (given and derived coordinates) meets the exactness condition and has float32 oracle == float64 oracle -- asserted by the
    builder itself (gather_cases.check_lattice), so the device tests may compare with torch.equal;
  * every continuous case excludes at most 2 % of its (sample, view) pairs;
  * the lattice set holds the spots the gather kernels can get wrong, decided from the float64 coordinates;
  * tests/exact_div_check.cpp, compiled for the host alone, sweeps ExactDiv over every divisor 2..8192."""
import os
import subprocess

import pytest

import gather_cases as G
from conftest import ROOT


@pytest.mark.parametrize("name", G.LATTICE_NAMES + G.DERIVED_NAMES)
def test_lattice_case_is_exact(name):
    case, feats, grads = G.lattice(name)                     # (check_lattice ran inside: equality of the two oracles, the 2^24 bounds)
    assert feats.shape[-1] == 24 + 12 * case["V"] + 1 and feats.numel() == case["m"] * feats.shape[-1]
    mask = feats[..., G.columns(case["V"])["mask"]]
    assert bool(((mask == 0) | (mask == 1)).all())
    assert max(G.weight_bits(case).values()) <= 13             # (few fraction bits: the lattice is coarse on purpose)


def test_lattice_sizes_cover_the_wave_and_block_edges():
    ms = {G.lattice(n)[0]["m"] for n in G.LATTICE_NAMES}
    assert {1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000} <= ms
    assert {G.lattice(n)[0]["V"] for n in G.LATTICE_NAMES} >= {1, 2, 3, 8}
    sizes = {s for n in G.LATTICE_NAMES for dhw in G.lattice(n)[0]["dhw"] for s in dhw}
    assert sizes >= {1, 2, 3, 5, 7, 8}
    for n in G.DERIVED_NAMES:
        c = G.lattice(n)[0]
        assert (c["n"] * c["S"]) % 256 != 0 and len({tuple(r) for r in c["rays_d"].tolist()}) == c["n"]      # rays all different
    assert {G.lattice(n)[0]["S"] for n in G.DERIVED_NAMES} == {1, 2, 3, 5, 30, 90, 192}


def test_lattice_set_contains_what_it_claims():
    total = {}
    for n in G.LATTICE_NAMES:
        for k, v in G.census(G.lattice(n)[0]).items():
            total[k] = total.get(k, 0) + v
    for k in ("edge_x_lo", "edge_x_hi", "edge_y_lo", "edge_y_hi",            # exactly on gx = -1, gx = 1, gy = -1, gy = 1 (the other axis inside)
              "view_texel", "vol_texel",                                     # exactly on a texel of a source view / of the finest volume
              "out_x_lo", "out_x_hi", "out_y_lo", "out_y_hi", "vol_out_lo", "vol_out_hi",      # past every border
              "behind", "clamped", "clamped_negative", "clamped_zero",      # behind a camera; |cz| < 1e-4, also from the negative side and exactly 0
              "absorbed_run", "a_b_a"):                                      # a run crossing positions 7 -> 8 of a wave; a cell met again after another
        assert total.get(k, 0) >= 1, k
    # the run patterns: every length at every start offset within a wave's 16 samples
    order = G.run_order()
    runs, i = set(), 0
    while i < len(order):
        j = i
        while j + 1 < len(order) and order[j + 1] == order[i]:
            j += 1
        runs.add((i % 16, j - i + 1))
        i = j + 1
    assert {(o, n) for o in G.RUN_OFFSETS for n in G.RUN_LENGTHS} <= runs
    # a derived case sits on the edges and texels too (the given-coordinate kernels are not the only ones that meet them)
    d = {}
    for n in G.DERIVED_NAMES:
        for k, v in G.census(G.lattice(n)[0]).items():
            d[k] = d.get(k, 0) + v
    assert d["edge_x_lo"] and d["edge_y_hi"] and d["view_texel"] and d["behind"] and d["absorbed_run"]


@pytest.mark.parametrize("name", G.CONTINUOUS_NAMES)
def test_continuous_case_keeps_98_percent(name):
    case, feats, grads, oracle_d, scale = G.continuous(name)
    assert case["excluded_share"] <= G.EXCLUDED_CAP
    assert 1.0 - G.keep_columns(case).double().mean().item() <= G.EXCLUDED_CAP
    assert case["census"]["behind"] > 0 and case["census"]["front"] > 0 and case["census"]["outside"] > 0
    assert oracle_d["mask_flips"] == 0                       # (away from the excluded spots the two oracles agree on every in-mask bit)
    # the float32 oracle is a float32 computation: its distance from the reference is rounding, not a different result
    for k, v in oracle_d.items():
        if k != "mask_flips":
            assert 0 < v < 1e-5 * max(1.0, scale[k]), (k, v)


@pytest.mark.parametrize("name", G.LATTICE_NAMES + G.DERIVED_NAMES)
def test_network_of_the_fused_comparison_is_well_conditioned_on_the_lattice_features(name):
    """gather_cases.lattice_state_dict: on the exact features the float32 oracle network is within 2e-6 of the float64 one, so the 1e-5 bars of the
    fused-route comparison measure the gather and the split arithmetic, not an ill-conditioned network."""
    import torch
    from oracle import ucnerf_oracle as O
    case, feats, _ = G.lattice(name)
    sd = G.lattice_state_dict(case["V"])
    dirs = torch.tensor([[0.0, 0.0, 1.0]]).repeat(feats.shape[0], 1)
    raw = {}
    for dt in (torch.float64, torch.float32):
        raw[dt] = O.run_network_mvs({k: v.to(dt) for k, v in sd.items()}, case["stage3"].to(dt), dirs.to(dt), feats.to(dt), n_src=case["V"]).double()
    assert (raw[torch.float32] - raw[torch.float64]).abs().max().item() < 2e-6
    assert raw[torch.float64][..., 3].abs().max().item() < 4.0                      # densities of order 1, as on a live scene


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    import shutil
    return shutil.which("hipcc")


def test_exact_div_sweep_on_the_host(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine: tests/exact_div_check.cpp cannot be compiled")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "exact_div_check")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", inc, os.path.join(ROOT, "tests", "exact_div_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ExactDiv ok" in r.stdout, r.stdout + r.stderr
