"""No GPU: the cases of tests/rays_cases.py are what they claim to be, and the float32 restatement is what the kernels of csrc/rays.hip run.

  * fma32 (the exactly rounded fmaf the restatement needs) equals std::fmaf on 1.2 M triples, constructed half-way cases included; the naive
    float64 emulation does NOT, so the sweep has teeth;
  * linspace01 and sincos_pe_fast of the restatement equal, bit for bit, the device headers compiled for the host (tests/rays_host_check.cpp);
    a shifted linspace midpoint does not;
  * every lattice case has restatement == float64 reference element for element (asserted by the builder); every continuous case keeps every
    element and stays within a few float32 roundings of float64;
  * the restatement reproduces the golden fixtures G1-G5 under the bars of tests/test_hip_parity.py;
  * every case hits the edge it is named for (census);
  * the sincos restatement is within 2e-7 of float64 (the claim of sincos_cw.h), odd / even symmetric bit for bit, and (0, 1) at 0;
  * linspace01 is within 1 ulp of torch.linspace for S = 1..300, 512, 768 -- equality is NOT asserted, it depends on the host's vector width;
  * every argument error of the eight entry points is UCNERF_EINVAL with a message (tests/rays_probe.py, in a child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rays_cases as RC
from conftest import ROOT, load_golden

F32, F64 = np.float32, np.float64
LIN_SIZES = tuple(range(1, 301)) + (512, 768)


# ------------------------------------------------------------------------------------------------ the device headers on the host
def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    import shutil
    return shutil.which("hipcc")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """(fma [n,4], lin [n], sc [n,3]) written by tests/rays_host_check.cpp, compiled the way tests/test_gather_cases_host.py compiles its sweep."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine: tests/rays_host_check.cpp cannot be compiled")
    tmp = tmp_path_factory.mktemp("rays_host_check")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe, data = str(tmp / "rays_host_check"), str(tmp / "data.bin")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", inc,
           os.path.join(ROOT, "tests", "rays_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0 and "rays host check ok" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(data, dtype=np.uint8)
    n_fma, n_lin, n_sc = raw[:12].view(np.int32)
    body = raw[12:].view(F32)
    assert body.size == 4 * n_fma + n_lin + 3 * n_sc
    return body[:4 * n_fma].reshape(-1, 4), body[4 * n_fma:4 * n_fma + n_lin], body[4 * n_fma + n_lin:].reshape(-1, 3)


def test_fma32_equals_std_fmaf_and_the_naive_emulation_does_not(host_check):
    fma, _, _ = host_check
    assert fma.shape[0] >= 1000000
    a, b, c, want = fma.T
    got = RC.fma32(a, b, c)
    bad = ~((RC.bits(got) == RC.bits(want)) | ((got != got) & (want != want)))
    assert not bad.any(), (int(bad.sum()), fma[bad][:4], got[bad][:4])
    # the constructed half-way cases: float64(a b + c) sits ON a float32 tie with a residual left over
    p = a.astype(F64) * b.astype(F64)
    s = p + c.astype(F64)
    residual = (s - p) != c.astype(F64)
    with np.errstate(all="ignore"):
        up, down = np.nextafter(s.astype(F32), F32(np.inf)).astype(F64), np.nextafter(s.astype(F32), F32(-np.inf)).astype(F64)
        on_tie = np.isfinite(s) & ((s - s.astype(F32).astype(F64) == (up - s.astype(F32).astype(F64)) / 2) |
                                   (s - s.astype(F32).astype(F64) == (down - s.astype(F32).astype(F64)) / 2))
    assert int((on_tie & residual).sum()) >= 10000
    naive = RC.fma32_double_rounded(a, b, c)
    wrong = RC.bits(naive) != RC.bits(want)
    assert int(wrong.sum()) >= 1000 and bool((on_tie & residual)[wrong].all())      # a deliberately wrong fmaf turns this test red, and only there


def _linspace01_shifted(i, S):
    """linspace01 with the switch one element late (`i <= S / 2`): deliberately wrong."""
    i = np.asarray(i, dtype=np.int64)
    if S == 1:
        return np.zeros(i.shape, F32)
    step = F32(1) / F32(S - 1)
    return np.where(i <= S // 2, step * i.astype(F32), F32(1) - step * (S - 1 - i).astype(F32)).astype(F32)


def test_linspace01_equals_the_device_header_and_a_shifted_midpoint_does_not(host_check):
    _, lin, _ = host_check
    got = np.concatenate([RC.linspace01(np.arange(S), S) for S in LIN_SIZES])
    assert got.shape == lin.shape and np.array_equal(RC.bits(got), RC.bits(lin))
    shifted = np.concatenate([_linspace01_shifted(np.arange(S), S) for S in LIN_SIZES])
    assert int((RC.bits(shifted) != RC.bits(lin)).sum()) > 0                                          # (one element each of 75 of the 302 lengths)
    near, far = F32([[0.75]]), F32([[5.5]])                                                           # and it reaches the depths the device is held to
    assert not RC.same_bits(RC.stratified32(near, far, 64, 0, 0.0, None, linspace=_linspace01_shifted), RC.stratified32(near, far, 64, 0, 0.0, None))


def test_sincos_restatement_equals_the_device_header_bit_for_bit(host_check):
    _, _, sc = host_check
    assert sc.shape[0] >= 1000000
    s, c = RC.sincos_fast32(sc[:, 0])
    assert np.array_equal(RC.bits(s), RC.bits(sc[:, 1])) and np.array_equal(RC.bits(c), RC.bits(sc[:, 2]))


# ------------------------------------------------------------------------------------------------ sincos against float64
def _sincos_error(r):
    s, c = RC.sincos_fast32(r)
    r64 = np.asarray(r, F64)
    return max(float(np.abs(s.astype(F64) - np.sin(r64)).max()), float(np.abs(c.astype(F64) - np.cos(r64)).max()))


def test_sincos_restatement_is_within_the_header_claim_of_float64():
    rng = np.random.default_rng(7)
    sweep = np.concatenate([F32(rng.uniform(-65536, 65536, 800000)), F32(rng.uniform(-8, 8, 200000)), F32(rng.uniform(-1.3, 1.3, 100000))])
    e_sweep = _sincos_error(sweep)
    args = np.concatenate([RC.embed_arguments(RC.embed_case(n)).reshape(-1) for n in RC.EMBED_NAMES])
    args = args[np.isfinite(args) & ~RC.is_slow(args)]
    e_cases = _sincos_error(args)
    # every float within 4 ulp of k pi/4 (multiples of pi/2 and the odd multiples of pi/4 between them), |k| <= 83442: up to the switch
    centre = F32(np.arange(-83442, 83443) * (np.pi / 4))
    ring, lo, hi = [centre], centre, centre
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        ring += [lo, hi]
    ring = np.concatenate(ring)
    ring = ring[np.abs(ring) <= 65536]
    e_ring = _sincos_error(ring)
    print("sincos restatement vs float64: %.3e over %d random |r| <= 65536, %.3e over the %d case arguments, %.3e over the %d floats within 4 ulp of "
          "k pi/4" % (e_sweep, sweep.size, e_cases, args.size, e_ring, ring.size))
    assert sweep.size >= 1000000 and ring.size >= 1500000 and e_sweep <= 2e-7 and e_cases <= 2e-7 and e_ring <= 2e-7
    # odd / even symmetry bit for bit, apart from the sign of a zero
    for r in (sweep[:200000], args):
        s, c = RC.sincos_fast32(r)
        sm, cm = RC.sincos_fast32(-r)
        nz = s != 0
        assert np.array_equal(RC.bits(sm)[nz], RC.bits(-s)[nz]) and bool((sm[~nz] == 0).all())
        nz = c != 0
        assert np.array_equal(RC.bits(cm)[nz], RC.bits(c)[nz]) and bool((cm[~nz] == 0).all())
    s, c = RC.sincos_fast32(F32([0.0, -0.0]))
    assert s.tolist() == [0.0, 0.0] and c.tolist() == [1.0, 1.0]


def test_linspace01_is_within_one_ulp_of_torch_linspace():
    differing, worst = 0, 0.0
    for S in LIN_SIZES:
        mine, theirs = RC.linspace01(np.arange(S), S), torch.linspace(0, 1, S).numpy()
        ulp = np.spacing(np.maximum(mine, theirs))
        d = np.abs(mine.astype(F64) - theirs.astype(F64))
        assert bool((d <= ulp).all()), S
        differing += int((d > 0).any())
        worst = max(worst, float(d.max()))
        t64 = torch.linspace(0, 1, S, dtype=torch.float64).numpy()                      # what the float64 reference of the samplers is built on
        assert float(np.abs(t64 - (np.arange(S) / max(S - 1, 1))).max()) <= 2.0 ** -52
    print("linspace01 differs from torch.linspace(0, 1, S) for %d of %d lengths, by at most %.2e" % (differing, len(LIN_SIZES), worst))
    assert worst <= 2.0 ** -24                                                           # 1 ulp of t < 1


# ------------------------------------------------------------------------------------------------ per case
@pytest.mark.parametrize("kind,name", RC.ALL)
def test_case_is_exact_on_lattices_and_a_float32_computation_elsewhere(kind, name):
    c = RC.case(kind, name)                                   # (a lattice builder asserts restatement == float64 element for element)
    assert c["m" if "m" in c else "n"] < 4096
    for k, d in c["dist"].items():
        w = c["want"][k]
        assert w.dtype == F32 and w.shape == c["ref"][k].shape
        if c["lattice"]:
            assert d == 0.0
        else:                                                 # no element is left out; <= 1e-6 of the scale: at most 16 roundings of 2^-24 each, not another result
            assert d <= 1e-6 * max(1.0, c["scale"][k]), (k, d, c["scale"][k])


def test_dir_feature_routes_share_one_restatement():
    for name in RC.DIR_FEATURE_NAMES:
        host, dev = RC.dir_feature_case(name, "host"), RC.dir_feature_case(name, "device")
        assert RC.same_bits(host["want"]["angle"], dev["want"]["angle"]) and RC.same_bits(host["want"]["cos_angle"], RC.dir_feature_case(name, "none")["want"]["cos_angle"])


# ------------------------------------------------------------------------------------------------ the golden fixtures
def _close(a, b, atol=1e-5, rtol=1e-5):
    torch.testing.assert_close(torch.from_numpy(np.array(a, F32)), b.float().reshape(np.shape(a)), atol=atol, rtol=rtol, equal_nan=True)


def test_restatement_reproduces_fixtures_g1_and_g2():
    g = load_golden("g1_raygen")
    H, W = g["H"], g["W"]
    base = dict(lattice=True, xs=None, ys=None, H=H, W=W, K=g["K"].numpy().astype(F32), c2w=g["c2w"].numpy().astype(F32)[:3], opengl=False)
    full = RC.ray_gen32(dict(base, grid_start=0, n=H * W))
    _close(full["rays_d"], g["rays_d"]); _close(full["rays_o"], g["rays_o"])
    assert np.array_equal(full["pix"], g["mvs_full_pix"].numpy())
    part = RC.ray_gen32(dict(base, grid_start=128, n=64))
    _close(part["rays_d"], g["mvs_d"]); assert np.array_equal(part["pix"], g["mvs_pix"].numpy())
    gl = RC.ray_gen32(dict(base, grid_start=0, n=H * W, opengl=True, K=np.full((3, 3), g["gl_focal"], F32)))
    _close(gl["rays_d"], g["gl_d"]); _close(gl["rays_o"], g["gl_o"])
    g = load_golden("g2_ndc_rays")
    c = dict(H=g["H"], W=g["W"], near=F32(g["near"]), rays_o=g["rays_o"].numpy().reshape(-1, 3), rays_d=g["rays_d"].numpy().reshape(-1, 3))
    out = RC.ndc_rays32(dict(c, fx=F32(g["focal2"][0]), fy=F32(g["focal2"][1]), variant=0))
    _close(out["out_o"], g["o_ru"]); _close(out["out_d"], g["d_ru"])
    out = RC.ndc_rays32(dict(c, fx=F32(g["focal"]), fy=F32(g["focal"]), variant=1))
    _close(out["out_o"], g["o_h"]); _close(out["out_d"], g["d_h"])


def test_restatement_reproduces_fixture_g3():
    g = load_golden("g3_sampling")
    rays, S, noise = g["rays"].numpy(), g["S"], g["noise"].numpy()
    near, far = rays[:, 6:7], rays[:, 7:8]
    pts = lambda z: np.stack([rays[:, None, k] + rays[:, None, 3 + k] * z for k in range(3)], -1)
    z = RC.stratified32(near, far, S, 0, 0.0, None)
    _close(z, g["z_det"], 1e-6, 1e-6); _close(pts(z), g["pts_det"], 1e-6, 1e-6)
    _close(RC.stratified32(near, far, S, 1, 0.0, None), g["z_lindisp"], 1e-6, 1e-6)
    z = RC.stratified32(near, far, S, 0, 1.0, noise)
    _close(z, g["z_p1"], 1e-6, 1e-6); _close(pts(z), g["pts_p1"], 1e-5, 1e-5)
    _close(RC.stratified32(near, far, S, 0, 0.5, noise), g["z_p05"], 1e-6, 1e-6)
    # the cascade sampler and the projection, composed as build_rays_test composes them (test_hip_parity.py)
    H, W, NS = g["bt_H"], g["bt_W"], g["bt_NS"]
    K, c2w = g["bt_K"].numpy().astype(F32), g["bt_c2w"].numpy().astype(F32)
    rg = RC.ray_gen32(dict(lattice=True, xs=None, ys=None, H=H, W=W, K=K, c2w=c2w[:3], opengl=False, grid_start=32, n=32))
    _close(rg["rays_d"], g["bt_dir"])
    p = torch.from_numpy(rg["pix"]).long()
    cols = []
    for k, d in (("1", 4), ("2", 2), ("3", 1)):
        dv = g["bt_dv" + k]
        pr, pc = torch.div(p[0], d, rounding_mode="trunc"), torch.div(p[1], d, rounding_mode="trunc")
        cols += [dv[0, 0, pr, pc], dv[0, -1, pr, pc]]
    near_far = torch.stack(cols, -1).numpy().astype(F32)
    out, _ = RC.cascade32(dict(S=NS, near_far=near_far, t_rand=g["bt_t_rand"].numpy().astype(F32), rays_o=c2w[:3, 3], rays_d=rg["rays_d"]))
    _close(out["z"], g["bt_z"], 1e-6, 1e-6); _close(out["pts"], g["bt_pts"], 1e-5, 1e-5)
    c = dict(pts=out["pts"].reshape(-1, 3), has_w2c=1, sample_2d=0, w2c=g["bt_w2c"].numpy().astype(F32)[:3], K=K, inv_scale=F32([W - 1, H - 1]),
             near=F32(g["bt_near_fars"][0, 0]), far=F32(g["bt_near_fars"][0, 1]))
    for i, k in enumerate(("near_1", "far_1", "near_2", "far_2", "near_3", "far_3")):
        c[k] = np.repeat(near_far[:, i], NS)
    proj, _ = RC.ndc_project32(c)
    for k, name in (("stage1", "bt_ndc1"), ("stage2", "bt_ndc2"), ("stage3", "bt_ndc3"), ("ndc", "bt_ndc")):
        _close(proj[k].reshape(32, NS, 3), g[name], 2e-5, 2e-5)


def test_restatement_reproduces_fixtures_g4_and_g5():
    g = load_golden("g4_ndc_coord")
    c = dict(pts=g["pts"].numpy().reshape(-1, 3), has_w2c=1, sample_2d=0, w2c=g["w2c"].numpy().astype(F32)[:3], K=g["K"].numpy().astype(F32),
             inv_scale=g["inv_scale"].numpy().astype(F32).reshape(-1), near=F32(g["near"]), far=F32(g["far"]))
    for k in ("near_1", "far_1", "near_2", "far_2", "near_3", "far_3"):
        c[k] = g[k].numpy().astype(F32).reshape(-1)
    out, _ = RC.ndc_project32(c)
    for k in ("stage1", "stage2", "stage3", "ndc"):
        _close(out[k].reshape(g["out_" + k].shape), g["out_" + k], 1e-5, 5e-5)
    out, _ = RC.ndc_project32(dict(c, sample_2d=1))
    _close(out["ndc"].reshape(g["q2d"].shape), g["q2d"], 1e-5, 5e-5)
    g = load_golden("g5_embed")
    x = g["x"].numpy()
    for key, L, layout in (("live10", 10, 0), ("live4", 4, 0), ("inter10", 10, 1), ("inter4", 4, 1)):
        _close(RC.embed32(x, L, layout)[0], g[key], 2e-6, 0)


# ------------------------------------------------------------------------------------------------ census: every case hits its edge
def test_census_of_the_sampler_cases():
    S_odd = [S for S in RC.STRAT_S if S % 2 and S > 1]
    assert S_odd == [3, 5, 65]
    for S in S_odd + [4, 64]:                                 # both branches of linspace01, the midpoint S / 2 on the upper one
        i = np.arange(S)
        assert (i < S // 2).any() and (i >= S // 2).any()
    # S = 4 and 64: the two branches differ AT the midpoint (a power-of-two step hides a switch on the wrong side)
    for S in (4, 64):
        step = F32(1) / F32(S - 1)
        assert step * F32(S // 2) != F32(1) - step * F32(S - 1 - S // 2)
    names = RC.STRAT_NAMES
    assert {RC.stratified_case(n)["S"] for n in names} == set(RC.STRAT_S)
    assert {(RC.stratified_case(n)["form"], RC.stratified_case(n)["lindisp"]) for n in names} == {("rays", 0), ("rays", 1), ("scalar", 0), ("scalar", 1)}
    assert {RC.stratified_case(n)["perturb"] for n in names} == {0.0, 0.5, 1.0}
    top = RC.stratified_case("S5_rays_disp_p0.5_top")["noise"]
    assert float(top.max()) == 1 - 2.0 ** -24 < 1 and float(RC.stratified_case("S5_rays_lin_p1_zero")["noise"].max()) == 0.0
    assert all((c["n"] * c["S"]) % 256 for c in map(RC.stratified_case, names) if c["S"] > 1)
    assert all(S == 1 or (n * S) % 256 for n, S in ((300, 1), (85, 3), (5, 257), (37, 7))) and 5 * 257 > 256


def test_census_of_the_cascade_cases():
    for S in RC.CASCADE_S:
        c = RC.cascade_case("S%d_rand" % S)
        v = c["unsorted"]
        assert v.shape == (6, S) and c["layouts"] == RC.CASCADE_LAYOUTS
        P = 1 << (S - 1).bit_length()
        assert {3: 4, 6: 8, 9: 16, 63: 64, 192: 256, 384: 512, 387: 512, 765: 1024, 768: 1024}[S] == P
        ties = [S - len(np.unique(row)) for row in v]
        assert ties[3] >= 2 * (S // 3) and sum(ties) > 0                    # identical stages: every value three times
        n3 = S // 3
        assert bool((np.diff(v[0]) >= 0).all()) and not bool((np.diff(v[4]) >= 0).all())          # ascending as built / stages in descending order
        assert v[5, n3] > v[5, 2 * n3 - 1] or n3 == 1                       # one stage runs from far down to near
        z = RC.cascade_case("S%d_null" % S)["want"]["z"]
        assert bool((np.diff(z, axis=1) >= 0).all())                        # sorted output is non-decreasing
    assert RC.cascade_case("S3_rand")["S"] // 3 == 1                        # n3 = 1: linspace01(j, 1)
    assert 1024 - 765 == 259 and 1024 - 768 == 256               # padding slots of the two lengths that sort 1024 values


def test_census_of_the_clamp_case():
    c = RC.ndc_project_case("clamp")
    d = c["depths"]
    t = RC.CLAMP
    assert float(t) < 1e-4                                    # 1e-4f lies below the double 1e-4
    inside, at, outside = np.abs(d) < t, np.abs(d) == t, np.abs(d) > t
    assert inside.sum() >= 12 and at.sum() == 6 and outside.sum() >= 12 and (d[at] > 0).any() and (d[at] < 0).any()
    assert np.nextafter(t, F32(0)) in d and np.nextafter(t, F32(1)) in d and -np.nextafter(t, F32(0)) in d
    cz = c["cz"]
    assert bool((cz[inside] == t).all()) and np.array_equal(RC.bits(cz[~inside]), RC.bits(d[~inside]))      # clamped to +1e-4f (sign dropped); '<' is strict
    assert bool((cz[at & (d < 0)] == -t).all())
    assert bool((cz[inside & (d < 0)] > 0).all())             # a '<=' would move the points at the threshold, and change the sign of the negative ones
    e = RC.ndc_project_case("m64_equal_range")
    assert np.isinf(e["want"]["stage2"][5, 2]) and np.isfinite(e["want"]["stage1"]).all() and np.isfinite(np.delete(e["want"]["stage2"], 5, 0)).all()


def test_census_of_the_embed_cases():
    c = RC.embed_case("edges_lay0")
    r = RC.embed_arguments(c)                                 # [m, L, 3]
    slow = RC.is_slow(r)
    # the kernel's threads: one per (vector, frequency slot), 64 consecutive ones are a wave
    lanes = np.concatenate([slow.any(-1), np.zeros((c["m"], 1), bool)], 1).reshape(-1)
    fast_lanes = np.concatenate([(~slow).any(-1), np.ones((c["m"], 1), bool)], 1).reshape(-1)
    groups = range(0, lanes.size - 63, 64)
    assert any(lanes[g:g + 64].any() and fast_lanes[g:g + 64].any() for g in groups)
    x = c["x"].reshape(-1)
    assert (RC.bits(x) == 0).any() and (RC.bits(x) == 0x80000000).any() and np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert (r == 65536.0).any() and (r == -65536.0).any() and not slow[r == 65536.0].any()          # x = 64, k = 10: exactly at the switch, fast
    above = np.nextafter(F32(65536), F32(np.inf))
    assert (r[:, 0] == above).any() and slow[:, 0][r[:, 0] == above].all() and (r[:, 0] == -above).any()
    # quadrants: all four residues mod 4 with k > 2^15, at multiples and at odd multiples of pi/4
    r0 = r[:, 0][np.isfinite(r[:, 0]) & ~slow[:, 0]].astype(F64)
    k = np.rint(r0 / (np.pi / 2)).astype(np.int64)
    near_multiple = np.abs(r0 - k * np.pi / 2) < 1e-2
    assert {int(v) % 4 for v in k[near_multiple & (k > 2 ** 15)]} == {0, 1, 2, 3}
    assert {int(v) % 4 for v in k[near_multiple & (k < -2 ** 15)]} == {0, 1, 2, 3}
    assert int(np.abs(k[near_multiple]).max()) == 41721 and int((np.abs(np.abs(r0 / (np.pi / 2) % 1) - 0.5) < 1e-3).sum()) >= 100
    assert {RC.embed_case(n)["n_freqs"] for n in RC.EMBED_NAMES} == set(RC.EMBED_FREQS)
    assert {(RC.embed_case(n)["layout"], RC.embed_case(n)["m"]) for n in RC.EMBED_NAMES} >= {(l, m) for l in (0, 1) for m in RC.EMBED_MS}
    assert float(np.abs(RC.embed_case("fixture_range_lay0")["x"]).max()) > 500 and RC.embed_case("L10_lay0_3d")["shape"] == (4, 5, 3)
    nan_row = np.argwhere(np.isnan(c["x"]))[0]
    w = c["want"]["out"][nan_row[0]]
    assert np.isnan(w[nan_row[1]]) and np.isnan(w[3 + nan_row[1]]) and np.isfinite(np.delete(c["want"]["out"], [i for i in range(c["m"]) if not np.isfinite(c["x"][i]).all()], 0)).all()


def test_census_of_the_ray_and_direction_cases():
    sizes = {(c["H"], c["W"], c["grid_start"], c["n"]) for c in map(RC.ray_gen_case, RC.RAY_GEN_NAMES) if c["xs"] is None}
    assert {(5, 7, 10, 1), (5, 7, 10, 2), (5, 7, 10, 25), (20, 16, 3, 255), (20, 16, 3, 256), (20, 16, 3, 257)} <= sizes and 10 % 7 and 10 + 25 == 35
    p = RC.ray_gen_case("pixels")
    assert (p["xs"] < 0).any() and (p["ys"] < 0).any() and (p["xs"] % 1 != 0).any() and p["K"][0, 0] != p["K"][1, 1]
    assert {c["opengl"] for c in map(RC.ray_gen_case, RC.RAY_GEN_NAMES)} == {True, False} and len(RC.OUTPUT_SUBSETS) == 8
    assert {RC.dir_feature_case(n)["repeat"] for n in RC.DIR_FEATURE_NAMES} == {0, 1, 2, 5}
    z = RC.dir_feature_case("zero_direction")
    a = z["want"]["angle"].reshape(z["n"], 2, 3)
    assert np.isnan(a[40]).all() and np.isfinite(np.delete(a, 40, 0)).all() and z["want"]["cos_angle"][40] == 0
    v = {n: RC.ndc_rays_case(n) for n in RC.NDC_RAYS_NAMES}
    assert v["v0"]["fx"] != v["v0"]["fy"] and (v["v0"]["rays_d"][:, 2] > 0).any() and (v["v0"]["rays_d"][:, 2] < 0).any()
    # FINDING: no well-conditioned input tells the two variants apart.  They differ only in out_d[:, 2] = 1 - o2 against -a, with o2 = 1 + a and
    # a = 2 near / o_z.  The warp has moved the origin to the near plane, so o_z = -near up to rounding and a is within rounding of -2; for every
    # float32 a in [-4, -1] the sum 1 + a is exact (it lies in a's binade or the one below) and so is 1 - (1 + a): the same bits as -a.
    for name in RC.NDC_RAYS_NAMES:
        c = v[name]
        a = c["want"]["out_o"][:, 2] - F32(1)                 # o2 - 1, exact
        assert bool(((a >= -4) & (a <= -1)).all()), name
        other = RC.ndc_rays32(dict(c, variant=1 - c["variant"]))["out_d"]
        assert RC.same_bits(other, c["want"]["out_d"]), name
    a = F32(np.random.default_rng(3).uniform(-4, -1, 200000))
    assert np.array_equal(RC.bits(F32(1) - (F32(1) + a)), RC.bits(-a))
    assert len(RC.STAGE_SUBSETS) == 15 and {RC.ndc_project_case(n)["m"] for n in RC.NDC_PROJECT_NAMES} >= {1, 255, 257}


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_einval_in_a_child_process():
    """Probed through ctypes in a child (a crash must not take the run with it): every check comes before anything could be launched."""
    from uc_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no library is built")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rays_probe.py")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, "the probe died (exit %d): %s" % (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["calls"] >= 40 and not out["problems"], out["problems"]
