"""The ray front end on the GPU (csrc/rays.hip: ucnerf_ray_gen, ucnerf_ray_gen_sample, ucnerf_ndc_rays, ucnerf_dir_feature,
ucnerf_sample_stratified, ucnerf_sample_cascade, ucnerf_ndc_project, ucnerf_embed) against the float32 numpy restatement of tests/rays_cases.py.

Every output of every case is compared BIT FOR BIT (uint32 view; NaN matches NaN; the sign of a zero counts): the kernels' arithmetic is
+ - * /, sqrtf, fmaf, rintf and conversions, each correctly rounded on both sides (profiles/ray_edges.md).  The one exception is the embedding's
slots whose argument exceeds 65536: they go through OCML's sincosf, which cannot be restated, and are held to float64 under 2e-6 absolute (the
bar of test_hip_parity.py::test_embedders_both_layouts_large_arguments).  Every output is allocated with 64 floats of -7.0 behind it, which must
stay untouched; optional outputs passed as NULL change nothing else.  The entry points are driven through the C ABI (ctypes), because the torch
wrappers do not expose every option (repeat, NULL cos_angle, output subsets)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rays_cases as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32, F64 = np.float32, np.float64
SLOW_BAR = 2e-6


def L():
    from uc_nerf_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.array(a, dtype=F32)).to(DEV).contiguous()      # (a copy: the cached cases are read-only)


class Out:
    """A device output of prod(shape) floats with RC.GUARD floats of -7.0 behind it."""

    def __init__(self, *shape):
        self.shape, self.count = shape, int(np.prod(shape))
        self.t = torch.full((self.count + RC.GUARD,), -7.0, device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        a = self.t.cpu().numpy()
        assert (a[self.count:] == -7.0).all(), "the guard behind an output was written"
        return a[:self.count].reshape(self.shape)


def call(name, *params):
    lib = L().lib()
    rc = getattr(lib, name)(*[C.addressof(p) for p in params], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc, lib.ucnerf_last_error())
    torch.cuda.synchronize()


def fill(dst, src):
    for i, v in enumerate(np.asarray(src, F32).reshape(-1)):
        dst[i] = float(v)


def check(case, got, only=None):
    for k, want in case["want"].items():
        if only is not None and k not in only:
            continue
        slow = case.get("slow", {}).get(k)
        g = got[k].reshape(want.shape)
        if slow is None:
            bad = ~((RC.bits(g) == RC.bits(want)) | ((g != g) & (want != want)))
            assert not bad.any(), (case["kind"], case["name"], k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], want[bad][:6])
            continue
        fast = ~slow
        bad = fast & ~((RC.bits(g) == RC.bits(want)) | ((g != g) & (want != want)))
        assert not bad.any(), (case["kind"], case["name"], k, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6], want[bad][:6])
        ref = case["ref"][k]
        fin = slow & np.isfinite(ref)
        assert bool(np.isnan(g[slow & ~np.isfinite(ref)]).all())                     # sin / cos of +-inf: NaN
        with np.errstate(invalid="ignore"):
            err = float(np.abs(g.astype(F64) - ref)[fin].max()) if fin.any() else 0.0
        print("%s %s: %d slots through sincosf, largest distance from float64 %.3e" % (case["kind"], case["name"], int(fin.sum()), err))
        assert err <= SLOW_BAR, (case["name"], err)


# ------------------------------------------------------------------------------------------------ ray_gen
def ray_gen_params(c, outputs):
    p = L().RayGenParams()
    p.n, p.H, p.W, p.grid_start, p.opengl = c["n"], c["H"], c["W"], c["grid_start"], int(c["opengl"])
    fill(p.K, c["K"]); fill(p.c2w, c["c2w"]); fill(p.w2c_dir, c["w2c_dir"])
    keep = []
    if c["xs"] is not None:
        keep = [dev(c["xs"]), dev(c["ys"])]
        p.xs, p.ys = keep[0].data_ptr(), keep[1].data_ptr()
    outs = {"rays_d": Out(c["n"], 3)}
    if "rays_o" in outputs:
        outs["rays_o"] = Out(c["n"], 3)
    if "pix" in outputs:
        outs["pix"] = Out(2, c["n"])
    if "angle" in outputs:
        outs["angle"] = Out(c["n"], 3)
    for k, o in outs.items():
        setattr(p, k, o.ptr)
    return p, outs, keep


def run_ray_gen(c, outputs):
    p, outs, keep = ray_gen_params(c, outputs)
    call("ucnerf_ray_gen", p)
    return {k: o.get() for k, o in outs.items()}


@pytest.mark.parametrize("name", RC.RAY_GEN_NAMES)
def test_ray_gen_bit_for_bit(name):
    c = RC.ray_gen_case(name)
    outputs = ("rays_o", "pix") + (() if c["lattice"] else ("angle",))
    check(c, run_ray_gen(c, outputs))


@pytest.mark.parametrize("outputs", RC.OUTPUT_SUBSETS, ids=lambda s: "+".join(s) or "rays_d_only")
def test_ray_gen_every_subset_of_the_optional_outputs(outputs):
    for name in ("pixels", "grid20x16_n257"):
        c = RC.ray_gen_case(name)
        got = run_ray_gen(c, outputs)
        assert set(got) == {"rays_d"} | set(outputs)
        check(c, got, only=set(got))


def test_ray_gen_of_no_rays_writes_nothing():
    c = dict(RC.ray_gen_case("pixels"), n=0, xs=None, ys=None)
    p, outs, _ = ray_gen_params(c, ("rays_o", "pix", "angle"))
    call("ucnerf_ray_gen", p)
    assert all((o.t == -7.0).all() for o in outs.values())


# ------------------------------------------------------------------------------------------------ ray_gen_sample
def stratified_params(c, z, pts=None):
    p = L().SampleStratifiedParams()
    p.n, p.S, p.lindisp, p.perturb = c["n"], c["S"], int(c["lindisp"]), float(c["perturb"])
    keep = []
    if c.get("form") == "rays":
        keep.append(dev(c["rays"]))
        p.rays = keep[-1].data_ptr()
    else:
        p.near, p.far = (float(c["near"]), float(c["far"])) if "near" in c else (float(c["rays"][0, 6]), float(c["rays"][0, 7]))
    if c["perturb"] > 0:
        keep.append(dev(c["noise"]))
        p.noise = keep[-1].data_ptr()
    p.z = z.ptr
    if pts is not None:
        p.pts = pts.ptr
    return p, keep


@pytest.mark.parametrize("name", RC.RAY_GEN_SAMPLE_NAMES)
def test_ray_gen_sample_equals_the_two_launches_bit_for_bit(name):
    c = RC.ray_gen_sample_case(name)
    rg, outs, keep = ray_gen_params(c, ("angle",))
    z = Out(c["n"], c["S"])
    ss, keep2 = stratified_params(c, z)
    call("ucnerf_ray_gen_sample", rg, ss)
    fused = {"rays_d": outs["rays_d"].get(), "angle": outs["angle"].get(), "z": z.get()}
    check(c, fused)
    # the two stand-alone launches on the same inputs
    two = run_ray_gen(c, ("angle",))
    z2 = Out(c["n"], c["S"])
    ss2, keep3 = stratified_params(c, z2)
    call("ucnerf_sample_stratified", ss2)
    assert RC.same_bits(two["rays_d"], fused["rays_d"]) and RC.same_bits(two["angle"], fused["angle"]) and RC.same_bits(z2.get(), fused["z"])


# ------------------------------------------------------------------------------------------------ ndc_rays
@pytest.mark.parametrize("name", RC.NDC_RAYS_NAMES)
def test_ndc_rays_bit_for_bit(name):
    c = RC.ndc_rays_case(name)
    p = L().NdcRaysParams()
    p.n, p.H, p.W, p.variant = c["n"], c["H"], c["W"], c["variant"]
    p.focal_x, p.focal_y, p.near = float(c["fx"]), float(c["fy"]), float(c["near"])
    o, d, out_o, out_d = dev(c["rays_o"]), dev(c["rays_d"]), Out(c["n"], 3), Out(c["n"], 3)
    p.rays_o, p.rays_d, p.out_o, p.out_d = o.data_ptr(), d.data_ptr(), out_o.ptr, out_d.ptr
    call("ucnerf_ndc_rays", p)
    check(c, {"out_o": out_o.get(), "out_d": out_d.get()})


# ------------------------------------------------------------------------------------------------ dir_feature
def run_dir_feature(c, route, with_cos):
    p = L().DirFeatureParams()
    p.n, p.repeat = c["n"], c["repeat"]
    d = dev(c["rays_d"])
    angle, cos = Out(c["n"] * max(c["repeat"], 1), 3), Out(c["n"])
    p.rays_d, p.angle = d.data_ptr(), angle.ptr
    if with_cos:
        p.cos_angle = cos.ptr
    m = None
    if route == "host":
        p.has_ref = 1
        fill(p.w2c_ref, c["w2c_ref"])
    elif route == "device":
        m = dev(c["w2c_ref"])
        p.w2c_ref_dev = m.data_ptr()
    call("ucnerf_dir_feature", p)
    if not with_cos:
        assert (cos.t == -7.0).all()
    return {"angle": angle.get(), "cos_angle": cos.get()}


@pytest.mark.parametrize("name", RC.DIR_FEATURE_NAMES)
def test_dir_feature_every_route_bit_for_bit(name):
    got = {}
    for route in RC.DIR_ROUTES:
        c = RC.dir_feature_case(name, route)
        got[route] = run_dir_feature(c, route, True)
        check(c, got[route])
        without = run_dir_feature(c, route, False)                # cos_angle NULL: the feature is the same, nothing else is written
        assert RC.same_bits(without["angle"], got[route]["angle"])
    assert RC.same_bits(got["host"]["angle"], got["device"]["angle"])                # the two matrix routes: the same bits
    assert RC.same_bits(got["host"]["cos_angle"], got["none"]["cos_angle"]) and RC.same_bits(got["device"]["cos_angle"], got["none"]["cos_angle"])


# ------------------------------------------------------------------------------------------------ sample_stratified
@pytest.mark.parametrize("name", RC.STRAT_NAMES)
def test_sample_stratified_bit_for_bit(name):
    c = RC.stratified_case(name)
    z = Out(c["n"], c["S"])
    pts = Out(c["n"], c["S"], 3) if c["form"] == "rays" else None
    p, keep = stratified_params(c, z, pts)
    call("ucnerf_sample_stratified", p)
    got = {"z": z.get()}
    if pts is not None:
        got["pts"] = pts.get()
        z_only = Out(c["n"], c["S"])                               # pts NULL: the same depths
        p2, keep2 = stratified_params(c, z_only)
        call("ucnerf_sample_stratified", p2)
        assert RC.same_bits(z_only.get(), got["z"])
    check(c, got)


# ------------------------------------------------------------------------------------------------ sample_cascade
@pytest.mark.parametrize("name", RC.CASCADE_NAMES)
def test_sample_cascade_bit_for_bit(name):
    c = RC.cascade_case(name)
    n, S = c["n"], c["S"]
    keep = [dev(c["near_far"]), dev(c["rays_o"]), dev(c["rays_d"])]
    if c["t_rand"] is not None:
        keep.append(dev(c["t_rand"]))

    def run(with_pts):
        p = L().SampleCascadeParams()
        p.n, p.S, p.near_far = n, S, keep[0].data_ptr()
        if c["t_rand"] is not None:
            p.t_rand = keep[3].data_ptr()
        z, pts = Out(n, S), Out(n, S, 3)
        p.z = z.ptr
        if with_pts:
            p.rays_o, p.rays_d, p.pts = keep[1].data_ptr(), keep[2].data_ptr(), pts.ptr
        call("ucnerf_sample_cascade", p)
        if not with_pts:
            assert (pts.t == -7.0).all()
        return {"z": z.get(), "pts": pts.get()}

    got = run(True)
    check(c, got)
    assert RC.same_bits(run(False)["z"], got["z"])
    if c["t_rand"] is None:
        assert bool((np.diff(got["z"], axis=1) >= 0).all())       # sorted depths are non-decreasing


# ------------------------------------------------------------------------------------------------ ndc_project
def run_ndc_project(c, subset):
    p = L().NdcProjectParams()
    m = c["m"]
    p.m, p.has_w2c, p.sample_2d, p.nf_stride = m, c["has_w2c"], c["sample_2d"], c["nf_stride"]
    fill(p.w2c, c["w2c"]); fill(p.K, c["K"]); fill(p.inv_scale, c["inv_scale"])
    p.near, p.far = float(c["near"]), float(c["far"])
    keep = [dev(c["pts"])]
    p.pts = keep[0].data_ptr()
    for s in (1, 2, 3):
        for side in ("near", "far"):
            keep.append(dev(c["%s_%d" % (side, s)]))
            setattr(p, "%s_%d" % (side, s), keep[-1].data_ptr())
    outs = {k: Out(m, 3) for k in ("stage1", "stage2", "stage3", "ndc")}
    for k in subset:
        setattr(p, "out_" + k, outs[k].ptr)
    call("ucnerf_ndc_project", p)
    for k in outs:
        if k not in subset:
            assert (outs[k].t == -7.0).all()
    return {k: outs[k].get() for k in subset}


@pytest.mark.parametrize("name", RC.NDC_PROJECT_NAMES)
def test_ndc_project_bit_for_bit(name):
    c = RC.ndc_project_case(name)
    subset = ("ndc",) if c["sample_2d"] else ("stage1", "stage2", "stage3", "ndc")
    check(c, run_ndc_project(c, subset))


@pytest.mark.parametrize("subset", RC.STAGE_SUBSETS, ids="+".join)
def test_ndc_project_every_subset_of_the_outputs(subset):
    c = RC.ndc_project_case("m255_w2c")
    got = run_ndc_project(c, subset)
    assert set(got) == set(subset)
    check(c, got, only=set(subset))


# ------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("name", RC.EMBED_NAMES)
def test_embed_bit_for_bit_and_the_slow_path_against_float64(name):
    c = RC.embed_case(name)
    width = 3 + 6 * c["n_freqs"]
    p = L().EmbedParams()
    x, out = dev(c["x"].reshape(c["shape"])), Out(c["m"], width)
    p.m, p.n_freqs, p.layout, p.x, p.out = c["m"], c["n_freqs"], c["layout"], x.data_ptr(), out.ptr
    call("ucnerf_embed", p)
    got = out.get()
    check(c, {"out": got})
    assert RC.same_bits(got[:, :3], c["x"])                       # the pass-through x is copied unchanged, NaN and +-inf included
    if len(c["shape"]) == 3:                                      # the torch wrapper on a 3-D input: the same bits, shaped [4, 5, width]
        from uc_nerf_amd import ops
        via = ops.embed(x, c["n_freqs"], c["layout"])
        assert tuple(via.shape) == (4, 5, width) and RC.same_bits(via.cpu().numpy().reshape(-1, width), got)
