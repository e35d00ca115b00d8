"""Child process of tests/test_rays_cases_host.py: the eight ray front-end entry points of csrc/rays.hip called with every argument error that
tests/abi_null_probe.py does not already cover.  Each must return UCNERF_EINVAL (-1) with a message and never crash or launch; a count of zero
succeeds with NULL arrays (runs without a GPU: a call that passed validation with a positive count would need a device).  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first
INT_MAX = 2 ** 31 - 1


def make(cls, **kw):
    p = cls()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def ray_gen(**kw):
    return make(L.RayGenParams, **dict(dict(n=4, H=5, W=7, grid_start=10, rays_d=PTR), **kw))


def strat(**kw):
    return make(L.SampleStratifiedParams, **dict(dict(n=4, S=3, near=1.0, far=2.0, z=PTR), **kw))


def cascade(**kw):
    return make(L.SampleCascadeParams, **dict(dict(n=4, S=6, near_far=PTR, z=PTR), **kw))


def project(**kw):
    base = dict(m=4, has_w2c=1, nf_stride=1, pts=PTR, out_ndc=PTR)
    for s in (1, 2, 3):
        base.update({"near_%d" % s: PTR, "far_%d" % s: PTR, "out_stage%d" % s: PTR})
    return make(L.NdcProjectParams, **dict(base, **kw))


def embed(**kw):
    return make(L.EmbedParams, **dict(dict(m=4, n_freqs=10, layout=0, x=PTR, out=PTR), **kw))


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(fn, what, args, needle=None, want=EINVAL):
        out["calls"] += 1
        rc = getattr(lib, fn)(*[C.addressof(a) for a in args], None)
        msg = lib.ucnerf_last_error() or b""
        if rc != want or (want != 0 and (not msg or (needle and needle not in msg))):
            out["problems"].append("%s %s returned %d (%r)" % (fn, what, rc, msg[:160]))

    # ray_gen
    expect("ucnerf_ray_gen", "n < 0", [ray_gen(n=-1)], b"n < 0")
    expect("ucnerf_ray_gen", "n > INT_MAX / 3", [ray_gen(n=INT_MAX // 3 + 1, xs=PTR, ys=PTR)], b"overflow")
    expect("ucnerf_ray_gen", "xs without ys", [ray_gen(xs=PTR)], b"xs and ys")
    expect("ucnerf_ray_gen", "ys without xs", [ray_gen(ys=PTR)], b"xs and ys")
    expect("ucnerf_ray_gen", "grid range past H*W by one", [ray_gen(n=26)], b"grid range")
    expect("ucnerf_ray_gen", "grid range ending at H*W, NULL rays_d", [ray_gen(n=25, rays_d=None)], b"null rays_d")
    expect("ucnerf_ray_gen", "n = 0", [make(L.RayGenParams)], want=0)
    # ray_gen_sample
    expect("ucnerf_ray_gen_sample", "n mismatch", [ray_gen(), strat(n=5)], b"4 rays but depths for 5")
    expect("ucnerf_ray_gen_sample", "S = 0", [ray_gen(), strat(S=0)], b"S < 1")
    expect("ucnerf_ray_gen_sample", "rays set", [ray_gen(), strat(rays=PTR)], b"scalar near / far")
    expect("ucnerf_ray_gen_sample", "pts set", [ray_gen(), strat(pts=PTR)], b"scalar near / far")
    expect("ucnerf_ray_gen_sample", "perturb without noise", [ray_gen(), strat(perturb=1.0)], b"noise")
    expect("ucnerf_ray_gen_sample", "grid range past H*W by one", [ray_gen(n=26), strat(n=26)], b"grid range")
    expect("ucnerf_ray_gen_sample", "n = 0", [make(L.RayGenParams), make(L.SampleStratifiedParams)], want=0)
    # ndc_rays
    nr = dict(n=4, H=5, W=7, focal_x=1.0, focal_y=1.0, near=1.0, rays_o=PTR, rays_d=PTR, out_o=PTR, out_d=PTR)
    expect("ucnerf_ndc_rays", "variant 2", [make(L.NdcRaysParams, **dict(nr, variant=2))], b"variant 2")
    expect("ucnerf_ndc_rays", "variant -1", [make(L.NdcRaysParams, **dict(nr, variant=-1))], b"variant -1")
    expect("ucnerf_ndc_rays", "n = 0", [make(L.NdcRaysParams)], want=0)
    # dir_feature
    expect("ucnerf_dir_feature", "n = -1", [make(L.DirFeatureParams, n=-1, rays_d=PTR, angle=PTR)], b"negative count")
    expect("ucnerf_dir_feature", "n = 0", [make(L.DirFeatureParams)], want=0)
    # sample_stratified
    expect("ucnerf_sample_stratified", "pts without rays", [strat(pts=PTR)], b"needs the rays array")
    expect("ucnerf_sample_stratified", "S = 0", [strat(S=0)], b"S = 0")
    expect("ucnerf_sample_stratified", "perturb without noise", [strat(perturb=0.5)], b"noise")
    expect("ucnerf_sample_stratified", "n = 0", [make(L.SampleStratifiedParams)], want=0)
    # sample_cascade
    for S in (0, 4, 771):
        expect("ucnerf_sample_cascade", "S = %d" % S, [cascade(S=S)], b"S = %d" % S)
    expect("ucnerf_sample_cascade", "pts without rays_o / rays_d", [cascade(pts=PTR)], b"pts needs")
    expect("ucnerf_sample_cascade", "pts without rays_d", [cascade(pts=PTR, rays_o=PTR)], b"pts needs")
    expect("ucnerf_sample_cascade", "n = 0", [make(L.SampleCascadeParams)], want=0)
    # ndc_project
    expect("ucnerf_ndc_project", "nf_stride 2", [project(nf_stride=2)], b"nf_stride 2")
    expect("ucnerf_ndc_project", "sample_2d without out_ndc", [project(sample_2d=1, out_ndc=None)], b"sample_2d needs out_ndc")
    expect("ucnerf_ndc_project", "no outputs", [project(out_stage1=None, out_stage2=None, out_stage3=None, out_ndc=None)], b"no outputs")
    for s in (1, 2, 3):
        for side in ("near", "far"):
            expect("ucnerf_ndc_project", "stage %d without %s" % (s, side), [project(**{"%s_%d" % (side, s): None})], b"without its near/far")
    expect("ucnerf_ndc_project", "m = 0", [make(L.NdcProjectParams)], want=0)
    # embed
    for nf in (-1, 31):
        expect("ucnerf_embed", "n_freqs %d" % nf, [embed(n_freqs=nf)], b"n_freqs %d" % nf)
    expect("ucnerf_embed", "layout 2", [embed(layout=2)], b"layout 2")
    expect("ucnerf_embed", "m = 0", [make(L.EmbedParams)], want=0)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
