"""Child process of tests/test_build_rays_train_host.py: ucnerf_build_rays_train called with every argument error include/ucnerf_hip.h lists.  Each
must return UCNERF_EINVAL (-1) with a message and never crash or launch (runs without a GPU: a call that passed validation would need a device); a
call of zero rays must return 0 the same way.  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first
INPUTS = ("K", "c2w", "w2c_ref", "K_ref", "near_far_ref", "imgs")
OUTPUTS = ("rays_o", "rays_d", "colors", "pix", "z", "pts", "ndc1", "ndc2", "ndc3", "ndc")


def params(**kw):
    """A valid call: 24 x 32 image, 4 patches of 4 x 4, 26 uniform pixels, 7 coordinates, 12 samples."""
    p = L.BuildRaysTrainParams()
    p.S, p.H, p.W, p.P, p.ps, p.n_uniform, p.n_coord, p.coord_stride = 12, 24, 32, 4, 4, 26, 7, 2
    for k, (d, h, w) in enumerate(((5, 6, 8), (4, 12, 16), (3, 24, 32))):
        p.dv_d[k], p.dv_h[k], p.dv_w[k], p.depth_values[k] = d, h, w, PTR
    p.img_stride_c, p.img_stride_h, p.img_stride_w = 24 * 32, 32, 1
    for name in INPUTS + OUTPUTS + ("sel0", "sel1", "shift", "ux", "uy", "coords", "t_rand", "near_far"):
        setattr(p, name, PTR)
    for k, v in kw.items():
        if isinstance(v, tuple):                    # (index, value) of an array field
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(what, p, needle=None, want=EINVAL):
        out["calls"] += 1
        rc = lib.ucnerf_build_rays_train(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != want or (want == EINVAL and (not msg or (needle and needle not in msg))):
            out["problems"].append("%s returned %d (%r)" % (what, rc, msg[:160]))

    expect("NULL params", None, b"null params")
    for name in INPUTS:
        expect("NULL " + name, params(**{name: None}), b"null input")
    for k in range(3):
        expect("NULL depth_values[%d]" % k, params(depth_values=(k, None)), b"null input")
    for name in ("sel0", "sel1", "shift", "ux", "uy", "coords"):
        expect("NULL " + name, params(**{name: None}), b"null input")
    for name in OUTPUTS:
        expect("NULL " + name, params(**{name: None}), b"null output")
    for name in ("P", "n_uniform", "n_coord"):
        expect(name + " = -2", params(**{name: -2}), b"negative count")
    for P in (1, 3):
        expect("P = %d" % P, params(P=P), b"even")
    for ps in (0, -1):
        expect("ps = %d" % ps, params(ps=ps), b"ps = ")
    expect("H / ps < 2", params(ps=13), b"no two cells")
    expect("W / ps < 2", params(H=64, ps=17, dv_h=(2, 64)), b"no two cells")
    for S in (0, 2, 13, 771, -3):
        expect("S = %d" % S, params(S=S), b"S = ")
    for k, (h, w) in enumerate(((5, 7), (11, 15), (23, 31))):
        expect("depth_values[%d] one row short" % k, params(dv_h=(k, h)), b"the image needs at least")
        expect("depth_values[%d] one column short" % k, params(dv_w=(k, w)), b"the image needs at least")
    expect("depth_values[0] without planes", params(dv_d=(0, 0)), b"the image needs at least")
    expect("R S 3 overflows", params(n_uniform=2 ** 31 - 1, S=768), b"overflow")
    expect("R S 3 overflows by the patches", params(P=2 ** 30, S=3), b"overflow")
    expect("R 6 overflows", params(n_coord=2 ** 30, S=3), b"overflow")
    expect("huge patches", params(H=2 ** 20, W=2 ** 20, ps=2 ** 18), b"overflow")
    # zero rays: success, nothing launched, no pointer looked at (there is no device here to launch on); an empty segment's arrays may be NULL --
    # such a call passes validation and would launch, so it is covered on the GPU
    expect("no rays", params(P=0, n_uniform=0, n_coord=0), want=0)
    expect("no rays, NULL everything", params(P=0, n_uniform=0, n_coord=0, K=None, imgs=None, rays_d=None, pix=None), want=0)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
