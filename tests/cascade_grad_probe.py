"""Child process of tests/test_cascade_grad_host.py: ucnerf_depth_hypotheses_bwd, its scratch-size query and ucnerf_depth_regress_bwd_values
called with every argument error include/ucnerf_hip.h lists.  Each must return UCNERF_EINVAL (-1) with a message and never crash or launch
(runs without a GPU: a call that passed validation would need a device; the pointers handed over are not addresses of anything, so reading one
would end the child); an empty gradient / an empty volume must return 0 the same way.  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def hyp(**kw):
    bp = L.DepthHypothesesBwdParams()
    p = bp.fwd
    p.D, p.h, p.w, p.pad, p.H, p.W, p.h0, p.w0, p.D_in, p.k = 8, 16, 20, 1, 32, 40, 8, 10, 0, 1.0 / 48
    p.cur_depth = p.near_far = PTR
    bp.g_out = bp.scratch = bp.g_cur_depth = PTR
    for k, v in kw.items():
        setattr(bp if k in ("g_out", "scratch", "g_cur_depth") else p, k, v)
    return bp


def reg(**kw):
    p = L.DepthRegressBwdValuesParams()
    p.D, p.Hp, p.Wp, p.pad = 8, 12, 14, 2
    p.prob_volume = p.g_depth = p.g_depth_values = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(fn, what, p, needle=None, want=EINVAL):
        out["calls"] += 1
        rc = getattr(lib, fn)(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != want or (want == EINVAL and (not msg or (needle and needle not in msg))):
            out["problems"].append("%s: %s returned %d (%r)" % (fn, what, rc, msg[:160]))

    H = "ucnerf_depth_hypotheses_bwd"
    expect(H, "NULL params", None, b"null params")
    for field in ("D", "h", "w", "pad", "H", "W", "h0", "w0", "D_in"):
        expect(H, "%s = -1" % field, hyp(**{field: -1}), b"negative size")
    for D in (0, 1):
        expect(H, "D = %d" % D, hyp(D=D), b"D = ")
    expect(H, "h > H", hyp(h=33), b"must cover")
    expect(H, "w > W", hyp(w=41), b"must cover")
    expect(H, "h0 > H", hyp(h0=33), b"must cover")
    expect(H, "w0 > W", hyp(w0=41), b"must cover")
    expect(H, "plane of 2^31 pixels", hyp(h=46341, w=46341, H=46341, W=46341, pad=0), b"32-bit pixel index")
    expect(H, "full resolution of 2^31 pixels", hyp(H=46341, W=46341), b"32-bit pixel index")
    # an empty gradient: success before any pointer is looked at, whatever else is NULL
    expect(H, "empty g_cur_depth (h0)", hyp(h0=0, g_out=None, scratch=None, g_cur_depth=None, cur_depth=None, near_far=None), want=0)
    expect(H, "empty g_cur_depth (w0)", hyp(w0=0, g_cur_depth=None), want=0)
    # ... but not before the size checks
    expect(H, "empty g_cur_depth, D = 1", hyp(h0=0, D=1), b"D = ")
    expect(H, "empty g_cur_depth, h > H", hyp(h0=0, h=33), b"must cover")
    expect(H, "NULL g_cur_depth", hyp(g_cur_depth=None), b"null g_cur_depth")
    expect(H, "NULL cur_depth", hyp(cur_depth=None), b"map mode only")
    expect(H, "row mode", hyp(row=PTR, D_in=48), b"map mode only")
    expect(H, "NULL near_far", hyp(near_far=None), b"near_far")
    expect(H, "NULL g_out", hyp(g_out=None), b"null g_out")
    expect(H, "NULL scratch", hyp(scratch=None), b"null g_out")
    expect(H, "no inner column under a border", hyp(h=0), b"empty map")
    # the scratch size: 2 h w + H W floats, < 0 on bad sizes
    sizes = hyp()
    out["calls"] += 3
    if lib.ucnerf_depth_hypotheses_bwd_scratch_floats(C.addressof(sizes.fwd)) != 2 * 16 * 20 + 32 * 40:
        out["problems"].append("scratch_floats of the standard sizes")
    if lib.ucnerf_depth_hypotheses_bwd_scratch_floats(C.addressof(hyp(D=1).fwd)) >= 0 or lib.ucnerf_depth_hypotheses_bwd_scratch_floats(None) >= 0:
        out["problems"].append("scratch_floats accepted bad sizes")

    R = "ucnerf_depth_regress_bwd_values"
    expect(R, "NULL params", None, b"null params")
    for field in ("D", "Hp", "Wp", "pad"):
        expect(R, "%s = -1" % field, reg(**{field: -1}), b"negative size")
    expect(R, "Hp < 2 pad", reg(Hp=3), b"border")
    expect(R, "Wp < 2 pad", reg(Wp=3), b"border")
    expect(R, "plane of 2^31 pixels", reg(Hp=46341, Wp=46341), b"32-bit pixel index")
    for name in ("prob_volume", "g_depth", "g_depth_values"):
        expect(R, "NULL " + name, reg(**{name: None}), b"null pointer")
    expect(R, "empty volume (D)", reg(D=0, prob_volume=None, g_depth=None, g_depth_values=None), want=0)
    expect(R, "empty volume (Hp)", reg(Hp=0, pad=0, g_depth_values=None), want=0)
    expect(R, "empty volume (Wp)", reg(Wp=0, pad=0, prob_volume=None), want=0)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
