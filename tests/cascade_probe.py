"""Child process of tests/test_cascade_host.py: ucnerf_depth_hypotheses called with every argument error include/ucnerf_hip.h lists.  Each must
return UCNERF_EINVAL (-1) with a message and never crash or launch (runs without a GPU: a call that passed validation would need a device); an
output of zero elements must return 0 the same way.  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def params(mode="map", **kw):
    p = L.DepthHypothesesParams()
    p.D, p.h, p.w, p.pad, p.H, p.W, p.h0, p.w0, p.D_in, p.k = 8, 16, 20, 1, 32, 40, 8, 10, 0, 1.0 / 48
    p.near_far = p.out = PTR
    if mode == "map":
        p.cur_depth = PTR
    else:
        p.row, p.D_in = PTR, 48
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(what, p, needle=None, want=EINVAL):
        out["calls"] += 1
        rc = lib.ucnerf_depth_hypotheses(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != want or (want == EINVAL and (not msg or (needle and needle not in msg))):
            out["problems"].append("%s returned %d (%r)" % (what, rc, msg[:160]))

    expect("NULL params", None, b"null params")
    for mode in ("map", "row"):
        expect(mode + ": NULL output", params(mode, out=None), b"null output")
        for field in ("D", "h", "w", "pad", "H", "W", "h0", "w0", "D_in"):
            expect("%s: %s = -1" % (mode, field), params(mode, **{field: -1}), b"negative size")
        for D in (0, 1):
            expect("%s: D = %d" % (mode, D), params(mode, D=D), b"D = ")
        # an output of zero elements: success, nothing launched (there is no device here to launch on)
        expect(mode + ": empty output", params(mode, h=0, pad=0), want=0)
        expect(mode + ": empty output (w)", params(mode, w=0, pad=0), want=0)
    expect("both inputs NULL", params("map", cur_depth=None), b"exactly one")
    expect("both inputs given", params("map", row=PTR, D_in=48), b"exactly one")
    expect("h > H", params(h=33), b"must cover")
    expect("w > W", params(w=41), b"must cover")
    expect("h0 > H", params(h0=33), b"must cover")
    expect("w0 > W", params(w0=41), b"must cover")
    expect("map: NULL near_far", params(near_far=None), b"near_far")
    expect("map: empty depth map", params(h0=0), b"empty map")
    expect("row: empty row", params("row", D_in=0), b"empty hypothesis row")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
