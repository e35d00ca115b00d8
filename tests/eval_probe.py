"""Child process of tests/test_eval_cases_host.py: ucnerf_depth_eval, ucnerf_image_eval and ucnerf_eval_workspace_floats called with every
argument error include/ucnerf_hip.h lists.  Each must return UCNERF_EINVAL (-1) with a message and never crash or launch (runs without a GPU: a
call that passed validation would need a device).  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def depth(**kw):
    p = L.DepthEvalParams()
    p.n, p.H, p.W, p.min_depth, p.max_depth = 3, 12, 16, 1e-4, 100.0
    p.gt = p.pred = p.workspace = p.out = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def image(**kw):
    p = L.ImageEvalParams()
    p.n, p.H, p.W = 2, 9, 11
    p.gt = p.pred = p.workspace = p.out = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(fn, what, p, needle=None):
        out["calls"] += 1
        rc = getattr(lib, fn)(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != EINVAL or not msg or (needle and needle not in msg):
            out["problems"].append("%s %s returned %d (%r)" % (fn, what, rc, msg[:160]))

    for fn, make in (("ucnerf_depth_eval", depth), ("ucnerf_image_eval", image)):
        expect(fn, "NULL params", None, b"null params")
        for field in ("n", "H", "W"):
            expect(fn, field + " = -1", make(**{field: -1}), b"negative or empty")
            expect(fn, field + " = 0", make(**{field: 0}), b"negative or empty")
        for field in ("gt", "pred", "workspace", "out"):
            expect(fn, "NULL " + field, make(**{field: None}), b"null gt, pred, workspace or out")
        expect(fn, "misaligned workspace", make(workspace=PTR + 4), b"8-byte aligned")
        expect(fn, "n above the grid limit", make(n=65536, H=7, W=7), b"65535")
    expect("ucnerf_depth_eval", "2^31 pixels", depth(n=2, H=32768, W=32768), b"32-bit")
    expect("ucnerf_depth_eval", "min above max", depth(min_depth=2.0, max_depth=1.0), b"above max_depth")
    expect("ucnerf_image_eval", "2^31 values", image(n=3, H=16384, W=16384), b"32-bit")
    for H, W in ((6, 9), (9, 6), (1, 1), (6, 6)):
        expect("ucnerf_image_eval", "%d x %d" % (H, W), image(H=H, W=W), b"7 x 7 SSIM window")
    for args in ((0, 12, 16), (3, 0, 16), (3, 12, 0), (-1, 12, 16), (3, -1, 16), (3, 12, -1), (3, 32768, 32768)):
        out["calls"] += 1
        rc = lib.ucnerf_eval_workspace_floats(*args)
        if rc != EINVAL or not lib.ucnerf_last_error():
            out["problems"].append("ucnerf_eval_workspace_floats%r returned %d" % (args, rc))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
