"""Child process of tests/test_image_cases_host.py: ucnerf_image_put, ucnerf_depth_minmax, ucnerf_depth_colormap, ucnerf_minmax_reset and
ucnerf_minmax_read called with every argument error include/ucnerf_hip.h lists.  Each must return UCNERF_EINVAL (-1) with a message and never
crash or launch; a count of zero succeeds without a launch (runs without a GPU: a call that passed validation with a positive count would need
a device).  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def put(**kw):
    p = L.ImagePutParams()
    p.n, p.first_pixel, p.pixels = 4, 31, 35
    p.rgb = p.depth = p.rgb_chw = p.depth_hw = p.minmax = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def minmax(**kw):
    p = L.DepthMinmaxParams()
    p.count = 35
    p.depth = p.minmax = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def colormap(**kw):
    p = L.DepthColormapParams()
    p.count = 35
    p.depth = p.minmax = p.table = p.index = p.color = PTR
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
        if rc != want or (want != 0 and (not msg or (needle and needle not in msg))):
            out["problems"].append("%s %s returned %d (%r)" % (fn, what, rc, msg[:160]))

    for fn in ("ucnerf_image_put", "ucnerf_depth_minmax", "ucnerf_depth_colormap"):
        expect(fn, "NULL params", None, b"null params")
    # image_put: negative sizes, overruns (by one, far, at the int32 edge), NULL arrays, a misaligned array; an empty chunk is fine anywhere inside
    for field in ("n", "first_pixel", "pixels"):
        expect("ucnerf_image_put", field + " = -1", put(**{field: -1}), b"negative")
    expect("ucnerf_image_put", "overrun by one", put(n=5), b"overrun")
    expect("ucnerf_image_put", "first pixel past the end", put(n=1, first_pixel=35), b"overrun")
    expect("ucnerf_image_put", "int32 edge", put(n=2 ** 31 - 1, first_pixel=2 ** 31 - 1, pixels=2 ** 31 - 1), b"overrun")
    for field in ("rgb", "depth", "rgb_chw", "depth_hw"):
        expect("ucnerf_image_put", "NULL " + field, put(**{field: None}), b"null rgb, depth, rgb_chw or depth_hw")
    expect("ucnerf_image_put", "misaligned depth", put(depth=PTR + 2), b"4-byte aligned")
    expect("ucnerf_image_put", "empty chunk", put(n=0), want=0)
    expect("ucnerf_image_put", "empty chunk at the end", put(n=0, first_pixel=35), want=0)
    expect("ucnerf_image_put", "empty chunk, NULL arrays", put(n=0, rgb=None, depth=None, rgb_chw=None, depth_hw=None, minmax=None), want=0)
    expect("ucnerf_image_put", "empty chunk past the end", put(n=0, first_pixel=36), b"overrun")
    # depth_minmax
    expect("ucnerf_depth_minmax", "count = -1", minmax(count=-1), b"negative count")
    expect("ucnerf_depth_minmax", "count = 0", minmax(count=0, depth=None, minmax=None), want=0)
    for field in ("depth", "minmax"):
        expect("ucnerf_depth_minmax", "NULL " + field, minmax(**{field: None}), b"null depth or cell")
    expect("ucnerf_depth_minmax", "misaligned cell", minmax(minmax=PTR + 1), b"4-byte aligned")
    # depth_colormap
    expect("ucnerf_depth_colormap", "count = -1", colormap(count=-1), b"negative count")
    expect("ucnerf_depth_colormap", "count = 0", colormap(count=0, depth=None, table=None, index=None, color=None, minmax=None), want=0)
    expect("ucnerf_depth_colormap", "NULL depth", colormap(depth=None), b"null depth")
    expect("ucnerf_depth_colormap", "nothing to write", colormap(index=None, color=None), b"nothing to write")
    expect("ucnerf_depth_colormap", "colour without a table", colormap(table=None), b"256 x 3 table")
    expect("ucnerf_depth_colormap", "misaligned color", colormap(color=PTR + 2), b"4-byte aligned")
    # the cell's own entry points
    for fn, args in (("ucnerf_minmax_reset", (None, None)), ("ucnerf_minmax_reset", (PTR + 2, None)), ("ucnerf_minmax_read", (None, PTR, None)),
                     ("ucnerf_minmax_read", (PTR, None, None)), ("ucnerf_minmax_read", (PTR, PTR + 1, None))):
        out["calls"] += 1
        rc = getattr(lib, fn)(*args)
        if rc != EINVAL or not lib.ucnerf_last_error():
            out["problems"].append("%s%r returned %d" % (fn, args, rc))
    out["group_pixels"] = int(lib.ucnerf_image_group_pixels())
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
