"""Child process of tests/test_composite_merged_bwd_host.py: ucnerf_composite_merged_bwd called with every argument error include/ucnerf_hip.h
lists.  Each must return UCNERF_EINVAL (-1) with a message and never crash or launch (runs without a GPU: a call that passed validation would
need a device); an empty batch must return 0 the same way.  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def params(**kw):
    p = L.CompositeMergedBwdParams()
    p.n, p.na, p.nb = 4, 128, 64
    p.raw_a = p.raw_b = p.rank = p.z = p.g_raw_a = p.g_raw_b = PTR
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(what, p, needle=None, want=EINVAL):
        out["calls"] += 1
        rc = lib.ucnerf_composite_merged_bwd(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != want or (want == EINVAL and (not msg or b"composite_merged_bwd" not in msg or (needle and needle not in msg))):
            out["problems"].append("%s returned %d (%r)" % (what, rc, msg[:160]))

    expect("NULL params", None, b"null params")
    expect("n = -1", params(n=-1), b"negative count")
    expect("empty batch", params(n=0), want=0)
    expect("empty batch, nothing else set", L.CompositeMergedBwdParams(), want=0)
    for field in ("raw_a", "raw_b", "rank", "z", "g_raw_a", "g_raw_b"):
        expect("NULL " + field, params(**{field: None}), b"null pointer")
    expect("na = -1", params(na=-1), b"negative row count")
    expect("nb = -1", params(nb=-1), b"negative row count")
    expect("na + nb = 0", params(na=0, nb=0), b"outside 1..1024")
    expect("na + nb = 1025", params(na=1024, nb=1), b"outside 1..1024")
    expect("na + nb = 1025 (b)", params(na=1, nb=1024), b"outside 1..1024")
    expect("na + nb overflows int32", params(na=2 ** 31 - 1, nb=2 ** 31 - 1), b"outside 1..1024")
    for field in ("raw_a", "raw_b", "g_raw_a", "g_raw_b"):
        for off in (4, 8, 12):
            expect("%s misaligned by %d" % (field, off), params(**{field: PTR + off}), b"16-byte aligned")
    expect("rank misaligned", params(rank=PTR + 2), b"4-byte aligned")
    # a side without rows may leave its pointers NULL: these pass the pointer check and stop at a later one
    expect("na = 0, raw_a / g_raw_a NULL pass the pointer check", params(na=0, nb=64, raw_a=None, g_raw_a=None, rank=PTR + 2), b"4-byte aligned")
    expect("nb = 0, raw_b / g_raw_b NULL pass the pointer check", params(na=64, nb=0, raw_b=None, g_raw_b=None, rank=PTR + 2), b"4-byte aligned")
    # ... and only that side: the other's are still required
    expect("na = 0, g_raw_b NULL", params(na=0, nb=64, raw_a=None, g_raw_a=None, g_raw_b=None), b"null pointer")
    # the upstream gradients are optional, each of them: all four NULL is valid up to the launch (not probed: it would need a device)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
