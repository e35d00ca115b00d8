"""Child process of tests/test_cas_loss_host.py: ucnerf_cas_loss_fwd / _bwd / _workspace_floats called with every argument error include/ucnerf_hip.h
lists.  Each must return UCNERF_EINVAL (-1) with a message and never crash or launch (runs without a GPU: a call that passed validation would need
a device).  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1
PTR = 64            # stands for a device address: never dereferenced, validation comes first


def fwd(n_stages=3, sizes=(48, 192, 768), **kw):
    p = L.CasLossParams()
    p.n_stages, p.with_weight = n_stages, 1
    for s in range(3):
        p.n[s], p.stage_w[s] = sizes[s], (0.5, 1.0, 2.0)[s]
        p.est[s] = p.gt[s] = p.w[s] = p.wpair[s] = PTR
    p.workspace = p.total = p.stage_loss = p.count = p.status = PTR
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def bwd(n_stages=3, sizes=(48, 192, 768), **kw):
    p = L.CasLossBwdParams()
    p.n_stages = n_stages
    for s in range(3):
        p.n[s], p.stage_w[s] = sizes[s], (0.5, 1.0, 2.0)[s]
        p.est[s] = p.gt[s] = p.wpair[s] = p.g_est[s] = PTR
    p.count = p.g_total = PTR
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}

    def expect(fn, what, p, needle):
        out["calls"] += 1
        rc = getattr(lib, fn)(C.addressof(p) if p is not None else None, None)
        msg = lib.ucnerf_last_error() or b""
        if rc != EINVAL or not msg or needle not in msg:
            out["problems"].append("%s: %s returned %d (%r)" % (fn, what, rc, msg[:160]))

    for fn, make in (("ucnerf_cas_loss_fwd", fwd), ("ucnerf_cas_loss_bwd", bwd)):
        expect(fn, "NULL params", None, b"null params")
        for k in (0, 4, -1):
            expect(fn, "n_stages = %d" % k, make(n_stages=k), b"outside 1..3")
        for stages in (1, 2, 3):
            for bad in (0, -1, (1 << 30) + 1):
                expect(fn, "%d stages, last n = %d" % (stages, bad), make(n_stages=stages, n=(stages - 1, bad)), b"elements, outside")
        for field in ("est", "gt"):
            for s in range(3):
                expect(fn, "NULL %s[%d]" % (field, s), make(**{field: (s, None)}), b"null")
    for field in ("total", "stage_loss", "count", "workspace"):
        expect("ucnerf_cas_loss_fwd", "NULL " + field, fwd(**{field: None}), b"null")
    expect("ucnerf_cas_loss_fwd", "NULL w[1]", fwd(w=(1, None)), b"null w")
    expect("ucnerf_cas_loss_fwd", "wpair of one stage only missing", fwd(wpair=(2, None)), b"all or none")
    for field in ("count", "g_total"):
        expect("ucnerf_cas_loss_bwd", "NULL " + field, bwd(**{field: None}), b"null")
    for field in ("wpair", "g_est"):
        expect("ucnerf_cas_loss_bwd", "NULL %s[2]" % field, bwd(**{field: (2, None)}), b"null")
    # the workspace size: the sum of the stage sizes, or the same refusals
    sizes = (C.c_int32 * 3)(48, 192, 768)
    out["calls"] += 4
    if lib.ucnerf_cas_loss_workspace_floats(3, sizes) != 1008 or lib.ucnerf_cas_loss_workspace_floats(1, sizes) != 48:
        out["problems"].append("workspace_floats: wrong size")
    if lib.ucnerf_cas_loss_workspace_floats(3, None) >= 0 or lib.ucnerf_cas_loss_workspace_floats(4, sizes) >= 0:
        out["problems"].append("workspace_floats: accepted NULL sizes or four stages")
    sizes[1] = 0
    out["calls"] += 1
    if lib.ucnerf_cas_loss_workspace_floats(2, sizes) >= 0:
        out["problems"].append("workspace_floats: accepted an empty stage")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
