"""Child process of tests/test_split_guard_host.py: the entry points of the guarded fp16 split called with a NULL status / condition word, NULL params,
a misaligned word, the wrong operand, a precision outside the split ones and negative counts.  Each must return UCNERF_EINVAL (-1) with a message and
never crash or launch (runs without a GPU: a call that passed validation would need a device).  Prints one JSON line."""
import ctypes as C
import json
import sys

from uc_nerf_amd import _lib as L

EINVAL = -1


def main():
    lib = L.lib()
    out = {"calls": 0, "problems": []}
    word = (C.c_uint32 * 4)()                      # host memory: never dereferenced, validation comes first
    wp = C.addressof(word)

    def expect(what, rc, needle=None):
        out["calls"] += 1
        msg = lib.ucnerf_last_error() or b""
        if rc != EINVAL or not msg or (needle and needle not in msg):
            out["problems"].append("%s returned %d (%r)" % (what, rc, msg[:120]))

    def mlp(operand=1, precision=1, m=64):
        p = L.MlpParams()
        p.cfg = L.MlpConfig(6, 0, precision, operand)
        p.m, p.S = m, 1
        p.pts = p.dirs = p.feats = p.wstream = p.raw = 64
        return p

    def render(operand=1, precision=3, n=4):
        r = L.RenderParams()
        r.n, r.S, r.cfg = n, 64, L.MlpConfig(6, 0, precision, operand)
        r.rays_o = r.rays_d = r.z = r.workspace = r.wstream = r.rgb_map = r.depth_map = 64
        return r

    for name, mk in (("ucnerf_mlp_fwd", mlp), ("ucnerf_render_fused_fwd", render)):
        g, f = getattr(lib, name + "_guarded"), getattr(lib, name + "_if")
        p = mk()
        expect(name + "_guarded(NULL status)", g(C.addressof(p), None, None), b"null pointer")
        expect(name + "_if(NULL run_if)", f(C.addressof(p), None, None), b"null pointer")
        expect(name + "_guarded(NULL params)", g(None, wp, None), b"null pointer")
        expect(name + "_if(NULL params)", f(None, wp, None), b"null pointer")
        expect(name + "_guarded(misaligned word)", g(C.addressof(p), wp + 2, None), b"aligned")
        expect(name + "_if(misaligned word)", f(C.addressof(p), wp + 2, None), b"aligned")
        p = mk(operand=0)
        expect(name + "_guarded(operand 0)", g(C.addressof(p), wp, None), b"operand")
        p = mk(precision=0)
        expect(name + "_guarded(precision 0)", g(C.addressof(p), wp, None), b"precision")
        expect(name + "_if(precision 0)", f(C.addressof(p), wp, None), b"precision")
    p = mlp(m=-1)
    expect("ucnerf_mlp_fwd_guarded(m = -1)", lib.ucnerf_mlp_fwd_guarded(C.addressof(p), wp, None), b"negative count")
    expect("ucnerf_mlp_fwd_if(m = -1)", lib.ucnerf_mlp_fwd_if(C.addressof(p), wp, None), b"negative count")
    r = render(n=-1)
    expect("ucnerf_render_fused_fwd_guarded(n = -1)", lib.ucnerf_render_fused_fwd_guarded(C.addressof(r), wp, None), b"negative count")
    expect("ucnerf_render_fused_fwd_if(n = -1)", lib.ucnerf_render_fused_fwd_if(C.addressof(r), wp, None), b"negative count")

    cfg, cfg0, cfg_f32 = L.MlpConfig(6, 0, 1, 1), L.MlpConfig(6, 0, 1, 0), L.MlpConfig(6, 0, 0, 1)
    a = C.addressof
    expect("ucnerf_mlp_pack_guarded(NULL status)", lib.ucnerf_mlp_pack_guarded(a(cfg), 64, 64, 64, None, None), b"null pointer")
    expect("ucnerf_mlp_pack_if(NULL run_if)", lib.ucnerf_mlp_pack_if(a(cfg0), 64, 64, 64, None, None), b"null pointer")
    expect("ucnerf_mlp_pack_guarded(NULL cfg)", lib.ucnerf_mlp_pack_guarded(None, 64, 64, 64, wp, None), b"null pointer")
    expect("ucnerf_mlp_pack_guarded(operand 0)", lib.ucnerf_mlp_pack_guarded(a(cfg0), 64, 64, 64, wp, None), b"operand")
    expect("ucnerf_mlp_pack_guarded(precision 0)", lib.ucnerf_mlp_pack_guarded(a(cfg_f32), 64, 64, 64, wp, None), b"precision")
    expect("ucnerf_mlp_pack_guarded(NULL flat)", lib.ucnerf_mlp_pack_guarded(a(cfg), None, 64, 64, wp, None), b"null pointer")
    expect("ucnerf_mlp_pack_if(NULL flat)", lib.ucnerf_mlp_pack_if(a(cfg0), None, 64, 64, wp, None), b"null pointer")
    ptrs, numel = (C.c_void_p * 1)(64), (C.c_int64 * 1)(8)
    expect("ucnerf_mlp_pack_tensors_guarded(NULL status)", lib.ucnerf_mlp_pack_tensors_guarded(a(cfg), 1, ptrs, numel, 64, 64, None, None), b"null pointer")
    expect("ucnerf_mlp_pack_tensors_if(NULL run_if)", lib.ucnerf_mlp_pack_tensors_if(a(cfg0), 1, ptrs, numel, 64, 64, None, None), b"null pointer")
    expect("ucnerf_mlp_pack_tensors_guarded(operand 0)", lib.ucnerf_mlp_pack_tensors_guarded(a(cfg0), 1, ptrs, numel, 64, 64, wp, None), b"operand")
    expect("ucnerf_mlp_pack_tensors_guarded(-1 tensors)", lib.ucnerf_mlp_pack_tensors_guarded(a(cfg), -1, ptrs, numel, 64, 64, wp, None), b"tensors")
    expect("ucnerf_mlp_pack_tensors_if(-1 tensors)", lib.ucnerf_mlp_pack_tensors_if(a(cfg0), -1, ptrs, numel, 64, 64, wp, None), b"tensors")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
