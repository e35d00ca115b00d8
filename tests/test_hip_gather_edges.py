"""The feature gather on every route against the float64 oracle (tests/gather_cases.py): bit for bit on the lattice cases -- samples on gx = +-1,
on texels, past every border, on / behind the camera plane, volume dimensions of 1, runs of equal cells at every position of a wave -- and under
a bar derived from the float32 oracle's own error on the continuous cases.

Forward:  feat_gather_fwd_kernel (ops.feat_gather_fwd: row-major, tiled, u_out, masked units; an un-repacked RenderPass),
          feat_gather_cl_kernel<TILED, GIVEN, S16> (RenderPass after repack_sources / with in-place sources / cl_bf16; coords given or derived;
          features kept row-major (keep=("feats",)) or tiled (keep=("raw", "feats"))),
          the gather inside the split-MLP kernel ("bf16x3_fused" held to "bf16x3" on the same scenes).
Backward: ucnerf_feat_gather_bwd on its routes (ops.feat_gather_bwd(route=)): direct, scratch + transposed add, g_cl for all four sources,
          g_cl for the volumes / the image features alone (mixed with scratch); each with every `need` flag off in turn, each called twice."""
import pytest
import torch

import gather_cases as G
from test_hip_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ("direct", "scratch", "cl", "cl_vols", "cl_img_feat")
ALL_LATTICE = G.LATTICE_NAMES + G.DERIVED_NAMES


def f32(t):
    return t.float().to(DEV)


def coords_of(case):
    return {k: f32(case[k]).contiguous() for k in ("pts", "stage1", "stage2", "stage3")}


def sources(case, layout="planar", cl_bf16=False, vols=True, conf=True, imgs=True):
    """GatherSources of a case.  layout: "planar" (reference layouts), "inplace3" / "inplace4" (every source channel-last in its own allocation,
    colours 3 / 4 values per pixel), "inplace_vols" (the volumes alone)."""
    from uc_nerf_amd import ops
    v, im, ft = [f32(t) for t in case["vols"]], f32(case["imgs"]), f32(case["img_feat"])
    if layout != "planar":
        c = ops.ChannelLastSources.from_reference_layout(v, im, ft)
        v = c.vols
        if layout != "inplace_vols":
            ft = c.img_feat
            if layout == "inplace3":
                im = c.imgs
            else:
                buf = torch.zeros(case["V"], case["H"], case["W"], 4, device=DEV)
                buf[..., :3] = im[0].permute(0, 2, 3, 1)
                im = buf[..., :3].permute(0, 3, 1, 2)
    src = ops.GatherSources(v if vols else None, f32(case["confidence"]) if conf else None, im if imgs else None, ft if imgs else None,
                            case["w2cs"].float(), case["intrinsics"].float(), cl_bf16=cl_bf16)
    if layout == "inplace3":
        assert src.zero_copy and src.rgb_stride == 3
    if layout == "inplace4":
        assert src.zero_copy and src.rgb_stride == 4
    if layout == "inplace_vols":
        assert src.inplace == [True, True, True, False, False]
    return src


_FLAT = {}


def render_pass(case, src, precision="f32"):
    from uc_nerf_amd import ops
    from uc_nerf_amd.pipeline import flat_params_of
    V = case["V"]
    if V not in _FLAT:
        _FLAT[V] = flat_params_of(G.lattice_state_dict(V)).to(DEV)
    pw = ops.PackedWeights.get(V, 0, torch.device(DEV), precision)
    if "rays_d" in case:
        return ops.RenderPass(src, pw, pw.pack(_FLAT[V]), f32(case["rays_o"]), case["w2c_ref"].float(), case["K_ref"].float(), case["w2c_ref"].float(),
                              case["near"], case["far"])
    return ops.RenderPass(src, pw, pw.pack(_FLAT[V]))


def run_pass(case, rp, given, keep=("feats",)):
    """One forward of the pass: coordinates handed over (given) or derived from the case's rays and depths."""
    from uc_nerf_amd import ops
    if given:
        co = coords_of(case)
        n, S = co["pts"].shape[:2]
        co["ndc"] = co["stage3"]
        rays_d, z = torch.tensor([[0.0, 0.0, 1.0]], device=DEV).repeat(n, 1), torch.ones(n, S, device=DEV)
        if "rays_d" in case:
            rays_d, z = f32(case["rays_d"]), f32(case["z"])
        out = rp(rays_d, z, keep=keep, coords=co)
    else:
        n, S = case["z"].shape
        out = rp(f32(case["rays_d"]), f32(case["z"]), near_far=f32(case["near_far"]) if "near_far" in case else None, keep=keep)
    if "feats" in keep:
        F = rp.src.F
        out["feats_rows"] = (ops.untile_feats(out["feats"], n * S, F) if out.get("feats_tiled") else out["feats"]).reshape(n * S, F)
    return out


def same(got, want, what):
    got, want = got.cpu(), want.float().reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, reference %r"
                             % (what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


# ------------------------------------------------------------------------------------------------ forward, lattice
@pytest.mark.parametrize("name", ALL_LATTICE)
def test_planar_forward_is_exact(name):
    """feat_gather_fwd_kernel, both output layouts, u_out, and each unit group masked out alone."""
    from uc_nerf_amd import ops
    case, ref, _ = G.lattice(name)
    m, V = case["m"], case["V"]
    F = 24 + 12 * V + 1
    ref = ref.reshape(m, F)
    co = coords_of(case)
    args = (co["pts"], co["stage1"], co["stage2"], co["stage3"])
    src = sources(case)
    same(ops.feat_gather_fwd(src, *args).reshape(m, F), ref, name + " row-major")
    u = torch.full((m,), 7.0, device=DEV)
    tiled = ops.feat_gather_fwd(src, *args, tiled=True, u_out=u)
    same(ops.untile_feats(tiled, m, F), ref, name + " tiled")
    same(u, 1.0 - ref[:, -1], name + " u_out")
    cols = G.columns(V)
    for tiled_out in (False, True):
        def rows(s, t):
            return ops.untile_feats(t, m, s.F) if tiled_out else t.reshape(m, s.F)
        want = ref.clone(); want[:, :24] = 0
        s = sources(case, vols=False)
        same(rows(s, ops.feat_gather_fwd(s, co["pts"], None, None, co["stage3"], tiled=tiled_out)), want, name + " vols=None")
        want = ref.clone(); want[:, -1] = 0
        s = sources(case, conf=False)
        same(rows(s, ops.feat_gather_fwd(s, *args, tiled=tiled_out)), want, name + " conf=None")
        s = sources(case, imgs=False)                                   # (one masked view: F = 37 whatever the case's V)
        want = torch.zeros(m, s.F, dtype=ref.dtype); want[:, :24] = ref[:, :24]; want[:, -1] = ref[:, -1]
        same(rows(s, ops.feat_gather_fwd(s, None, co["stage1"], co["stage2"], co["stage3"], tiled=tiled_out)), want, name + " imgs=None")
    assert cols["confidence"] == [F - 1]


@pytest.mark.parametrize("name", ALL_LATTICE)
def test_pass_forward_with_given_coordinates_is_exact(name):
    """The gather of a render pass, coordinates handed over: the planar kernel (sources not repacked), then feat_gather_cl_kernel<*, GIVEN = true, *>
    from repacked copies, from in-place sources (colours 3 and 4 values per pixel, volumes alone in place) and from bf16 copies; features kept
    row-major (TILED = false) and in the tile layout (TILED = true)."""
    case, ref, _ = G.lattice(name)
    ref = ref.reshape(case["m"], -1)
    rp = render_pass(case, sources(case))
    same(run_pass(case, rp, True)["feats_rows"], ref, name + " planar kernel in the pass")
    for layout, bf16, repack in (("planar", False, True), ("inplace3", False, False), ("inplace4", False, False), ("inplace_vols", False, True),
                                 ("planar", True, True)):
        rp = render_pass(case, sources(case, layout, cl_bf16=bf16))
        if repack:
            rp.repack_sources()
        assert rp.use_cl
        for keep in (("feats",), ("raw", "feats")):
            out = run_pass(case, rp, True, keep)
            assert bool(out.get("feats_tiled")) == (len(keep) == 2)
            same(out["feats_rows"], ref, "%s %s bf16=%s keep=%s" % (name, layout, bf16, keep))


@pytest.mark.parametrize("name", G.DERIVED_NAMES)
def test_pass_forward_with_derived_coordinates_is_exact(name):
    """coords=None: the pass derives points and stage coordinates from (ray, depth) -- idx / S through ExactDiv, the reference camera's projection,
    scene or per-ray near / far: the planar route (render_points + feat_gather_fwd_kernel) and feat_gather_cl_kernel<*, GIVEN = false, *>."""
    case, ref, _ = G.lattice(name)
    ref = ref.reshape(case["m"], -1)
    rp = render_pass(case, sources(case))
    same(run_pass(case, rp, False)["feats_rows"], ref, name + " planar route")
    for layout, bf16, repack in (("planar", False, True), ("inplace3", False, False), ("inplace4", False, False), ("planar", True, True)):
        rp = render_pass(case, sources(case, layout, cl_bf16=bf16))
        if repack:
            rp.repack_sources()
        for keep in (("feats",), ("raw", "feats")):
            out = run_pass(case, rp, False, keep)
            assert bool(out.get("feats_tiled")) == (len(keep) == 2)
            same(out["feats_rows"], ref, "%s %s bf16=%s keep=%s" % (name, layout, bf16, keep))


# ------------------------------------------------------------------------------------------------ backward, lattice
def ref_grads(case, grads):
    V, H, W = case["V"], case["H"], case["W"]
    shapes = [(8,) + tuple(s) for s in case["dhw"]] + [(H, W), (V, 8, H, W)]
    return [grads[k].reshape(s) for k, s in zip(G.GRADS, shapes)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ALL_LATTICE)
def test_backward_route_is_exact(name, route):
    """All five gradients on one route; then with each `need` flag off in turn (the others unchanged, the one left out None); then a second call
    into the same arrays: exactly twice the first."""
    from uc_nerf_amd import ops
    case, _, grads = G.lattice(name)
    want = ref_grads(case, grads)
    co = coords_of(case)
    args = (co["pts"], co["stage1"], co["stage2"], co["stage3"], f32(case["g_feats"]).reshape(case["m"], -1))
    src = sources(case)
    got = ops.feat_gather_bwd(src, *args, route=route)
    for k, g, w in zip(G.GRADS, got, want):
        same(g, w, "%s %s %s" % (name, route, k))
    ops._feat_gather_bwd_into(src, *args, got, route)
    for k, g, w in zip(G.GRADS, got, want):
        same(g, 2 * w, "%s %s %s after a second call" % (name, route, k))
    for off in range(5):
        need = tuple(i != off for i in range(5))
        part = ops.feat_gather_bwd(src, *args, need=need, route=route)
        assert part[off] is None
        for i, (k, g, w) in enumerate(zip(G.GRADS, part, want)):
            if i != off:
                same(g, w, "%s %s %s with need[%d] off" % (name, route, k, off))


@pytest.mark.parametrize("name", ("sweep_v2_m257", "runs_v2", "small_m9_v8"))
def test_backward_serves_in_place_sources_on_the_cl_route(name):
    from uc_nerf_amd import ops
    case, _, grads = G.lattice(name)
    co = coords_of(case)
    args = (co["pts"], co["stage1"], co["stage2"], co["stage3"], f32(case["g_feats"]).reshape(case["m"], -1))
    src = sources(case, "inplace3")
    with pytest.raises(RuntimeError, match="channel-last"):
        ops.feat_gather_bwd(src, *args)
    got = ops.feat_gather_bwd(src, *args, route="cl")
    for k, g, w, s in zip(G.GRADS, got, ref_grads(case, grads), src.vols + [src.conf, src.img_feat]):
        same(g, w, "%s in place %s" % (name, k))
        assert all(n == 1 or a == b for n, a, b in zip(g.shape, g.stride(), s.stride())), k      # the gradient comes back with the source's strides


# ------------------------------------------------------------------------------------------------ continuous cases
def _held(name, route, dist, oracle_d, scale, report):
    """Every group's distance under its bar; the figures are printed and recorded before anything is asserted."""
    rows = {k: dict(device=v, oracle_f32=oracle_d[k], bar=G.bar(oracle_d[k], scale[k])) for k, v in dist.items() if k != "mask_flips"}
    report["%s/%s" % (name, route)] = rows
    fails = ["%s %s %s: %.3e > bar %.3e (float32 oracle %.3e)" % (name, route, k, r["device"], r["bar"], r["oracle_f32"])
             for k, r in rows.items() if not r["device"] <= r["bar"]]
    if dist.get("mask_flips"):
        fails.append("%s %s: %d in-mask bits differ outside the excluded set" % (name, route, dist["mask_flips"]))
    return fails


@pytest.mark.parametrize("name", G.CONTINUOUS_NAMES)
def test_continuous_case_within_four_times_the_float32_oracle(name):
    from uc_nerf_amd import ops
    case, ref, grads, oracle_d, scale = G.continuous(name)
    m = case["m"]
    co = coords_of(case)
    args = (co["pts"], co["stage1"], co["stage2"], co["stage3"])
    report, fails = {}, []
    fwd = {}
    src = sources(case)
    fwd["planar_rows"] = ops.feat_gather_fwd(src, *args).reshape(m, -1)
    fwd["planar_tiled"] = ops.untile_feats(ops.feat_gather_fwd(src, *args, tiled=True), m, src.F)
    for layout, repack in (("planar", True), ("inplace3", False), ("inplace4", False)):
        rp = render_pass(case, sources(case, layout))
        if repack:
            rp.repack_sources()
        fwd["cl_%s_rows" % layout] = run_pass(case, rp, True)["feats_rows"]
        fwd["cl_%s_tiled" % layout] = run_pass(case, rp, True, ("raw", "feats"))["feats_rows"]
    for route, feats in fwd.items():
        fails += _held(name, route, G.distances(case, ref, grads, feats.cpu(), {}), oracle_d, scale, report)
    g_feats = f32(case["g_feats"]).reshape(m, -1)
    want = dict(zip(G.GRADS, ref_grads(case, grads)))
    for route in ROUTES:
        got = dict(zip(G.GRADS, [g.cpu() for g in ops.feat_gather_bwd(src, *args, g_feats, route=route)]))
        d = G.distances(case, ref, want, ref.float(), got)
        fails += _held(name, "bwd_" + route, {k: d[k] for k in G.GRADS}, oracle_d, scale, report)
    # bf16 copies: the reference is the float64 oracle on sources rounded to bf16
    case_b, ref_b, grads_b, oracle_b, scale_b = G.continuous(name, True)
    rp = render_pass(case, sources(case, cl_bf16=True))
    rp.repack_sources()
    for keep in (("feats",), ("raw", "feats")):
        feats = run_pass(case, rp, True, keep)["feats_rows"]
        fails += _held(name, "cl_bf16_" + ("tiled" if len(keep) == 2 else "rows"), G.distances(case_b, ref_b, grads_b, feats.cpu(), {}), oracle_b,
                       scale_b, report)
    record("gather_edges/" + name, excluded_share=case["excluded_share"], **report)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the gather inside the split-MLP kernel
@pytest.mark.parametrize("name", ALL_LATTICE)
def test_gather_fused_kernel_sees_the_same_features(name):
    """"bf16x3_fused" keeps no features: its render of the lattice scenes is held to the two-kernel "bf16x3" pass with the same weights (the bars of
    test_gather_fused_pass_matches_oracle_and_the_two_kernel_pass; the weights: gather_cases.lattice_state_dict).  The two-kernel pass's features are exact (tests above), edge samples included,
    so a difference beyond the bars is the third copy of the gather disagreeing."""
    case, _, _ = G.lattice(name)
    src = sources(case)
    passes = {}
    for prec in ("bf16x3", "bf16x3_fused"):
        passes[prec] = render_pass(case, src, prec)
        passes[prec].repack_sources()
    for given in ((True, False) if "rays_d" in case else (True,)):
        two = run_pass(case, passes["bf16x3"], given, ("raw",))
        one = run_pass(case, passes["bf16x3_fused"], given, ("raw",))
        scale = max(1.0, two["raw"][..., 3].abs().max().item())
        what = "%s given=%s" % (name, given)
        assert torch.isfinite(one["raw"]).all() and torch.isfinite(two["raw"]).all(), what
        torch.testing.assert_close(one["raw"], two["raw"], atol=2e-5 * scale, rtol=1e-5, msg=lambda s: what + " raw: " + s)
        torch.testing.assert_close(one["rgb"], two["rgb"], atol=1e-5, rtol=0, msg=lambda s: what + " rgb: " + s)
        torch.testing.assert_close(one["depth"], two["depth"], atol=2e-5, rtol=0, msg=lambda s: what + " depth: " + s)
