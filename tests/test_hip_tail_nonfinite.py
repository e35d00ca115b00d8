"""The ray tail of the renderer on non-finite data (cases and CPU references: tests/tail_nonfinite_cases.py): compositing, inverse-CDF
re-sampling, the sorted merge and the merged compositing put NaN, +inf and -inf where torch puts them, leave nothing unwritten and let nothing
leak from a poisoned ray into its neighbours.

  ucnerf_sample_pdf            cdf, inds, samples against the reference's lines run by torch on the CPU; z_sorted against torch.sort (NaN last);
                               merge_rank a permutation that places the concatenation into z_sorted; both forms, with and without z_merge
  sample_pdf_ray's three homes the stand-alone launch, ucnerf_composite_sample_pdf and the tail of the gather-fused MLP launch: same bits
  ucnerf_composite_fwd / _bwd  both variants against the float64 oracle; ucnerf_composite_fold_grads against its float64 restatement
  ucnerf_composite_merged_*    fed the merge_rank of a poisoned re-sampling: merge_rows + the dense launches, bit for bit
  CoarseFineRenderer           one poisoned ray in a default render
  every launch                 a second call into the same, dirtied buffers gives the same bits"""
import pytest
import torch

import composite_cases as CC
import composite_maps_cases as MC
import tail_nonfinite_cases as TN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PDF_NAMES, COMP_NAMES = TN.pdf_names(), TN.comp_names()


def dev(t):
    return None if t is None else t.to(DEV)


def same(got, want, what):
    assert TN.same_bits(got, want), "%s: %s" % (what, TN.first_difference(got, want) if got.shape == want.shape else "shapes differ")


def run_pdf(case, which="poisoned", merge=True, **kw):
    from uc_nerf_amd import ops
    src = case if which == "poisoned" else case["clean"]
    if case["from_coarse"]:
        return ops.sample_pdf(None, dev(src["w"]), dev(src["u"]), z_merge=dev(src["z"]), from_coarse=True, **kw)
    return ops.sample_pdf(dev(src["z"]), dev(src["w"]), dev(src["u"]), z_merge=dev(src["zm"]) if merge else None, **kw)


# ------------------------------------------------------------------------------------------------ 1. ucnerf_sample_pdf
@pytest.mark.parametrize("name", PDF_NAMES)
def test_inds_cdf_and_samples_are_torchs_for_any_input(name):
    case, ref = TN.pdf_case(name), TN.pdf_reference(name)
    out = run_pdf(case, want_cdf=True, want_rank=True)
    same(out["cdf"], ref["cdf"], name + " cdf")
    assert torch.equal(out["inds"].cpu(), ref["inds"]), name + " inds: " + TN.first_difference(out["inds"].float(), ref["inds"].float())
    same(out["samples"], ref["samples"], name + " samples")
    if not case["from_coarse"]:                                              # the same call without a second list: nothing but the merge changes
        alone = run_pdf(case, merge=False, want_cdf=True)
        assert "z_sorted" not in alone
        for k in ("cdf", "inds", "samples"):
            same(alone[k], out[k], name + " without z_merge: " + k)


@pytest.mark.parametrize("name", PDF_NAMES)
def test_merge_rank_is_a_permutation_and_z_sorted_is_torch_sort_with_nan_last(name):
    case, ref = TN.pdf_case(name), TN.pdf_reference(name)
    out = run_pdf(case, want_rank=True)
    rank = out["merge_rank"].cpu()
    assert TN.is_permutation(rank), "%s: merge_rank is not a permutation on rays %s" % (
        name, [r for r in range(case["n"]) if not TN.is_permutation(rank[r:r + 1])])
    same(out["z_sorted"], ref["z_sorted"], name + " z_sorted")
    same(TN.placed(ref["cat"], rank), out["z_sorted"].cpu(), name + " cat scattered by merge_rank against z_sorted")
    if not case["from_coarse"]:                                              # no second list: the samples alone, sorted
        from uc_nerf_amd import ops
        empty = torch.empty(case["n"], 0, device=DEV)
        alone = ops.sample_pdf(dev(case["z"]), dev(case["w"]), dev(case["u"]), z_merge=empty, want_rank=True)
        assert TN.is_permutation(alone["merge_rank"]), name + ": merge_rank of the samples alone"
        same(alone["z_sorted"], torch.sort(ref["samples"], -1)[0], name + " samples alone, sorted")


@pytest.mark.parametrize("name", PDF_NAMES)
def test_resampling_keeps_a_poisoned_ray_to_itself(name):
    case = TN.pdf_case(name)
    keep = ~case["poisoned"]
    got, clean = run_pdf(case, want_cdf=True, want_rank=True), run_pdf(case, "clean", want_cdf=True, want_rank=True)
    for k in ("cdf", "inds", "samples", "z_sorted", "merge_rank"):
        same(got[k].cpu()[keep], clean[k].cpu()[keep], "%s %s of the clean rays" % (name, k))


# ------------------------------------------------------------------------------------------------ 3. compositing
def run_comp(case, white, src=None):
    from uc_nerf_amd import ops
    src = case if src is None else src
    if case["variant"] == 0:
        return ops.composite_fwd(dev(src["raw"]), dev(src["z"]), 0, white, u=dev(case["u"]))
    return ops.composite_fwd(dev(src["raw"]), dev(src["z"]), 1, white, rays_d=dev(src["rays_d"]), noise=dev(src["noise"]), u=dev(case["u"]))


def _grads(case):
    return {t: dev(case[t]) for t in CC.TARGETS}


@pytest.mark.parametrize("name", COMP_NAMES)
def test_compositing_puts_non_finite_values_where_the_float64_oracle_does(name):
    from uc_nerf_amd import ops
    case = TN.comp_case(name)
    keep, fails = ~case["poisoned"], []
    for white in (False, True):
        out = {k: v.cpu() for k, v in run_comp(case, white).items()}
        fails += TN.comp_fwd_failures(out, name, white, "forward")
        clean = run_comp(case, white, TN.clean_of(case))
        for k in out:
            same(out[k][keep], clean[k].cpu()[keep], "%s %s of the clean rays, white=%s" % (name, k, white))
        if case["variant"] == 0:
            g = ops.composite_bwd(dev(case["raw"]), dev(case["z"]), white_bkgd=white, **_grads(case)).cpu()
            fails += TN.comp_bwd_failures(g, name, white, "backward")
            g_clean = ops.composite_bwd(dev(case["clean"]["raw"]), dev(case["clean"]["z"]), white_bkgd=white, **_grads(case)).cpu()
            same(g[keep], g_clean[keep], "%s g_raw of the clean rays, white=%s" % (name, white))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", [n for n in COMP_NAMES if n.startswith("live") and "S3_" not in n or n == "live_S3_sigma"])
def test_gradient_fold_on_poisoned_maps(name):
    """composite_fold_grads with g_var, g_disp and g_wu on the forward outputs of a poisoned batch (the float32 oracle's, so that device and
    reference fold the same numbers) against the fold restated in float64.  Bar per output: 4 x the distance of the same restatement run in
    float32, the margin of composite_cases.bars()."""
    from uc_nerf_amd import ops
    case = TN.comp_case(name)
    n, S = case["n"], case["S"]
    f32 = TN.comp_reference(name, False)[1]
    gen = torch.Generator().manual_seed(S)
    ups = dict(g_var=torch.randn(n, generator=gen), g_disp=torch.randn(n, generator=gen), g_wu=torch.randn(n, generator=gen),
               g_depth=case["g_depth"], g_acc=case["g_acc"], g_weights=case["g_weights"])
    args = (f32["weights"], f32["depth"], f32["acc"], case["u"])
    ref = MC.fold64(*(a.double() for a in args), **{k: v.double() for k, v in ups.items()})
    own = MC.fold64(*args, **ups)
    got = ops.composite_fold_grads(*(dev(a) for a in args), **{k: dev(v) for k, v in ups.items()})
    fails = []
    for what, g, r, o in zip(("g_depth'", "g_acc'", "g_weights'", "g_u"), got, ref, own):
        assert torch.equal(TN.classes(o), TN.classes(r)), what                # (the restatement agrees with itself across the two precisions)
        fin = TN.classes(r) == 0
        bar = 4.0 * (o.double()[fin] - r[fin]).abs().max().item()
        assert bar > 0
        fails += TN.held(g, r, bar, "%s fold %s" % (name, what))
    assert not fails, "\n".join(fails)
    buf = tuple(torch.full_like(g, 7.0) for g in got)
    for _ in range(2):                                                       # written, not accumulated; stale values of another call in between
        ops.composite_fold_grads(*(dev(a) for a in args), out=buf, **{k: dev(v) for k, v in ups.items()})
        for g, b in zip(got, buf):
            same(b, g.cpu(), name + " fold into the caller's buffers")
            b.add_(1.0)


# ------------------------------------------------------------------------------------------------ 4. merged compositing with poisoned ranks
@pytest.mark.parametrize("name", [n for n in PDF_NAMES if n.startswith("coarse") and n.rsplit("_", 1)[1] in ("weights", "draws", "depths")])
def test_merged_compositing_follows_the_rank_of_a_poisoned_resampling(name):
    """The fine pass as the renderer's default route runs it: raw_a the rows of the M new depths, raw_b the rows of the S coarse ones, rank the
    merge_rank of the poisoned re-sampling.  Forward: merge_rows + composite_fwd, bit for bit; backward: composite_bwd of the merged rows taken
    back through the rank."""
    from uc_nerf_amd import ops
    case = TN.pdf_case(name)
    n, S, M = case["n"], case["S"], case["M"]
    out = run_pdf(case, want_rank=True)
    rank, z = out["merge_rank"], out["z_sorted"]
    assert TN.is_permutation(rank)
    gen = torch.Generator().manual_seed(S * 100 + M)
    raw_a = torch.cat([3.0 * torch.rand(n, M, 3, generator=gen) - 1.0, 0.25 + 1.5 * torch.rand(n, M, 1, generator=gen)], -1)
    raw_b = torch.cat([3.0 * torch.rand(n, S, 3, generator=gen) - 1.0, 0.25 + 1.5 * torch.rand(n, S, 1, generator=gen)], -1)
    raw_a[0, M // 2, 3] = TN.NAN                                             # ... and a row of the new evaluations that is itself poisoned
    u = torch.rand(n, S + M, generator=gen)
    g = dict(g_rgb=torch.randn(n, 3, generator=gen), g_depth=torch.randn(n, generator=gen), g_acc=torch.randn(n, generator=gen),
             g_weights=torch.randn(n, S + M, generator=gen))
    raw_a, raw_b, u, g = dev(raw_a), dev(raw_b), dev(u), {k: dev(v) for k, v in g.items()}
    merged = ops.merge_rows(raw_a, raw_b, rank)
    want_rows = torch.zeros(n, S + M, 4).scatter_(1, rank.cpu().long()[..., None].expand(n, S + M, 4), torch.cat([raw_a, raw_b], 1).cpu())
    same(merged, want_rows, name + " merge_rows")
    for white in (False, True):
        dense = ops.composite_fwd(merged, z, 0, white, u=u)
        one = ops.composite_merged_fwd(raw_a, raw_b, rank, z, white, u=u)
        assert set(one) == set(dense)
        for k in dense:
            same(one[k], dense[k], "%s merged forward %s white=%s" % (name, k, white))
        g_dense = ops.composite_bwd(merged, z, white_bkgd=white, **g).cpu()
        back = torch.gather(g_dense, 1, rank.cpu().long()[..., None].expand(n, S + M, 4))      # row j of cat(a, b) sits on merged position rank[j]
        bufs = (torch.full((n, M, 4), 7.0, device=DEV), torch.full((n, S, 4), 7.0, device=DEV))
        for _ in range(2):
            g_a, g_b = ops.composite_merged_bwd(raw_a, raw_b, rank, z, white_bkgd=white, out=bufs, **g)
            same(g_a, back[:, :M], "%s merged backward g_raw_a white=%s" % (name, white))
            same(g_b, back[:, M:], "%s merged backward g_raw_b white=%s" % (name, white))
            for b in bufs:
                b.add_(1.0)


# ------------------------------------------------------------------------------------------------ 6. nothing kept between calls
@pytest.mark.parametrize("name", ("bins_L130_M65_weights", "coarse_S132_M65_draws", "coarse_S66_M7_depths", "bins_L9_M7_shared"))
def test_second_resampling_into_the_same_dirty_buffers_gives_the_same_bits(name):
    from uc_nerf_amd import _lib as L, ops
    case = TN.pdf_case(name)
    n, Lb, M, nm = case["n"], case["L"], case["M"], case["n_merge"]
    w, z, u, zm = dev(case["w"]), dev(case["z"]), dev(case["u"]), dev(case["zm"])
    out = dict(samples=torch.full((n, M), 7.0, device=DEV), inds=torch.full((n, M), 7, dtype=torch.int64, device=DEV), cdf=torch.full((n, Lb), 7.0, device=DEV),
               z_sorted=torch.full((n, M + nm), 7.0, device=DEV), merge_rank=torch.full((n, M + nm), 7, dtype=torch.int32, device=DEV))
    p = L.SamplePdfParams()
    p.n, p.n_bins, p.n_samples, p.from_coarse, p.n_merge, p.u_stride = n, Lb, M, int(case["from_coarse"]), nm, 0 if case["shared"] else M
    p.bins, p.weights, p.u, p.z_merge = (None if case["from_coarse"] else z.data_ptr()), w.data_ptr(), u.data_ptr(), zm.data_ptr()
    p.samples, p.inds, p.cdf, p.z_sorted, p.merge_rank = (out[k].data_ptr() for k in ("samples", "inds", "cdf", "z_sorted", "merge_rank"))
    fresh = run_pdf(case, want_cdf=True, want_rank=True)
    for i in range(2):
        ops._launch("ucnerf_sample_pdf", p, w.device)
        for k, v in out.items():
            same(v, fresh[k].cpu(), "%s %s, call %d into the caller's buffers" % (name, k, i))
            v.add_(1)                                                        # (stale values of another call in every output, slots of NaN included)


@pytest.mark.parametrize("name", ("live_S257_sigma", "helpers_S65_geometry"))
def test_second_compositing_into_the_same_dirty_buffers_gives_the_same_bits(name):
    from uc_nerf_amd import _lib as L, ops
    case = TN.comp_case(name)
    n, S = case["n"], case["S"]
    raw, z, u = dev(case["raw"]), dev(case["z"]), dev(case["u"])
    rays_d, noise = dev(case.get("rays_d")), dev(case.get("noise"))
    shapes = dict(rgb=(n, 3), depth=(n,), acc=(n,), disp=(n,), weights=(n, S), wu=(n,))
    if case["variant"] == 0:
        shapes["var"] = (n,)
    out = {k: torch.full(s, 7.0, device=DEV) for k, s in shapes.items()}
    p = L.CompositeParams()
    p.n, p.S, p.variant, p.white_bkgd, p.raw, p.z, p.u = n, S, case["variant"], 1, raw.data_ptr(), z.data_ptr(), u.data_ptr()
    p.rgb_map, p.depth_map, p.acc_map, p.disp_map = (out[k].data_ptr() for k in ("rgb", "depth", "acc", "disp"))
    p.weights, p.wu = out["weights"].data_ptr(), out["wu"].data_ptr()
    if case["variant"] == 0:
        p.var = out["var"].data_ptr()
    else:
        p.rays_d, p.noise = rays_d.data_ptr(), noise.data_ptr()
    fresh = run_comp(case, True)
    for i in range(2):
        ops._launch("ucnerf_composite_fwd", p, raw.device)
        for k, v in out.items():
            same(v, fresh[k].cpu(), "%s %s, call %d into the caller's buffers" % (name, k, i))
            v.add_(1.0)
    if case["variant"] == 0:
        g = _grads(case)
        bp = L.CompositeBwdParams()
        bp.fwd.n, bp.fwd.S, bp.fwd.variant, bp.fwd.white_bkgd, bp.fwd.raw, bp.fwd.z = n, S, 0, 1, raw.data_ptr(), z.data_ptr()
        bp.g_rgb, bp.g_depth, bp.g_acc, bp.g_weights = (g[t].data_ptr() for t in CC.TARGETS)
        g_raw = torch.full((n, S, 4), 7.0, device=DEV)
        bp.g_raw = g_raw.data_ptr()
        want = ops.composite_bwd(raw, z, white_bkgd=True, **g).cpu()
        for i in range(2):
            ops._launch("ucnerf_composite_bwd", bp, raw.device)
            same(g_raw, want, "%s g_raw, call %d" % (name, i))
            g_raw.add_(1.0)


# ------------------------------------------------------------------------------------------------ 2. the three homes of sample_pdf_ray
def test_the_three_homes_of_the_resampling_give_the_same_bits_on_poisoned_rays():
    """One RenderPass call over 768 rays of 32 depths, re-sampled to 64: with the tail route (the gather-fused MLP launch composites and re-samples
    its own rays, sample_pdf_ray<.., WAVE_ONLY>), without it (ucnerf_composite_sample_pdf) and from the stand-alone ucnerf_sample_pdf fed the
    weights of the pass.  The poison is a NaN in a ray's own depths z[r, k]: the sample's point o + z d is NaN, and the MLP kernel hands a
    sample whose point is not finite four NaN outputs (csrc/mlp_bf16.hip: through the uncertainty blend u -- its ReLUs, fmaxf(x, 0), would
    swallow the NaN of the encoding), as the reference's network does.  A row of the MLP's input reaches its own output row only, so the NaN
    stays in its ray: the weights from k on (asserted below), the depth map, the mid-point bins k - 1 and k, the samples and the second list
    of the merge.  Rays 5, 300 and 767 carry it at the first, an inner and the last depth."""
    from uc_nerf_amd import _lib as L, ops
    from uc_nerf_amd.pipeline import flat_params_of
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict, make_scene, random_pixels, scene_to
    n, S, M = 768, 32, 64
    scene = scene_to(make_scene(seed=0), torch.device(DEV))
    sd = init_ucnerf_state_dict(seed=0, n_src=6, sigma_scale=0.05, sigma_bias=0.05)
    src = ops.GatherSources(scene["vols"], scene["confidence"], scene["imgs"], scene["img_feat"], scene["w2cs"][1:], scene["intrinsics"][1:])
    pw = ops.PackedWeights.get(6, 0, torch.device(DEV), "bf16x3_fused")
    rp = ops.RenderPass(src, pw, pw.pack(dev(flat_params_of(sd))), dev(scene["c2w"][:3, 3]), scene["w2cs"][0], scene["intrinsics"][0], scene["w2cs"][0],
                        scene["near"], scene["far"], False)
    rp.repack_sources()
    xs, ys = random_pixels(n, 256, 320, seed=5)
    rays_d, _, _ = ops.ray_gen(scene["K"].cpu(), scene["c2w"].cpu(), xs=dev(xs), ys=dev(ys))
    z_clean, _ = ops.sample_stratified(None, S, n=n, near=float(scene["near"]), far=float(scene["far"]), device=torch.device(DEV), perturb=1.0,
                                       noise=dev(torch.rand(n, S, generator=torch.Generator().manual_seed(S))))
    z = z_clean.clone()
    poison = {5: 0, 300: 11, 767: S - 1}
    for r, k in poison.items():
        z[r, k] = TN.NAN
    ang, _ = ops.dir_feature(rays_d, scene["w2cs"][0])
    count = L.lib().ucnerf_fused_tail_launches
    assert L.lib().ucnerf_fused_tail_fits(n, S) == 1
    keep = torch.ones(n, dtype=torch.bool)
    keep[list(poison)] = False
    try:
        for u in (torch.linspace(0., 1., M, device=DEV), dev(torch.rand(n, M, generator=torch.Generator().manual_seed(M)))):
            outs = {}
            for tail, zz in ((False, z), (True, z), (True, z_clean)):
                L.lib().ucnerf_set_fused_tail(int(tail))
                c0 = count()
                o = rp(rays_d, zz, want=("acc", "weights", "var"), dir_feat=ang, resample={"u": u, "want_rank": True})
                assert count() - c0 == int(tail)
                outs[tail, zz is z] = {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}
            fused, tail, clean = outs[False, True], outs[True, True], outs[True, False]
            for r, k in poison.items():
                w = fused["weights"][r].cpu()
                assert bool(torch.isnan(w[k:]).all()) and bool(torch.isfinite(w[:k]).all()) and bool(torch.isnan(fused["depth"][r])), (r, k)
                assert int(torch.isnan(fused["z_sorted"][r]).sum()) >= 1 and bool(torch.isnan(fused["z_sorted"][r, -1])), (r, k)
            alone = ops.sample_pdf(None, fused["weights"], u, z_merge=z, from_coarse=True, want_inds=False, want_rank=True)
            for k in ("samples", "z_sorted", "merge_rank"):
                same(fused[k], alone[k].cpu(), "compositing fused with re-sampling against the stand-alone launch: " + k)
            for k in fused:
                same(tail[k], fused[k].cpu(), "tail of the fused MLP launch against the separate launches: " + k)
                same(tail[k].cpu()[keep], clean[k].cpu()[keep], "clean rays of the poisoned batch against the clean batch: " + k)
            assert TN.is_permutation(tail["merge_rank"])
            ref = torch.sort(torch.cat([tail["samples"].cpu(), z.cpu()], -1), -1)[0]
            same(tail["z_sorted"], ref, "z_sorted of the tail route against torch.sort")
    finally:
        L.lib().ucnerf_set_fused_tail(1)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_one_poisoned_ray_in_a_default_render_stays_alone():
    _render_with_one_poisoned_ray()


def _render_with_one_poisoned_ray():
    """CoarseFineRenderer at its defaults (bf16x3_fused, the fine pass reusing the coarse evaluations) on the 32 x 40 synthetic scene, 64 rays,
    16 + 16 samples; ray 17's stratification noise is NaN at one sample, so one of its coarse depths is.  Memory safety, by reading: a NaN or
    infinite coordinate becomes an index only through geometry_device.h axis(), whose unnorm clamps it (fmaxf(NaN, 0) = 0); the search of
    sample_pdf_ray ends in [0, L] and its two reads are clamped; the counting merge's ranks are sums of at most tot_n - 1 ones; MergedRows and
    MergedGradRows clamp the inverse rank they read, and the inversion drops ranks outside the row."""
    from uc_nerf_amd.pipeline import CoarseFineRenderer, flat_params_of
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict, make_scene, random_pixels, scene_to
    n, bad = 64, 17
    scene = scene_to(make_scene(seed=3, H=32, W=40, small_volumes=True), torch.device(DEV))
    sd = init_ucnerf_state_dict(seed=3, sigma_scale=0.05, sigma_bias=0.05)
    xs, ys = random_pixels(n, 32, 40, seed=4)
    r = CoarseFineRenderer(scene, flat_params_of(sd).to(DEV), 16, 16, precision="bf16x3_fused")
    noise = torch.rand(n, 16, generator=torch.Generator().manual_seed(1))
    poisoned = noise.clone()
    poisoned[bad, 6] = TN.NAN
    keep = torch.arange(n) != bad
    for reuse in (None, True):                                               # what the renderer chooses at this size, and the reuse forced
        outs = []
        for nz in (noise, poisoned):
            o = r.render(dev(xs), dev(ys), perturb=1.0, noise=dev(nz), reuse_coarse=reuse)
            torch.cuda.synchronize()
            outs.append({k: v.cpu().clone() for k, v in o.items() if torch.is_tensor(v)})
        _one_ray_alone(outs[0], outs[1], keep, bad)
    return outs[1]


def test_the_poisoned_ray_of_a_default_render_is_nan_in_every_map():
    """The rest of what the issue sets for the render above: the poisoned ray's rgb, depth and acc are NaN, as the reference's are (torch's relu
    keeps a NaN, so a NaN point makes every output of its sample NaN).  It failed before the MLP kernel gave such a sample NaN outputs (depth
    NaN, but rgb = (0.2697, 0.1910, 0.2019) and acc = 0.5007): every ReLU there is fmaxf(x, 0), which returns the 0 for a NaN, so the density
    was never NaN and the poisoned ray's weights stayed finite.  Now the sample's uncertainty blend carries the NaN to its four outputs."""
    got = _render_with_one_poisoned_ray()
    bad = 17
    print("poisoned ray: rgb %s depth %s acc %s" % (got["rgb"][bad].tolist(), got["depth"][bad].item(), got["acc"][bad].item()))
    assert bool(torch.isnan(got["rgb"][bad]).all()) and bool(torch.isnan(got["depth"][bad])) and bool(torch.isnan(got["acc"][bad]))


def _one_ray_alone(clean, got, keep, bad):
    assert bool(torch.isfinite(clean["rgb"]).all())
    for k in ("rgb", "depth", "acc", "z_coarse", "z_samples", "z_fine", "weights"):
        same(got[k][keep], clean[k][keep], k + " of the other rays")
    assert bool(torch.isnan(got["z_coarse"][bad]).any())
    assert bool(torch.isnan(got["rgb"][bad]).all()) and bool(torch.isnan(got["depth"][bad])) and bool(torch.isnan(got["acc"][bad]))
    same(got["z_fine"][bad], torch.sort(torch.cat([got["z_samples"][bad], got["z_coarse"][bad]]))[0], "z_fine of the poisoned ray")
