"""The fine pass reuses the coarse evaluations by default (CoarseFineRenderer.render(..., reuse_coarse=None)) and composites the new and the kept
rows where they are (ucnerf_composite_merged_fwd): every returned tensor equals the full evaluation's, bit for bit, on every route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# rays per batch.  1, 33, 777 and 1100: partial tiles, several blocks, and (1100 x 192) a fine pass past three rounds of tiles on a 256-CU part.
# A pass composites inside its MLP launch only when its whole-rays-per-block dealing fills nine tenths of the CUs -- on 256 CUs
# none of those four does -- so 500 is there for that route (two rays per block on 250 blocks; 500 x 57 and 500 x 4 leave partial tiles there);
# the tests read the library's own predicate and assert that both routes were seen.  Where the all-depths fine pass itself is of that size the
# default keeps it (one launch; ucnerf_reuse_coarse_pays) and the tests force the reuse there as well.
N_RAYS = (1, 33, 500, 777, 1100)
# (n_coarse, n_fine): merged 192 -> three samples per lane; 57 -> one, ragged last lane; (3, 1): the smallest pair the entry points take
# (ucnerf_composite_sample_pdf: S >= 3, n_bins = S - 1 >= 2; n_samples >= 1)
PAIRS = ((64, 128), (17, 40), (3, 1))


def _scene():
    from uc_nerf_amd.synthetic import make_scene, scene_to
    return scene_to(make_scene(seed=2, H=64, W=80, small_volumes=True), DEV)


def _networks():
    """The suite's usual network (small density heads) and one at density-head scale 1, the reference's own init."""
    from uc_nerf_amd.pipeline import flat_params_of
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    return [flat_params_of(init_ucnerf_state_dict(seed=2, sigma_scale=0.05, sigma_bias=0.05)).to(DEV),
            flat_params_of(init_ucnerf_state_dict(seed=2)).to(DEV)]


def _flat(out, prefix=""):
    res = {}
    for k, v in out.items():
        if isinstance(v, dict):
            res.update(_flat(v, prefix + k + "."))
        else:
            res[prefix + k] = v
    return res


def _assert_same(got, want, what):
    got, want = _flat(got), _flat(want)
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        assert torch.is_tensor(got[k]) and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k)


def _set_white(r, white):
    r.white_bkgd = white
    for p in (r.pass_, r.pass_small):
        if p is not None:
            p.set_white_bkgd(white)


def _inputs(n, nc, nf, perturb, seed):
    from uc_nerf_amd.synthetic import random_pixels
    xs, ys = random_pixels(n, 64, 80, seed=5 + seed)
    kw = {}
    if perturb:
        g = torch.Generator().manual_seed(seed)
        kw = dict(perturb=1.0, noise=torch.rand(n, nc, generator=g).to(DEV), u=torch.rand(n, nf, generator=g).to(DEV))
    return xs.to(DEV), ys.to(DEV), kw


@pytest.fixture
def operand(request):
    from uc_nerf_amd import ops
    before = ops.split_operand()
    ops.set_split_operand(request.param)
    yield request.param
    ops.set_split_operand(before)


CONFIGS = [("f32", "bf16"), ("bf16x3", "bf16"), ("bf16x3", "fp16"), ("bf16x3_fused", "bf16"), ("bf16x3_fused", "fp16")]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d+%d" % p)
@pytest.mark.parametrize("precision,operand", CONFIGS, indirect=["operand"])
def test_default_equals_full_evaluation_on_every_returned_tensor(precision, operand, pair):
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.pipeline import CoarseFineRenderer
    nc, nf = pair
    scene = _scene()
    tail_seen = set()
    for k, flat in enumerate(_networks()):
        r = CoarseFineRenderer(scene, flat, nc, nf, precision=precision)
        assert not r.pw.guarded
        for n in N_RAYS:
            fits = bool(L.lib().ucnerf_fused_tail_fits(n, nc + nf))
            tail_seen.add(fits)
            assert bool(L.lib().ucnerf_reuse_coarse_pays(n, nc, nf)) == (not fits)
            in_launch = fits and precision == "bf16x3_fused"      # (only the gather-fused kernel composites inside its launch)
            for fold in (True, False):
                r.fold_launches = fold
                for white in (False, True):
                    _set_white(r, white)
                    for perturb in (0, 1):
                        xs, ys, kw = _inputs(n, nc, nf, perturb, seed=n + k)
                        what = (k, n, fold, white, perturb)
                        full = r.render(xs, ys, reuse_coarse=False, **kw)
                        assert r.fine_route == "all_depths"
                        got = r.render(xs, ys, **kw)
                        if in_launch:                    # the all-depths pass is one launch there: the default keeps it (ucnerf_reuse_coarse_pays)
                            assert r.fine_route == "all_depths" and "tail route" in r.fine_route_reason, (what, r.fine_route_reason)
                            forced = r.render(xs, ys, reuse_coarse=True, **kw)      # the reuse behind a coarse pass that composited in its launch
                            assert r.fine_route == "new_depths"
                            _assert_same({k: v for k, v in _flat(forced).items() if k in _flat(full)}, full, what + ("forced",))
                        else:
                            assert r.fine_route == "new_depths", (what, r.fine_route_reason)
                        _assert_same(got, full, what)
                        assert got["weights"].shape == (n, nc + nf) and got["z_samples"].shape == (n, nf)
    # both sides of the boundary between the route that composites inside the MLP launch and the one with a compositing launch of its own
    if pair == (64, 128):
        assert tail_seen == {True, False}, tail_seen
        assert L.lib().ucnerf_fused_tail_fits_resample(500, nc, nf) == 1 and L.lib().ucnerf_fused_tail_fits(1100, nc + nf) == 0


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16x3_fused"])
def test_capture_replay_equals_eager(precision):
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.pipeline import CoarseFineRenderer
    scene, flat = _scene(), _networks()[0]
    r = CoarseFineRenderer(scene, flat, 64, 128, precision=precision)
    for n in (500, 1100):
        xs, ys, kw = _inputs(n, 64, 128, 1, seed=n)
        del kw["u"]                                      # (capture() draws with the renderer's deterministic u)
        g = r.capture(n, perturb=1.0)
        pays = bool(L.lib().ucnerf_reuse_coarse_pays(n, 64, 128)) or precision != "bf16x3_fused"
        assert r.fine_route == ("new_depths" if pays else "all_depths") and pays == (n != 500 or precision != "bf16x3_fused")
        got = g(xs, ys, kw["noise"])                     # (tensors of the graph's own pool: the eager renders below do not touch them)
        _assert_same(got, r.render(xs, ys, **kw), ("eager default", n))
        _assert_same(got, r.render(xs, ys, reuse_coarse=False, **kw), ("eager full", n))


@pytest.mark.parametrize("precision", ["f32", "bf16x3_fused"])
def test_ties_between_a_drawn_depth_and_a_coarse_depth(precision):
    """A network whose density is zero everywhere: all coarse weights are 0, the pdf is uniform, and draws placed at the right u land on a coarse
    depth bit for bit.  The merge rank is a permutation all the same and the render equals the full evaluation."""
    from uc_nerf_amd import ops
    from uc_nerf_amd.pipeline import CoarseFineRenderer, flat_params_of
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict, random_pixels
    nc, nf, n = 64, 128, 300
    sd = init_ucnerf_state_dict(seed=2)
    for name in ("nerf.alpha_linear", "nerf.alpha_linear_1"):
        sd[name + ".weight"].zero_()
        sd[name + ".bias"].zero_()
    r = CoarseFineRenderer(_scene(), flat_params_of(sd).to(DEV), nc, nf, precision=precision)
    xs, ys = (t.to(DEV) for t in random_pixels(n, 64, 80, seed=9))
    probe = r.render(xs, ys, reuse_coarse=False)
    assert torch.count_nonzero(probe["coarse"]["weights"]) == 0
    z_c = probe["z_coarse"]
    assert torch.equal(z_c, z_c[:1].expand_as(z_c))                                   # perturb 0: every ray has the same coarse depths
    # bin k of the mid-point bins spans coarse depth k + 1, near u = (k + 1/2) / (S - 2); the map u -> depth moves by about one float per float
    # of u there, so among the neighbouring floats of that u some give the coarse depth exactly: find them with the sampler itself
    c = ((np.arange(nc - 2) + 0.5) / (nc - 2)).astype(np.float32)
    for _ in range(32):
        c = np.nextafter(c, np.float32(0))
    hits = []
    for _ in range(4):                                                                 # 64 neighbouring floats per bin, 16 per call (n_samples <= 1024)
        cols = []
        for _ in range(16):
            cols.append(c.copy())
            c = np.nextafter(c, np.float32(1))
        cand = torch.from_numpy(np.stack(cols, 1).reshape(-1)).to(DEV)
        drawn = ops.sample_pdf(None, torch.zeros(1, nc, device=DEV), cand, z_merge=z_c[:1].contiguous(), from_coarse=True, want_inds=False)["samples"][0]
        hits.append(cand[(drawn[:, None] == z_c[0][None, :]).any(1)])
    hits = torch.cat(hits)
    assert hits.numel() >= 1, "no candidate draw lands on a coarse depth"
    # u: every second ray gets the tie draws (and two equal draws: a tie among the new depths), the rest seeded noise; sorted per ray or not
    g = torch.Generator().manual_seed(3)
    u = torch.rand(n, nf, generator=g).to(DEV)
    k = min(int(hits.numel()), nf - 2)
    u[::2, :k] = hits[:k]
    u[::2, k] = u[::2, k + 1]
    u[::4] = u[::4].sort(dim=1)[0]
    for fold in (True, False):
        r.fold_launches = fold
        full = r.render(xs, ys, u=u, reuse_coarse=False)
        tie = (full["z_samples"][:, :, None] == full["z_coarse"][:, None, :]).any(2).any(1)
        assert int(tie.sum()) >= 1 and bool(tie[::2].all())
        _assert_same(r.render(xs, ys, u=u), full, ("ties", fold))
        forced = r.render(xs, ys, u=u, reuse_coarse=True)
        rank = forced["coarse"]["merge_rank"] if fold else None
        if rank is not None:
            assert rank.dtype == torch.int32 and rank.shape == (n, nc + nf)
            assert torch.equal(rank.long().sort(dim=1)[0], torch.arange(nc + nf, device=DEV).expand(n, -1))
            # ... and it is the permutation of that sort
            cat = torch.cat([forced["z_samples"], forced["z_coarse"]], 1)
            assert torch.equal(torch.zeros_like(cat).scatter_(1, rank.long(), cat), forced["z_fine"])
        for key in ("rgb", "depth", "acc", "weights", "var"):
            assert torch.equal(forced[key], full[key]), key
    # the rank of the stand-alone re-sampling (the launch structure with fold_launches False), checked the same way
    hs = ops.sample_pdf(None, full["coarse"]["weights"], u, z_merge=z_c, want_inds=False, from_coarse=True, want_rank=True)
    assert torch.equal(hs["merge_rank"].long().sort(dim=1)[0], torch.arange(nc + nf, device=DEV).expand(n, -1))
    assert torch.equal(hs["z_sorted"], full["z_fine"])


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 192, 1024])
def test_composite_merged_fwd_equals_merge_rows_then_composite_fwd(S):
    from uc_nerf_amd import ops
    g = torch.Generator().manual_seed(S)
    for n in (1, 5):
        for na in sorted({0, 1, S - 1, S}):
            nb = S - na
            raw = torch.rand(n, S, 4, generator=g)
            raw[..., 3] *= 4.0 / S                                                    # (densities that leave transmittance along the whole ray)
            raw_a, raw_b = raw[:, :na].contiguous().to(DEV), raw[:, na:].contiguous().to(DEV)
            rank = torch.stack([torch.randperm(S, generator=g) for _ in range(n)]).int().to(DEV)
            z = (1.0 + 3.0 * torch.rand(n, S, generator=g)).sort(dim=1)[0].to(DEV)
            u = torch.rand(n, S, generator=g).to(DEV)
            for white in (False, True):
                for kw in (dict(), dict(want_var=False), dict(u=u)):
                    want = ops.composite_fwd(ops.merge_rows(raw_a, raw_b, rank), z, 0, white, **kw)
                    got = ops.composite_merged_fwd(raw_a, raw_b, rank, z, white, **kw)
                    _assert_same(got, want, (S, n, na, white, tuple(kw)))
                    assert ("var" in got) == (S >= 2 and kw.get("want_var", True)) and ("wu" in got) == ("u" in kw)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_fused"])
def test_guarded_mode_evaluates_all_depths(precision):
    from uc_nerf_amd import ops
    from uc_nerf_amd.pipeline import CoarseFineRenderer
    before = ops.split_operand()
    ops.set_split_operand("fp16_guarded")
    try:
        r = CoarseFineRenderer(_scene(), _networks()[1], 64, 128, precision=precision)
        assert r.pw.guarded
        for n in (33, 500):
            xs, ys, kw = _inputs(n, 64, 128, 1, seed=n)
            got = r.render(xs, ys, **kw)
            assert r.fine_route == "all_depths" and "fp16_guarded" in r.fine_route_reason
            _assert_same(got, r.render(xs, ys, reuse_coarse=False, **kw), ("guarded", n))
    finally:
        ops.set_split_operand(before)


def test_fused_min_rounds_on_different_kernels_evaluates_all_depths():
    """fused_min_rounds puts small passes on the two-kernel route: where the passes of one render do not all run on the same kernel, the default
    evaluates all depths (rows of different kernels are not bit-identical to each other)."""
    from uc_nerf_amd.pipeline import CoarseFineRenderer
    r = CoarseFineRenderer(_scene(), _networks()[0], 64, 128, precision="bf16x3_fused", fused_min_rounds=1)
    n = r.fused_min_samples // 128                     # coarse pass below the threshold, the other two at or above it
    assert n * 64 < r.fused_min_samples <= n * 128
    xs, ys, kw = _inputs(n, 64, 128, 0, seed=1)
    got = r.render(xs, ys)
    assert r.fine_route == "all_depths" and "fused_min_rounds" in r.fine_route_reason
    _assert_same(got, r.render(xs, ys, reuse_coarse=False), "mixed kernels")
    xs, ys, kw = _inputs(33, 64, 128, 0, seed=2)       # every pass below the threshold: one kernel again
    got = r.render(xs, ys)
    assert r.fine_route == "new_depths"
    _assert_same(got, r.render(xs, ys, reuse_coarse=False), "all small")
