"""CoarseFineRenderer.render_train: the hierarchical renderer with autograd history (gather + MLP at the coarse depths, ops.composite, re-sampling
without gradient, gather + MLP at the new depths only, ops.composite_merged), on the synthetic scene at its smallest size.

Expected gradients come from the CPU oracle's differentiable single pass (oracle/ucnerf_oracle.py through tests/fuzz_render.oracle_pass), run
once at the device's z_coarse and once at its z_fine -- sampling is bit-exact and carries no gradient -- with the two losses summed, and are
compared as tests/fuzz_grads.py compares the single-pass backward: its element-wise bar (`outside`), the oracle run on the device's side of
every relu (`Relus`), a bias held to its weight's scale, tensors the reference's autograd never reaches exactly zero, and a tensor excused only
where the float32 oracle itself misses the bar against float64."""
import functools

import pytest
import torch

import fuzz_grads as FG
from fuzz_render import oracle_pass

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 32, 40
SHAPES = [(37, 8, 16), (64, 64, 128)]


def _scene_cpu():
    from uc_nerf_amd.synthetic import make_scene
    return make_scene(seed=11, H=H, W=W, small_volumes=True)


def _sd():
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    return init_ucnerf_state_dict(seed=5, sigma_scale=0.1, sigma_bias=0.02)


def _inputs(n, nc, nf):
    from uc_nerf_amd.synthetic import random_pixels
    xs, ys = random_pixels(n, H, W, seed=n)
    g = torch.Generator().manual_seed(n)
    return dict(xs=xs.to(DEV), ys=ys.to(DEV), noise=torch.rand(n, nc, generator=g).to(DEV), u=torch.rand(n, nf, generator=g).to(DEV),
                target=torch.rand(n, 3, generator=g))


def _renderer(nc, nf, leaves=False, precision="f32"):
    from uc_nerf_amd.pipeline import CoarseFineRenderer, flat_params_of
    from uc_nerf_amd.synthetic import scene_to
    scene = scene_to(_scene_cpu(), DEV)
    if leaves:
        scene["vols"] = [v.requires_grad_(True) for v in scene["vols"]]
        scene["img_feat"].requires_grad_(True)
        scene["confidence"].requires_grad_(True)
    flat = flat_params_of(_sd()).to(DEV)
    return CoarseFineRenderer(scene, flat, nc, nf, precision=precision), flat


def _loss(c_rgb, f_rgb, f_depth, target, coarse=True):
    loss = ((f_rgb - target) ** 2).mean() + 0.1 * f_depth.mean()
    return loss + ((c_rgb - target) ** 2).mean() if coarse else loss


def _device_sides(r, flat, rays_d, z):
    """On which side of every relu the device's network was at the depths z ([n,S,units] bool, in the oracle's call order): the activation sets
    the training forward of the MLP keeps, and the sign of the density it returns (what fuzz_grads.DevicePass reads from a render pass)."""
    from uc_nerf_amd import ops
    n, S = z.shape
    pts, ndc = r._train_coords(rays_d, z)
    feats = ops.feat_gather_fwd(r.src, pts, ndc["stage1"], ndc["stage2"], ndc["stage3"])
    angle, _ = ops.dir_feature(rays_d, r.scene["w2cs"][0])
    raw, kept = ops.mlp_fwd_train(r.pw, r.pw.pack(flat.detach()), ndc["ndc"], angle, feats.view(n * S, -1), S)
    sides = [(kept["h%d" % k] > 0).view(n, S, 128).cpu() for k in range(6)]
    return sides + [(kept["vc"][:, :64] > 0).view(n, S, 64).cpu(), (kept["vc"][:, 64:] > 0).view(n, S, 64).cpu(), (raw.view(n, S, 4)[..., 3:4] > 0).cpu()]


def _oracle_grads(sd, sc, rays_d, z_c, z_f, target, sides_c, sides_f, dtype=torch.float32, coarse=True):
    """{tensor name: gradient} of the loss by autograd through two single passes of the oracle in `dtype`, on the given relu sides."""
    cv = lambda t: t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t              # noqa: E731
    p = {k: cv(v).clone().requires_grad_(True) for k, v in sd.items()}
    leaves = dict(vols=[cv(v).clone().requires_grad_(True) for v in sc["vols"]], img_feat=cv(sc["img_feat"]).clone().requires_grad_(True),
                  confidence=cv(sc["confidence"]).clone().requires_grad_(True))
    scene = {k: ([cv(x) for x in v] if isinstance(v, list) else cv(v)) for k, v in sc.items()}
    scene.update(leaves)
    with FG.Relus(sides_f):
        fine, _, _ = oracle_pass(p, scene, cv(rays_d), cv(z_f), False)
    c_rgb = None
    if coarse:
        with FG.Relus(sides_c):
            c_rgb = oracle_pass(p, scene, cv(rays_d), cv(z_c), False)[0]["rgb"]
    _loss(c_rgb, fine["rgb"], fine["depth"], cv(target), coarse).backward()
    out = {n_: (t.grad if t.grad is not None else torch.zeros_like(t)) for n_, t in zip(FG.NAMES5, leaves["vols"] + [leaves["img_feat"], leaves["confidence"]])}
    out.update({k: v.grad for k, v in p.items()})
    return out


def _merged_sides(sides_new, sides_coarse, rank):
    """Sides at the merged depths: row rank[j] of the merge is row j of cat(new, coarse)."""
    out = []
    for a, b in zip(sides_new, sides_coarse):
        cat = torch.cat([a, b], 1)
        out.append(torch.zeros_like(cat).scatter(1, rank.long()[..., None].expand(cat.shape), cat))
    return out


def _by_name(sd, g_flat, leaves):
    got = dict(zip(FG.NAMES5, leaves))
    o = 0
    for k, v in sd.items():
        got[k] = g_flat[o:o + v.numel()].view(v.shape)
        o += v.numel()
    return got


def _hold(got, want, want64_fn, what):
    """fuzz_grads.run's comparison with the sides given, for the exact-f32 route."""
    bad, w64 = [], None
    for k, w_ in want.items():
        if w_ is None:
            if torch.count_nonzero(got[k]):
                bad.append(k + ": gradient where the reference has none")
            continue
        wk = k[:-4] + "weight" if k.endswith(".bias") else None
        floor_ = float(want[wk].abs().max()) if wk is not None and want.get(wk) is not None else 0.0
        n_out, worst = FG.outside(got[k], w_, "f32", floor_)
        print("%s %s: %d of %d outside, worst %.3g of max|g|" % (what, k, n_out, w_.numel(), worst))
        if n_out:
            w64 = want64_fn() if w64 is None else w64
            w64k = w64[k].float()
            if FG.outside(w64k + FG.COARSER["f32"] * (w_ - w64k), w64k, "f32")[0]:
                continue                                  # a sum that cancels: the float32 oracle itself misses the bar against float64
            bad.append("%s: %d of %d outside the bar with the sides given, worst %.3g of max|g|" % (k, n_out, w_.numel(), worst))
    assert not bad, what + "\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("n,nc,nf", SHAPES)
def test_forward_is_the_inference_render_bit_for_bit(n, nc, nf):
    """Same kernels: the training route's gather (ucnerf_feat_gather_fwd on the channel-major sources), exact-f32 MLP, compositing, re-sampling
    and merged compositing are the launches render(reuse_coarse=True) makes on a renderer whose sources were not repacked channel-last
    (repack=False on a fresh renderer), so the depths AND every rendered value are required bit-identical -- no bar.  (After a repack the
    inference gather reads the channel-last copies: another kernel, whose features differ in the last bit; the training route never does.)"""
    r, flat = _renderer(nc, nf)
    i = _inputs(n, nc, nf)
    kw = dict(perturb=1.0, noise=i["noise"], u=i["u"])
    want = r.render(i["xs"], i["ys"], reuse_coarse=True, repack=False, **kw)
    assert not r.pass_.use_cl
    got = r.render_train(i["xs"], i["ys"], flat.clone().requires_grad_(True), **kw)
    assert set(got) == set(want) and set(got["coarse"]) == set(want["coarse"])
    for k in ("z_coarse", "z_samples", "z_fine", "rays_d", "rgb", "depth", "acc", "disp", "weights", "var"):
        assert torch.equal(got[k], want[k]), k
    for k in want["coarse"]:
        assert torch.equal(got["coarse"][k], want["coarse"][k]), "coarse." + k
    for k in ("rgb", "depth", "acc", "weights"):
        assert got[k].requires_grad and got[k].grad_fn is not None, k
    assert got["coarse"]["rgb"].requires_grad and got["coarse"]["raw"].requires_grad
    assert not got["z_fine"].requires_grad and not got["z_samples"].requires_grad and not got["disp"].requires_grad
    # without draws of its own: the deterministic ones of render()
    want = r.render(i["xs"], i["ys"], reuse_coarse=True, repack=False)
    got = r.render_train(i["xs"], i["ys"], flat)
    assert torch.equal(got["z_fine"], want["z_fine"]) and torch.equal(got["rgb"], want["rgb"]) and not got["rgb"].requires_grad


# ------------------------------------------------------------------------------------------------ gradients
@functools.lru_cache(maxsize=None)
def _trained(n, nc, nf, coarse):
    """One device step (loss through the coarse and the fine outputs, or the fine ones alone) and everything the checks read from it."""
    r, flat = _renderer(nc, nf, leaves=True)
    i = _inputs(n, nc, nf)
    flat = flat.requires_grad_(True)
    out = r.render_train(i["xs"], i["ys"], flat, perturb=1.0, noise=i["noise"], u=i["u"])
    out["coarse"]["raw"].retain_grad()
    _loss(out["coarse"]["rgb"], out["rgb"], out["depth"], i["target"].to(DEV), coarse).backward()
    sc = r.scene
    return r, flat, i, out, [t.grad for t in sc["vols"] + [sc["img_feat"], sc["confidence"]]]


@pytest.mark.parametrize("n,nc,nf", SHAPES)
def test_gradients_match_the_oracle_at_the_device_depths(n, nc, nf):
    r, flat, i, out, leaf_grads = _trained(n, nc, nf, True)
    sd, sc = _sd(), _scene_cpu()
    assert all(g is not None for g in leaf_grads) and flat.grad is not None
    rays_d, z_c, z_f, z_s = (out[k].detach() for k in ("rays_d", "z_coarse", "z_fine", "z_samples"))
    sides_c = _device_sides(r, flat, rays_d, z_c)
    sides_f = _merged_sides(_device_sides(r, flat, rays_d, z_s), sides_c, out["coarse"]["merge_rank"].cpu())
    args = (sd, sc, rays_d.cpu(), z_c.cpu(), z_f.cpu(), i["target"], sides_c, sides_f)
    want = _oracle_grads(*args)
    got = _by_name(sd, flat.grad, leaf_grads)
    _hold(got, want, lambda: _oracle_grads(*args, dtype=torch.float64), "%dx(%d+%d)" % (n, nc, nf))


@pytest.mark.parametrize("n,nc,nf", SHAPES)
def test_the_fine_loss_alone_reaches_the_coarse_rows(n, nc, nf):
    """No double counting and nothing lost: with the fine loss alone the kept coarse rows still receive gradient (g_raw_b), and the parameter
    gradient is that of the fine pass evaluated over all nc + nf depths without reuse -- same ops, same bar."""
    from uc_nerf_amd import ops
    r, flat, i, out, _ = _trained(n, nc, nf, False)
    g_raw_b = out["coarse"]["raw"].grad
    assert g_raw_b is not None and bool(torch.isfinite(g_raw_b).all()) and int(torch.count_nonzero(g_raw_b)) > g_raw_b.numel() // 2
    rays_d, z_f = out["rays_d"].detach(), out["z_fine"].detach()
    flat2 = flat.detach().clone().requires_grad_(True)
    angle, _ = ops.dir_feature(rays_d, r.scene["w2cs"][0])
    raw = r._eval_train(flat2, r.pw.pack(flat2.detach()), rays_d, angle, z_f)
    rgb, depth, _, _, _, _ = ops.composite(raw, z_f, False)
    _loss(None, rgb, depth, i["target"].to(DEV), False).backward()
    sd = _sd()
    got, want = _by_name(sd, flat.grad, [None] * 5), _by_name(sd, flat2.grad.cpu(), [None] * 5)
    bad = []
    for k in sd:
        wk = k[:-4] + "weight" if k.endswith(".bias") else None
        n_out, worst = FG.outside(got[k], want[k], "f32", float(want[wk].abs().max()) if wk else 0.0)
        print("%s: %d outside, worst %.3g of max|g|" % (k, n_out, worst))
        if n_out:
            bad.append("%s: %d of %d outside the bar, worst %.3g of max|g|" % (k, n_out, want[k].numel(), worst))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ refusals
def test_precisions_without_a_training_forward_are_refused():
    from uc_nerf_amd import ops
    i = _inputs(37, 8, 16)
    r, flat = _renderer(8, 16, precision="bf16")
    with pytest.raises(RuntimeError, match="no training forward"):
        r.render_train(i["xs"], i["ys"], flat)
    before = ops.split_operand()
    ops.set_split_operand("fp16_guarded")
    try:
        r, flat = _renderer(8, 16, precision="bf16x3")
        assert r.pw.guarded
        with pytest.raises(RuntimeError, match="fp16_guarded"):
            r.render_train(i["xs"], i["ys"], flat)
    finally:
        ops.set_split_operand(before)
