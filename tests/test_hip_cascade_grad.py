"""The gradient chain depth regression -> depth_values -> depth hypotheses -> previous depth on the GPU: ucnerf_depth_hypotheses_bwd and
ucnerf_depth_regress_bwd_values against CPU autograd through the restated op chain (tests/cascade_stubs.py, pinned to fixture G19 by
tests/test_cascade_host.py) and through oracle.mvs_oracle.depth_regress, in float64; the cases and the proofs that they are what they claim are
in tests/cascade_grad_cases.py / tests/test_cascade_grad_host.py.

  lattice cases      torch.equal, and a second launch bit-identical
  continuous cases   |device - float64| <= 4 x (float32 CPU autograd's max distance from float64 on that case) + 1e-6 x max|reference|, every element
                     (the bar of profiles/mvs_edges.md; the margin of 4 covers a different but equally valid summation order)
  end to end         CascadeMVSNet(grad_method="undetach") on G19's inputs: the stage-1 and stage-2 logits' gradients of sum(stage-3 depth) against
                     the restated cascade in float64, same bar recipe

Run on the GPU box:  python -m pytest tests/test_hip_cascade_grad.py -m gpu -q -s   (prints the measured distances; profiles/cascade_grad.md)
"""
import pytest
import torch
import torch.nn.functional as F

import cascade_grad_cases as G
import cascade_stubs as S
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ops():
    from uc_nerf_amd import ops as _ops
    return _ops


def dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def device_grad(c):
    """The direct kernel call on a case of cascade_grad_cases."""
    nf = torch.tensor([c["near"], c["far"]], device=DEV)
    interval = None if c["interval"] is None else torch.tensor([c["interval"]], device=DEV)
    sizes = (c["D"], c["hw"][0], c["hw"][1], c["pad"], c["HW"][0], c["HW"][1], c["k"])
    return ops().depth_hypotheses_bwd(dev(c["g_out"]), dev(c["cur"]), nf, interval, sizes)


@pytest.mark.parametrize("name", list(G.LATTICE))
def test_hypotheses_backward_is_exact_on_the_lattice(name):
    c = G.lattice_case(name)
    got = device_grad(c)
    again = device_grad(c)
    torch.cuda.synchronize()
    assert got.shape == c["want"].shape and got.dtype == torch.float32
    wrong = int((got.cpu().double() != c["want"]).sum())
    print("\n%s: %d of %d elements differ; census %s" % (name, wrong, got.numel(), c["census"]))
    assert torch.equal(got.cpu().double(), c["want"])
    assert torch.equal(got, again)                        # repeatability: two launches are bit-identical


@pytest.mark.parametrize("name", list(G.CONTINUOUS))
def test_hypotheses_backward_against_float64_autograd(name):
    c = G.continuous_case(name)
    got = device_grad(c)
    again = device_grad(c)
    torch.cuda.synchronize()
    err = (got.cpu().double() - c["want"]).abs().max().item()
    print("\n%s: device distance %.3e / bar %.3e = %.3f; float32 witness %.3e; excluded share %.2e; max|reference| %.3f"
          % (name, err, c["bar"], err / c["bar"], c["witness"], c["excluded_share"], c["want"].abs().max().item()))
    assert err <= c["bar"]
    assert torch.equal(got, again)


@pytest.mark.parametrize("name", list(G.REGRESS))
def test_regression_values_gradient_is_exact(name):
    c = G.regress_case(name)
    got = ops()._depth_regress_bwd_values(dev(c["prob"]), dev(c["g_depth"]), c["pad"])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c["want"].float())      # one product per element, correctly rounded


def _oracle_regress_grad(logits, dv, g, pad, dtype):
    from oracle import mvs_oracle
    x = dv.to(dtype).clone().requires_grad_(True)
    mvs_oracle.depth_regress(logits.to(dtype), x, pad=pad)[1].backward(g.to(dtype))
    return x.grad


def test_regression_values_gradient_against_the_float64_oracle():
    gen = torch.Generator().manual_seed(4400)
    D, H, W, pad = 9, 7, 11, 2
    logits = 2 * torch.randn(D, H + 2 * pad, W + 2 * pad, generator=gen)
    dv = 2 + 9 * torch.rand(D, H + 2 * pad, W + 2 * pad, generator=gen)
    g = torch.randn(H, W, generator=gen)
    want = _oracle_regress_grad(logits, dv, g, pad, torch.float64)
    witness = (_oracle_regress_grad(logits, dv, g, pad, torch.float32).double() - want).abs().max().item()
    bar = 4 * witness + 1e-6 * want.abs().max().item()
    x = dev(dv).requires_grad_(True)
    _, depth, conf = ops().depth_regress(dev(logits), x, pad=pad)
    assert depth.requires_grad and conf.requires_grad
    depth.backward(dev(g))
    err = (x.grad.cpu().double() - want).abs().max().item()
    print("\ndepth_regress, gradient of depth_values: device distance %.3e / bar %.3e = %.3f; float32 witness %.3e" % (err, bar, err / bar, witness))
    assert err <= bar
    assert x.grad[:, :pad].abs().max() == 0 and x.grad[:, :, -pad:].abs().max() == 0
    # the confidence does not depend on depth_values
    x.grad = None
    _, depth, conf = ops().depth_regress(dev(logits), x, pad=pad)
    conf.sum().backward()
    assert x.grad.abs().max() == 0


def test_autograd_wiring_of_depth_hypotheses():
    from uc_nerf_amd.network import mvs_models as M
    c = G.continuous_case("non_integer_ratio_pad1")
    nf = torch.tensor([c["near"], c["far"]], device=DEV)
    kw = dict(near_far=nf, k=c["k"], full_hw=c["HW"], pad=c["pad"])
    cur = dev(c["cur"])
    with torch.no_grad():
        plain = ops().depth_hypotheses(c["D"], c["hw"], cur_depth=cur.clone().requires_grad_(True), **kw)      # grad mode off: today's path
    same = ops().depth_hypotheses(c["D"], c["hw"], cur_depth=cur, **kw)                                         # no grad asked for: today's path
    assert not plain.requires_grad and not same.requires_grad and same.grad_fn is None and torch.equal(plain, same)
    x = cur.clone().requires_grad_(True)
    out = ops().depth_hypotheses(c["D"], c["hw"], cur_depth=x, **kw)
    assert out.requires_grad and torch.equal(out, plain)
    out.backward(dev(c["g_out"]))
    assert torch.equal(x.grad, device_grad(c))
    assert not nf.requires_grad and nf.grad is None
    # through the full-resolution mirror: the output at the map's own resolution, the interval a device value
    lc = G.lattice_case("all_scales_one_D5_pad1")
    x = dev(lc["cur"]).unsqueeze(0).requires_grad_(True)
    got = M.get_depth_range_samples(x, lc["D"], lc["interval"], x.device, x.dtype, list(x.shape), max_depth=lc["far"], min_depth=lc["near"])
    assert got.shape == (1, lc["D"]) + tuple(lc["cur"].shape) and got.requires_grad
    g = dev(lc["g_out"])[:, lc["pad"]:-lc["pad"], lc["pad"]:-lc["pad"]].contiguous()
    got.backward(g.unsqueeze(0))
    direct = ops().depth_hypotheses_bwd(g, dev(lc["cur"]), torch.tensor([lc["near"], lc["far"]], device=DEV), torch.tensor([lc["interval"]], device=DEV),
                                        (lc["D"],) + tuple(lc["cur"].shape) + (0,) + tuple(lc["cur"].shape) + (1.0,))
    assert torch.equal(x.grad[0], direct)
    want, _ = G.chain_grad(lc["cur"], g.cpu(), lc["near"], lc["far"], lc["interval"], lc["D"], lc["HW"], lc["hw"], 0, torch.float64)
    assert torch.equal(direct.cpu().double(), want)
    # an empty map and an empty output go through; a gradient of the wrong shape does not
    e = ops().depth_hypotheses(4, (0, 5), cur_depth=torch.rand(4, 5, device=DEV).requires_grad_(True), near_far=nf, k=1 / 48, full_hw=(8, 10))
    assert e.shape == (4, 0, 5)
    e.sum().backward()
    with pytest.raises(RuntimeError, match="g_out"):
        ops().depth_hypotheses_bwd(torch.zeros(4, 3, 5, device=DEV), cur, nf, None, (4, 4, 5, 0, 8, 10, 1 / 48))


@pytest.mark.parametrize("pad", [0, 2])
def test_depthnet_is_differentiable_in_depth_values(pad):
    from uc_nerf_amd.network.mvs_models import DepthNet
    V, H, W, D = 3, 32, 40, 6
    h, w = H // 4, W // 4
    maps = S.feature_maps(V, H, W, 4500)[0]
    affine, affine_inv = S.cameras(V, H, W, 4501)
    gen = torch.Generator().manual_seed(4502 + pad)
    reg = S.RegStub(torch.randn(1, 1, D, h + 2 * pad, w + 2 * pad, generator=gen)).to(DEV)
    dv = (2 + 9 * torch.rand(1, D, h, w, generator=gen)).to(DEV).requires_grad_(True)
    g = torch.randn(1, h, w, generator=gen).to(DEV)
    feats = [dev(maps[v:v + 1]) for v in range(V)]
    out = DepthNet()(feats, dev(affine[:, 0]), dev(affine_inv[:, 0]), dv, D, reg, None, pad=pad)
    assert out["depth"].requires_grad and out["depth_values"].shape == (1, D, h + 2 * pad, w + 2 * pad)
    out["depth"].backward(g)
    direct = ops()._depth_regress_bwd_values(out["prob_volume"][0], g[0].contiguous(), pad)
    if pad == 0:
        assert torch.equal(dv.grad[0], direct)
    else:                                                 # torch's replicate pad folds the border back (zeros here: the crop drops it)
        assert direct[:, :pad].abs().max() == 0 and torch.equal(dv.grad[0], direct[:, pad:-pad, pad:-pad])
        # ... and with the padded volume itself as the leaf (what CascadeMVSNet hands over)
        leaf = out["depth_values"].detach().clone().requires_grad_(True)
        out2 = DepthNet()(feats, dev(affine[:, 0]), dev(affine_inv[:, 0]), leaf, D, reg, None, pad=pad, depth_values_padded=True)
        assert torch.equal(out2["depth"], out["depth"])
        out2["depth"].backward(g)
        assert torch.equal(leaf.grad[0], direct)
    want = out["prob_volume"][0, :, pad:pad + h, pad:pad + w] * g
    assert torch.equal(dv.grad[0], want)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_cascade")


def _run_net(g, method):
    from uc_nerf_amd.network.mvs_models import CascadeMVSNet
    feature, regs = S.make_stubs(g["V"], g["H"], g["W"], [g["logits%d" % k] for k in (1, 2, 3)], seed=g["feature_seed"])
    net = CascadeMVSNet(grad_method=method, feature=feature, cost_regularization=regs).to(DEV)
    params = []
    for k in range(3):
        lg = torch.nn.Parameter(dev(g["logits%d" % (k + 1)]).clone())
        net.cost_regularization[k].logits = lg
        params.append(lg)
    result = net(dev(g["imgs"]), dev(g["affine_mat"]), dev(g["affine_mat_inv"]), dev(g["near_far"]), pad=g["pad"])
    result[3]["stage3"]["depth"].sum().backward()
    torch.cuda.synchronize()
    return result, params


def _restated_cascade_grads(g, dtype):
    """depth regression (oracle.mvs_oracle) + hypotheses_chain, stage after stage, on the fixed logits: autograd of sum(stage-3 depth)."""
    from oracle import mvs_oracle
    near, far = g["near_far"][0].to(dtype), g["near_far"][1].to(dtype)
    H, W, pad = g["H"], g["W"], g["pad"]
    D1, D2, D3 = (int(d) for d in g["ndepths"])
    interval = (far - near) / 48
    lg = [g["logits%d" % k][0, 0].to(dtype).clone().requires_grad_(True) for k in (1, 2, 3)]
    t = torch.linspace(0., 1., 48, dtype=dtype)
    dv1 = S.row_chain(near * (1. - t) + far * t, D1, (H // 4, W // 4))
    depth1 = mvs_oracle.depth_regress(lg[0], dv1)[1]
    dv2, _ = S.hypotheses_chain(depth1, near, far, 2 * interval, D2, (H, W), (H // 2, W // 2))
    depth2 = mvs_oracle.depth_regress(lg[1], dv2)[1]
    dv3, _ = S.hypotheses_chain(depth2, near, far, 1 * interval, D3, (H, W), (H, W), pad=pad)
    depth3 = mvs_oracle.depth_regress(lg[2], dv3, pad=pad)[1]
    depth3.sum().backward()
    return [x.grad for x in lg]


def test_cascade_trains_through_its_depth_hypotheses(g19):
    g = g19
    (_, _, depth_u, out_u), p_u = _run_net(g, "undetach")
    (_, _, depth_d, out_d), p_d = _run_net(g, "detach")
    # forward outputs of the two modes are bit-equal
    for k in (1, 2, 3):
        for key in ("depth_values", "depth", "photometric_confidence", "prob_volume"):
            assert torch.equal(out_u["stage%d" % k][key], out_d["stage%d" % k][key]), (k, key)
    assert out_u["stage2"]["depth_values"].requires_grad and out_u["stage3"]["depth_values"].requires_grad and not out_u["stage1"]["depth_values"].requires_grad
    assert not any(out_d["stage%d" % k]["depth_values"].requires_grad for k in (1, 2, 3))
    assert p_d[0].grad is None and p_d[1].grad is None and p_d[2].grad is not None
    want = _restated_cascade_grads(g, torch.float64)
    wit = _restated_cascade_grads(g, torch.float32)
    for k in (0, 1, 2):
        got = p_u[k].grad
        assert got is not None and torch.isfinite(got).all() and got.abs().sum() > 0, "stage %d logits got no gradient" % (k + 1)
        witness = (wit[k].double() - want[k]).abs().max().item()
        bar = 4 * witness + 1e-6 * want[k].abs().max().item()
        err = (got[0, 0].cpu().double() - want[k]).abs().max().item()
        print("\nstage-%d logits: device distance %.3e / bar %.3e = %.3f; float32 witness %.3e; max|reference| %.3e"
              % (k + 1, err, bar, err / bar, witness, want[k].abs().max().item()))
        assert err <= bar
    # the last stage's own logits get the same gradient in both modes
    assert torch.equal(p_u[2].grad, p_d[2].grad)


def test_ray_builders_take_the_undetached_outputs(g19):
    """The test-time builder and the training builder's launch read depth_values as data: outputs that carry a graph go through, and what comes
    back carries none."""
    from uc_nerf_amd.utils import utils as U
    g = g19
    (_, _, _, outputs), _ = _run_net(g, "undetach")
    H, W, pad, n_samples, chunk = g["H"], g["W"], g["pad"], 9, 256
    K = torch.tensor([[0.9 * W, 0, 0.5 * W], [0, 0.9 * W, 0.5 * H], [0, 0, 1]], device=DEV)
    c2w = torch.eye(4, device=DEV)
    nf = dev(g["near_far"]).view(1, 2)
    pts, rays_dir, ndc, z, rays_o, _ = U.build_rays_test(H, W, c2w, torch.eye(4, device=DEV), K, nf, nf[-1], n_samples, pad=pad, chunk=chunk, idx=1, outputs=outputs)
    assert pts.shape == (chunk, n_samples, 3) and not pts.requires_grad and not z.requires_grad and torch.isfinite(pts).all()
    dvs = [outputs["stage%d" % k]["depth_values"] for k in (1, 2, 3)]
    assert dvs[1].requires_grad and dvs[2].requires_grad
    imgs = torch.rand(1, 1, 3, H, W, device=DEV)
    o = ops().build_rays_train(imgs, K, c2w, torch.eye(4, device=DEV), K, nf[0], dvs, n_samples, 4, ux=torch.tensor([3., 17.], device=DEV),
                               uy=torch.tensor([5., 30.], device=DEV), t_rand=torch.rand(2, n_samples, device=DEV))
    assert o["pts"].shape == (2, n_samples, 3) and not o["pts"].requires_grad and torch.isfinite(o["pts"]).all()
    rng = U._stage_ranges(outputs, torch.tensor([[5, 30], [3, 17]], device=DEV))          # (the composed training route's reader)
    assert rng.shape == (2, 6) and not rng.requires_grad and torch.isfinite(rng).all()
