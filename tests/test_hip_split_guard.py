"""The guarded fp16 split on the GPU: set_split_operand("fp16_guarded") computes what "fp16" computes, notices on the device when an activation, an
input or a weight left fp16's safe range (|x| >= 65 504) and then re-renders the launch on bf16 terms without a host synchronisation.  Every
comparison between routes is torch.equal: a guarded call is bit-identical to "fp16" when nothing saturated and to "bf16" when something did.

Routes: ops.mlp_fwd (precision 1), the gather-fused pass (precision 3), its one-launch tail route, CoarseFineRenderer eager and graphed, and the
rendering() drop-in.  The tests run one after the other in one process; the status word is cleared at the start of each."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_STEP = 2.0 ** 9        # scale of each of the two amplifying trunk layers: a power of two, so the fp32 network is the benign one bit for bit


@pytest.fixture(autouse=True)
def _restore_mode():
    import uc_nerf_amd
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd import ops
    ops.split_guard_clear()
    yield
    uc_nerf_amd.set_split_operand("bf16")
    uc_nerf_amd.set_inference_precision("bf16x3_fused")
    L.lib().ucnerf_set_fused_tail(1)
    ops.split_guard_clear()


# ---------------------------------------------------------------------------------------------- networks
def benign_sd(seed=3):
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    return init_ucnerf_state_dict(seed=seed, sigma_scale=0.05, sigma_bias=0.05)     # the bench / G11 network with the 0.05 density-head scale


def big_activation_sd(sd):
    """Trunk layers 1 and 2 amplify by 2^9 each and layer 3's weights undo it (2^-18): h2 leaves fp16's range (checked on the CPU by the callers)
    while every WEIGHT stays far inside it (|w| < 2^9 * 1: the weight side must not be what raises the flag).  relu is positively homogeneous and
    the scales are powers of two, so in fp32 everything behind layer 3 is what the unscaled network gives -- finite throughout."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["nerf.pts_linears.1.weight"] *= K_STEP
    sd["nerf.pts_linears.1.bias"] *= K_STEP
    sd["nerf.pts_linears.2.weight"] *= K_STEP
    sd["nerf.pts_linears.2.bias"] *= K_STEP * K_STEP
    sd["nerf.pts_linears.3.weight"] /= K_STEP * K_STEP
    assert max(float(v.abs().max()) for v in sd.values()) < 65504 / 8
    return sd


def big_weight_sd(sd):
    sd = {k: v.clone() for k, v in sd.items()}
    sd["nerf.pts_linears.1.weight"][5, 7] = 1e5
    return sd


def trunk_h2_cpu(sd, e_pts, feats, n_src):
    """Plain torch restatement of the trunk through layer 2 (network/models.py:138-184): h_l = relu((W_l h_{l-1} + b_l) * b_depth), float32 on the CPU."""
    mvs = feats[..., :24 + 4 * n_src]
    bd = mvs @ sd["nerf.pts_bias_depth_fine.weight"].T + sd["nerf.pts_bias_depth_fine.bias"]
    h = e_pts
    for i in range(3):
        h = torch.relu((h @ sd["nerf.pts_linears.%d.weight" % i].T + sd["nerf.pts_linears.%d.bias" % i]) * bd)
    return h


# ---------------------------------------------------------------------------------------------- routes: each returns f(sd) -> tuple of tensors
def mlp_route(m=2048, S=64, n_src=6, seed=0):
    from uc_nerf_amd import ops
    from uc_nerf_amd.pipeline import flat_params_of
    g = torch.Generator().manual_seed(seed)
    F = 24 + 12 * n_src + 1
    pts, dirs = torch.rand(m, 3, generator=g), torch.randn(m // S, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    feats = torch.randn(m, F, generator=g)
    feats[:, -1] = torch.rand(m, generator=g)
    dpts, ddirs, dfeats = pts.to(DEV), dirs.to(DEV), feats.to(DEV)

    def run(sd):
        pw = ops.PackedWeights.get(n_src, 0, torch.device(DEV), "bf16x3")
        return (ops.mlp_fwd(pw, pw.pack(flat_params_of(sd).to(DEV)), dpts, ddirs, dfeats, S),)
    run.inputs = (pts, feats)
    return run


def renderer_route(n=512, tail=False, graphed=False):
    from uc_nerf_amd import _lib as L
    from uc_nerf_amd.pipeline import CoarseFineRenderer, flat_params_of
    from uc_nerf_amd.synthetic import make_scene, random_pixels, scene_to
    scene_cpu = make_scene(seed=3, H=32, W=40, small_volumes=True)
    scene = scene_to(scene_cpu, torch.device(DEV))
    xs, ys = random_pixels(n, 32, 40, seed=4)
    dxs, dys = xs.to(DEV), ys.to(DEV)

    def run(sd):
        L.lib().ucnerf_set_fused_tail(1 if tail else 0)
        before = L.lib().ucnerf_fused_tail_launches()
        r = CoarseFineRenderer(scene, flat_params_of(sd).to(DEV), 64, 128, precision="bf16x3_fused")
        out = r.capture(n)(dxs, dys) if graphed else r.render(dxs, dys)
        torch.cuda.synchronize()
        assert (L.lib().ucnerf_fused_tail_launches() > before) == tail
        return tuple(out[k].clone() for k in ("rgb", "depth", "acc", "z_fine")) + (out["coarse"]["weights"].clone(),)
    run.scene_cpu, run.pixels = scene_cpu, (xs, ys)
    return run


def dropin_route(sd_v7):
    from conftest import load_golden
    from test_hip_round4 import _call, _mods, _net, _qfn
    mods = _mods()
    g = load_golden("g10_rendering")
    qfn = _qfn(mods)

    def run(sd):
        net = _net(mods, g["V"], sd)
        with torch.no_grad():
            rgb, depth = _call(mods, g, net, qfn)
        return rgb.clone(), depth.clone()
    run.sd = sd_v7
    return run


def in_modes(run, sd, modes=("bf16", "fp16", "fp16_guarded")):
    """run(sd) under each split operand; the status word is cleared before the guarded call and read after it."""
    import uc_nerf_amd
    from uc_nerf_amd import ops
    out = {}
    for mode in modes:
        uc_nerf_amd.set_split_operand(mode)
        if mode == "fp16_guarded":
            ops.split_guard_clear()
        out[mode] = run(sd)
        if mode == "fp16_guarded":
            out["status"] = ops.split_guard_status()
    uc_nerf_amd.set_split_operand("bf16")
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def finite(a):
    return all(bool(torch.isfinite(x).all()) for x in a)


def check_route(run, sd, h2_max):
    """Benign scene, out-of-range activations, an out-of-range weight, sticky and clear -- on one route.  h2_max: the CPU's max |h2| of the scaled
    network on this route's inputs (None where the route's inputs are not restated on the CPU: the device's bit 0 is then the evidence)."""
    import uc_nerf_amd
    from uc_nerf_amd import ops
    # 1. benign: bit-identical to "fp16", nothing flagged
    o = in_modes(run, sd)
    print("benign: status %d, guarded == fp16 %s, fp16 == bf16 %s" % (o["status"], same(o["fp16_guarded"], o["fp16"]), same(o["fp16"], o["bf16"])))
    assert o["status"] == 0 and same(o["fp16_guarded"], o["fp16"]) and finite(o["fp16_guarded"])
    benign = o
    # 2. a hidden activation beyond 131 008, everything finite in fp32: bit-identical to "bf16", bit 0 set
    if h2_max is not None:
        print("max |h2| on the CPU: %.4g" % h2_max)
        assert 131008 < h2_max < 1e30
    o = in_modes(run, big_activation_sd(sd))
    print("activations: status %d, guarded == bf16 %s, unguarded fp16 differs from bf16: %s (max |d| %.3g)"
          % (o["status"], same(o["fp16_guarded"], o["bf16"]), not same(o["fp16"], o["bf16"]),
             max(float((x - y).abs().nan_to_num(nan=math.inf).max()) for x, y in zip(o["fp16"], o["bf16"]))))
    assert o["status"] == 1 and same(o["fp16_guarded"], o["bf16"]) and finite(o["fp16_guarded"])
    # 5. sticky: the word is still set, so a benign call replays and equals "bf16"; after a clear it equals "fp16" and the word reads 0
    uc_nerf_amd.set_split_operand("fp16_guarded")
    again = run(sd)
    assert ops.split_guard_status() & 1 and same(again, benign["bf16"])
    ops.split_guard_clear()
    again = run(sd)
    assert same(again, benign["fp16"]) and ops.split_guard_status() == 0
    # 3. one weight at 1e5: bit 1, finite, bit-identical to "bf16"
    o = in_modes(run, big_weight_sd(sd))
    print("weight: status %d, guarded == bf16 %s, unguarded fp16 finite: %s" % (o["status"], same(o["fp16_guarded"], o["bf16"]), finite(o["fp16"])))
    assert o["status"] & 2 and finite(o["fp16_guarded"]) and same(o["fp16_guarded"], o["bf16"])


def test_guard_on_the_stand_alone_network_launch():
    from oracle import ucnerf_oracle as O            # checker only (the encoding of the CPU restatement)
    run, sd = mlp_route(), benign_sd()
    pts, feats = run.inputs
    h2 = trunk_h2_cpu(big_activation_sd(sd), O.embed_live(pts, 10), feats, 6)
    check_route(run, sd, float(h2.abs().max()))


def _renderer_h2_max(run, sd):
    """max |h2| of the scaled network over the COARSE pass's samples, on the CPU: the oracle's own features and coordinates of that pass."""
    from oracle import ucnerf_oracle as O
    sc, (xs, ys) = run.scene_cpu, run.pixels
    n = min(64, xs.shape[0])
    xs, ys = xs[:n], ys[:n]
    ref = O.render_coarse_fine(sd, sc, xs, ys, 64, 128)
    rays_o, rays_d, _ = O.get_rays_mvs_pixels(xs, ys, sc["K"], sc["c2w"])
    z = ref["z_coarse"]
    pts = rays_o.expand(n, 3)[:, None] + rays_d[:, None] * z[..., None]
    H, W = sc["imgs"].shape[-2:]
    ndc = O.get_ndc_coordinate(sc["w2cs"][0], sc["intrinsics"][0], pts, torch.tensor([W - 1, H - 1], dtype=torch.float32),
                               O.scene_near_far(n, 64, sc["near"], sc["far"], torch.float32))
    ndc = ndc["ndc"] if isinstance(ndc, dict) else ndc[-1] if isinstance(ndc, (tuple, list)) else ndc
    h2 = trunk_h2_cpu(big_activation_sd(sd), O.embed_live(ndc, 10), ref["coarse"]["feats"], sc["w2cs"].shape[0] - 1)
    return float(h2.abs().max())


@pytest.mark.parametrize("tail,graphed", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["gather_fused", "tail_route", "gather_fused_graphed", "tail_route_graphed"])
def test_guard_on_the_coarse_fine_renderer(tail, graphed):
    run, sd = renderer_route(tail=tail, graphed=graphed), benign_sd()
    check_route(run, sd, _renderer_h2_max(run, sd))


def test_guard_on_the_rendering_drop_in(sd_v7):
    run = dropin_route(sd_v7)
    sd = {k: v.clone() for k, v in run.sd.items()}
    for nme in ("nerf.alpha_linear", "nerf.alpha_linear_1"):      # (the reference initialisation with the 0.05 density-head scale)
        sd[nme + ".weight"] = sd[nme + ".weight"] * 0.05
    check_route(run, sd, None)


# ---------------------------------------------------------------------------------------------- 4. the threshold, at two sites
def unit_path_sd(n_src=6, hidden=None):
    """An all-zero network with one live unit path: feature 0 -> b_depth[0] (weight 2^-16, or 1 for the hidden-layer probe) multiplies unit 0 of
    every trunk layer; layer 0's unit 0 is its bias 1; layers 1 .. 5 pass unit 0 on with weight 1; the base heads read unit 0.
    hidden = v: layer 1's unit 0 becomes its BIAS v (fp32 constants are not fp16 terms: no weight is out of range) and layer 2 scales it by 2^-16."""
    from uc_nerf_amd.synthetic import ucnerf_param_shapes
    sd = {name: torch.zeros(shape) for name, shape in ucnerf_param_shapes(n_src)}
    sd["nerf.pts_bias_depth_fine.weight"][0, 0] = 1.0 if hidden is not None else 2.0 ** -16
    sd["nerf.pts_linears.0.bias"][0] = 1.0
    for l in range(1, 6):
        sd["nerf.pts_linears.%d.weight" % l][0, 63 if l == 5 else 0] = 1.0
    if hidden is not None:
        sd["nerf.pts_linears.1.weight"][0, 0] = 0.0
        sd["nerf.pts_linears.1.bias"][0] = hidden
        sd["nerf.pts_linears.2.weight"][0, 0] = 2.0 ** -16
    sd["nerf.alpha_linear_1.weight"][0, 0] = 1.0
    sd["nerf.confi_rgb_linear.weight"][:, 0] = 1.0
    return sd


@pytest.mark.parametrize("site", ["input_feature", "hidden_layer"])
def test_the_flag_turns_at_fp16s_largest_finite_value(site):
    from uc_nerf_amd import ops
    from uc_nerf_amd.pipeline import flat_params_of
    m, S, F = 256, 64, 97
    pts, dirs = torch.full((m, 3), 0.25, device=DEV), torch.tensor([[0., 0., 1.]], device=DEV).repeat(m // S, 1)
    pw = lambda: ops.PackedWeights.get(6, 0, torch.device(DEV), "bf16x3")      # noqa: E731  (the packer of the current mode)
    for v, flagged in ((65000.0, False), (65504.0, True), (70000.0, True)):
        feats = torch.zeros(m, F, device=DEV)
        feats[:, -1] = 0.5
        feats[:, 0] = 1.0
        if site == "input_feature":
            feats[7, 0] = v                                   # ONE sample carries the probe value
            sd = unit_path_sd()
        else:
            sd = unit_path_sd(hidden=v)
        flat = flat_params_of(sd).to(DEV)
        run = lambda _sd: (ops.mlp_fwd(pw(), pw().pack(flat), pts, dirs, feats, S),)      # noqa: E731
        o = in_modes(run, None)
        print("%s = %g: status %d, sigma %s" % (site, v, o["status"], o["fp16_guarded"][0][7].tolist()))
        assert float(o["bf16"][0][7, 3]) > 0.1            # the path is live: the probe value reaches the density head
        if flagged:
            assert o["status"] == 1 and same(o["fp16_guarded"], o["bf16"])
        else:
            assert o["status"] == 0 and same(o["fp16_guarded"], o["fp16"])


def test_training_forward_refuses_the_mode_where_it_refuses_fp16():
    import uc_nerf_amd
    from uc_nerf_amd import ops
    uc_nerf_amd.set_split_operand("fp16_guarded")
    pw = ops.PackedWeights.get(3, 0, torch.device(DEV), "bf16x3")
    assert pw.guarded and pw.cfg.operand == 1
    m = 64
    flat = torch.zeros(pw.n_params, device=DEV)
    with pytest.raises(RuntimeError, match="bf16 terms"):
        ops.mlp_fwd_train(pw, pw.pack(flat), torch.zeros(m, 3, device=DEV), torch.zeros(m, 3, device=DEV), torch.zeros(m, 24 + 36 + 1, device=DEV), 1)
    assert ops.split_guard_status() == 0
