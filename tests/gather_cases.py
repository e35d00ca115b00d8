"""Cases and float64 reference for the feature gather's edge tests (tests/test_gather_cases_host.py, tests/test_hip_gather_edges.py).

The reference is oracle.ucnerf_oracle.gen_pts_feats run in float64, with autograd through it for the five source gradients.

LATTICE cases are exact: sources and g_feats hold small integers, every interpolation coordinate is dyadic with a few fraction bits, so each
weight, each product and each partial sum of the float32 kernels is representable -- whatever the order of the atomics.  The builder asserts
that itself (check_lattice): the float32 oracle equals the float64 oracle element for element, and
    max|reference| * 2^(fraction bits of the weights) < 2^24
for the features and, with |g_feats| in place of g_feats (which bounds every partial sum, not only the final one), for every gradient.
Both are conditions on the inputs.  A device result may then be compared with torch.equal.

How a lattice sample is placed:
  stage coordinates  u = k / gran on every axis, k swept over [-gran/4, 5 gran/4]: past both borders, on them, on texels and between;
  world points       chosen for ONE source view so that its pixel coordinate is a given multiple of 1/4 in [-2, W + 1] x [-2, H + 1] at a camera
                     depth in {0.5, 1, 2, 4, -1, -2}; W - 1, H - 1, the focal lengths are powers of two, w2c = [R | t] with R a signed
                     permutation that keeps the optical axis up to sign and t = (tx, ty, 0) integer -- so the point is dyadic in every other
                     view as well, in front of some and behind others;
  clamp points       camera depth 0, +-2^-14 (inside the |cz| < 1e-4 clamp: the reference moves them to +1e-4, sign dropped) and +-2^-13 (outside
                     it), with lateral offsets of 3 and 5: the projection lands far outside and the footprint is a border texel;
  runs               samples repeated along the sample dimension (the backward combines runs of equal cells over 16 samples of a wave, 64 for
                     the confidence map).

CONTINUOUS cases hold random sources, coordinates uniform over [-0.3, 1.3] and fuzz_render.pose cameras (its "wild" setting included), points in
front of and behind the cameras.  They are compared under a bar derived from the float32 oracle's own distance to the float64 reference
(f32_distance); per (sample, view) the in-mask bit and the view's features are left out where the float64 | |gx| - 1 | or | |gy| - 1 | < 1e-4, and
the whole view where |cz| < 1e-2 -- at most 2 % of a case (asserted by the builder)."""
import functools

import numpy as np
import torch

from oracle import ucnerf_oracle as O

F64 = torch.float64
DEPTHS = (0.5, 1.0, 2.0, 4.0, -1.0, -2.0)
CLAMP_DEPTHS = (0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -13, -2.0 ** -13)
# rotations that keep the optical axis up to sign: identity, quarter and half turn about z, half turns about x and y (the last two look backwards)
ROTS = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],
        [[1, 0, 0], [0, -1, 0], [0, 0, -1]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]]
SHIFTS = [(0, 0), (1, 0), (0, -1), (-2, 1), (1, 1), (2, -1), (-1, -2), (0, 2)]
FOCALS = (8.0, 8.0, 4.0, 16.0, 8.0, 4.0, 8.0, 16.0)
GRADS = ("g_vol1", "g_vol2", "g_vol3", "g_conf", "g_img_feat")


def columns(V):
    """Column groups of the feature row [vol 24 | (rgb, mask) x V | img_feat 8 x V | conf]."""
    F = 24 + 12 * V + 1
    rgb = [24 + 4 * v + c for v in range(V) for c in range(3)]
    return {"volumes": list(range(24)), "colours": rgb, "mask": [24 + 4 * v + 3 for v in range(V)],
            "view_feats": list(range(24 + 4 * V, 24 + 12 * V)), "confidence": [F - 1]}


def lattice_cameras(V, H, W):
    w2cs, Ks = [], []
    for v in range(V):
        m = torch.eye(4, dtype=F64)
        m[:3, :3] = torch.tensor(ROTS[v % len(ROTS)], dtype=F64)
        m[:2, 3] = torch.tensor(SHIFTS[v % len(SHIFTS)], dtype=F64)
        w2cs.append(m)
        f = FOCALS[v % len(FOCALS)]
        Ks.append(torch.tensor([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], dtype=F64))
    return torch.stack(w2cs), torch.stack(Ks)


def _integer_sources(gen, V, H, W, dhw):
    ri = lambda *s: torch.randint(-8, 9, s, generator=gen).to(F64)      # noqa: E731
    return dict(vols=[ri(1, 8, *s) for s in dhw], confidence=ri(H, W), imgs=ri(1, V, 3, H, W), img_feat=ri(V, 1, 8, H, W))


def _site(j, V, H, W, gran, w2cs, Ks):
    """Site j: three stage coordinates and one world point (float64 rows of 3)."""
    lat = np.arange(-(gran // 4), gran + gran // 4 + 1) / gran
    n = len(lat)                                                     # 13 or 25: the strides below are coprime to both
    strides = ((1, 2, 3), (4, 6, 7), (8, 9, 11))
    stages = [[lat[(j * strides[s][a] + 3 * s + a) % n] for a in range(3)] for s in range(3)]
    v = (j // 6) % V
    K, M = Ks[v], w2cs[v]
    if j % 11 == 10:                                                 # a point on / next to the camera plane of view v
        q = j // 11
        cam = [3.0 if q % 2 else -3.0, 5.0 if (q // 2) % 2 else -5.0, CLAMP_DEPTHS[q % 5]]
    else:
        pxs, pys = np.arange(-8, 4 * (W + 1) + 1) / 4, np.arange(-8, 4 * (H + 1) + 1) / 4
        px, py, d = pxs[(j * 5 + 2) % len(pxs)], pys[(j * 4 + 1) % len(pys)], DEPTHS[j % 6]
        cam = [(px - K[0, 2].item()) * d / K[0, 0].item(), (py - K[1, 2].item()) * d / K[1, 1].item(), d]
    world = M[:3, :3].T @ (torch.tensor(cam, dtype=F64) - M[:3, 3])
    return stages, world.tolist()


def lattice_case(name, V, HW, dhw, order, gran=16, seed=0, g_amp=2):
    """order: site index of every sample (a repeated index = a run of equal cells in every unit)."""
    H, W = HW
    gen = torch.Generator().manual_seed(seed)
    w2cs, Ks = lattice_cameras(V, H, W)
    case = dict(name=name, kind="lattice", V=V, H=H, W=W, dhw=[tuple(s) for s in dhw], w2cs=w2cs, intrinsics=Ks)
    case.update(_integer_sources(gen, V, H, W, dhw))
    order = np.asarray(order, dtype=np.int64)
    sites = {int(j): _site(int(j), V, H, W, gran, w2cs, Ks) for j in np.unique(order)}
    m = len(order)
    for s in range(3):
        case["stage%d" % (s + 1)] = torch.tensor([sites[int(j)][0][s] for j in order], dtype=F64).view(m, 1, 3)
    case["pts"] = torch.tensor([sites[int(j)][1] for j in order], dtype=F64).view(m, 1, 3)
    case["g_feats"] = torch.randint(-g_amp, g_amp + 1, (m, 1, 24 + 12 * V + 1), generator=gen).to(F64)
    case["m"] = m
    return case


def derived_case(name, n, S, V, per_ray, seed=0):
    """A lattice scene whose REFERENCE camera is of the exact kind too: the pass derives points and stage coordinates from (ray, depth).
    Rays go through pixels at multiples of 1/2 (all different), depths are powers of two, near / far ranges have power-of-two widths."""
    H, W = 5, 9
    gen = torch.Generator().manual_seed(seed)
    dhw = [(3, 5, 2), (8, 3, 5), (2, 2, 3)]
    w2cs, Ks = lattice_cameras(V, H, W)
    case = dict(name=name, kind="lattice", V=V, H=H, W=W, dhw=dhw, w2cs=w2cs, intrinsics=Ks, n=n, S=S, m=n * S)
    case.update(_integer_sources(gen, V, H, W, dhw))
    t_ref = torch.tensor([1.0, -2.0, 0.0], dtype=F64)
    case["w2c_ref"] = torch.eye(4, dtype=F64)
    case["w2c_ref"][:3, 3] = t_ref
    case["K_ref"] = torch.tensor([[8.0, 0, 4], [0, 8.0, 2], [0, 0, 1]], dtype=F64)
    case["rays_o"] = -t_ref
    pxs, pys = np.arange(-4, 2 * (W + 1) + 1) / 2, np.arange(-4, 2 * (H + 1) + 1) / 2        # 25 and 17 values
    r = np.arange(n)
    px, py = pxs[(r * 7 + 1) % len(pxs)], pys[(r // len(pxs) * 5 + r * 3 + 2) % len(pys)]
    case["rays_d"] = torch.tensor(np.stack([(px - 4) / 8, (py - 2) / 8, np.ones(n)], -1), dtype=F64)
    e = (r[:, None] + 2 * np.arange(S)[None, :]) % 5 - 2
    case["z"] = torch.sort(torch.tensor(2.0 ** e, dtype=F64), -1)[0]
    case["near"], case["far"] = 0.0, 4.0
    if per_ray:
        lo, wd = np.array([0.0, 0.5, -1.0]), np.array([4.0, 2.0, 8.0])
        nf = [np.stack([lo[(r + k) % 3], lo[(r + k) % 3] + wd[(r // 3 + k) % 3]], -1) for k in range(3)]
        case["near_far"] = torch.tensor(np.concatenate(nf, -1), dtype=F64)                    # [n,6]
    case["g_feats"] = torch.randint(-2, 3, (n, S, 24 + 12 * V + 1), generator=gen).to(F64)
    derive(case, F64, into=case)
    return case


def derive(case, dtype, into=None):
    """Points and stage coordinates of a derived case from its rays, depths and reference camera (get_ndc_coordinate), in `dtype`."""
    n, S = case["z"].shape
    c = lambda t: t.to(dtype)      # noqa: E731
    pts = c(case["rays_o"]).view(1, 1, 3) + c(case["rays_d"])[:, None] * c(case["z"])[..., None]
    nf = {"near": case["near"], "far": case["far"]}
    for i, k in enumerate(("near_1", "far_1", "near_2", "far_2", "near_3", "far_3")):
        nf[k] = c(case["near_far"])[:, i].view(n, 1, 1).expand(n, S, 1) if "near_far" in case else case["far" if i % 2 else "near"]
    ndc = O.get_ndc_coordinate(c(case["w2c_ref"]), c(case["K_ref"]), pts, torch.tensor([case["W"] - 1, case["H"] - 1], dtype=dtype), nf)
    out = into if into is not None else {}
    out["pts"] = pts
    for k in ("stage1", "stage2", "stage3"):
        out[k] = ndc[k]
    return out


def reference(case, dtype=F64, bf16_sources=False, g_feats=None, want_grads=True):
    """gen_pts_feats in `dtype` (sources rounded to bf16 first when asked) -> (feats [.., F], dict of the five source gradients)."""
    def src(t):
        t = t.to(torch.bfloat16).to(dtype) if bf16_sources else t.to(dtype)
        return t.clone().requires_grad_(want_grads)
    vols, conf, img_feat = [src(v) for v in case["vols"]], case["confidence"].to(dtype).clone().requires_grad_(want_grads), src(case["img_feat"])
    imgs = src(case["imgs"]).detach()
    co = derive(case, dtype) if ("rays_d" in case and dtype != F64) else case
    ndc = {k: co[k].to(dtype) for k in ("stage1", "stage2", "stage3")}
    feats = O.gen_pts_feats(imgs, vols, co["pts"].to(dtype), case["w2cs"].to(dtype), case["intrinsics"].to(dtype), ndc, img_feat, conf)
    grads = {}
    if want_grads:
        feats.backward((case["g_feats"] if g_feats is None else g_feats).to(dtype))
        got = vols + [conf, img_feat]
        grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).detach() for k, t in zip(GRADS, got)}
    return feats.detach(), grads


# ------------------------------------------------------------------------------------------------ geometry of a case, from its float64 coordinates
def geometry(case):
    """Float64 footprint coordinates: per stage the unnormalised clamped (x, y, z) [m], for the confidence map (x, y), per view gx, gy, cz [V,m]
    and the unnormalised clamped pixel (x, y)."""
    g = {"vol": [], "view": {}}
    for s, (D, h, w) in enumerate(case["dhw"]):
        u = case["stage%d" % (s + 1)].reshape(-1, 3) * 2 - 1.0
        g["vol"].append([O._unnorm(u[:, a], size, False) for a, size in enumerate((w, h, D))])
    u = case["stage3"].reshape(-1, 3) * 2 - 1.0
    g["conf"] = [O._unnorm(u[:, 0], case["W"], False), O._unnorm(u[:, 1], case["H"], False)]
    gx, gy, cz = [], [], []
    inv = torch.tensor([case["W"] - 1, case["H"] - 1], dtype=F64)
    pts = case["pts"].reshape(-1, 3)
    for v in range(case["V"]):
        q = O.project_points(case["w2cs"][v], case["intrinsics"][v], pts, inv)
        gx.append(q[:, 0] * 2 - 1.0); gy.append(q[:, 1] * 2 - 1.0)
        cz.append(pts @ case["w2cs"][v][2, :3] + case["w2cs"][v][2, 3])
    g["view"] = dict(gx=torch.stack(gx), gy=torch.stack(gy), cz=torch.stack(cz))
    g["view"]["x"], g["view"]["y"] = O._unnorm(g["view"]["gx"], case["W"], True), O._unnorm(g["view"]["gy"], case["H"], True)
    return g


def _frac_bits(x):
    """Smallest b with x * 2^b integer for every element (float64 input)."""
    for b in range(0, 40):
        y = x * 2.0 ** b
        if bool((y == torch.floor(y)).all()):
            return b
    raise AssertionError("coordinate is not dyadic")


def weight_bits(case):
    """Fraction bits of the interpolation weights per column group / gradient tensor."""
    g = geometry(case)
    vol = [sum(_frac_bits(a) for a in axes) for axes in g["vol"]]
    conf = sum(_frac_bits(a) for a in g["conf"])
    view = _frac_bits(g["view"]["x"]) + _frac_bits(g["view"]["y"])
    return dict(g_vol1=vol[0], g_vol2=vol[1], g_vol3=vol[2], g_conf=conf, g_img_feat=view, volumes=max(vol), confidence=conf, colours=view,
                view_feats=view)


def check_lattice(case):
    """The exactness conditions (module docstring); returns the float64 reference (feats, grads)."""
    feats, grads = reference(case)
    f32, g32 = reference(case, torch.float32)
    assert torch.equal(f32.double(), feats), "%s: float32 oracle != float64 oracle (features)" % case["name"]
    for k in GRADS:
        assert torch.equal(g32[k].double(), grads[k]), "%s: float32 oracle != float64 oracle (%s)" % (case["name"], k)
    bits = weight_bits(case)
    cols = columns(case["V"])
    for grp in ("volumes", "colours", "view_feats", "confidence"):
        assert feats[..., cols[grp]].abs().max().item() * 2.0 ** bits[grp] < 2 ** 24, (case["name"], grp)
        assert 8 * 8 * 2.0 ** bits[grp] < 2 ** 24                     # every partial sum of a footprint: 8 corners of |v| <= 8
    _, bound = reference(case, g_feats=case["g_feats"].abs())           # sum of |contribution| per cell: bounds every partial sum of the atomics
    for k in GRADS:
        assert grads[k].abs().max().item() <= bound[k].max().item()
        assert 2 * bound[k].max().item() * 2.0 ** bits[k] < 2 ** 24, (case["name"], k, bound[k].max().item(), bits[k])      # (2: the call-twice test)
    return feats, grads


def census(case):
    """What a case contains, decided from its float64 coordinates: counts of (sample, view) pairs / samples."""
    g = geometry(case)
    v = g["view"]
    gx, gy, cz = v["gx"], v["gy"], v["cz"]
    inside_y, inside_x = (gy > -1) & (gy < 1), (gx > -1) & (gx < 1)
    out = {"edge_x_lo": (gx == -1) & inside_y, "edge_x_hi": (gx == 1) & inside_y, "edge_y_lo": (gy == -1) & inside_x, "edge_y_hi": (gy == 1) & inside_x,
           "view_texel": inside_x & inside_y & (v["x"] == v["x"].floor()) & (v["y"] == v["y"].floor()),
           "out_x_lo": gx < -1, "out_x_hi": gx > 1, "out_y_lo": gy < -1, "out_y_hi": gy > 1,
           "behind": cz < -1e-4, "clamped": cz.abs() < 1e-4, "clamped_negative": (cz.abs() < 1e-4) & (cz < 0), "clamped_zero": cz == 0}
    vx, vy, vz = g["vol"][2]
    s3 = case["stage3"].reshape(-1, 3)
    out["vol_texel"] = (vx == vx.floor()) & (vy == vy.floor()) & (vz == vz.floor())
    out["vol_out_lo"] = (s3 < 0).any(-1)
    out["vol_out_hi"] = (s3 > 1).any(-1)
    out = {k: int(t.sum()) for k, t in out.items()}
    # runs of equal cells: cell id of the finest volume and of view 0 per sample; an absorbed run = positions 7 and 8 of a wave's 16 samples equal
    cells = [torch.stack([vx.floor(), vy.floor(), vz.floor()], -1), torch.stack([v["x"][0].floor(), v["y"][0].floor()], -1)]
    m = case["m"]
    absorbed = aba = 0
    for c in cells:
        same = (c[1:] == c[:-1]).all(-1)                                 # sample i + 1 in the cell of sample i
        idx = torch.arange(m - 1)
        absorbed += int((same & (idx % 16 == 7)).sum())
        if m >= 3:
            aba += int(((c[2:] == c[:-2]).all(-1) & ~same[:-1] & ((idx[:-1] // 16) == ((idx[:-1] + 2) // 16))).sum())
    out["absorbed_run"], out["a_b_a"] = absorbed, aba
    return out


# ------------------------------------------------------------------------------------------------ the lattice cases
VOLS_A = [(1, 2, 3), (3, 5, 2), (8, 3, 5)]
VOLS_B = [(2, 3, 1), (5, 1, 7), (7, 8, 2)]
VOLS_C = [(3, 5, 2), (1, 1, 2), (2, 7, 8)]      # (not 1x1x1: that memory is channel-major and channel-last at once)
RUN_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 33, 64, 65)
RUN_OFFSETS = (0, 1, 7, 8, 15)


def run_order():
    """Runs of every length in RUN_LENGTHS starting at every offset in RUN_OFFSETS within a wave's 16 samples; singles (each its own site) between."""
    order, nxt = [], 0
    for off in RUN_OFFSETS:
        for length in RUN_LENGTHS:
            while len(order) % 16 != off:                               # singles up to the start position
                order.append(nxt); nxt += 1
            order += [nxt] * length
            nxt += 1
            order.append(nxt); nxt += 1                                   # a different cell ends the run
    return order


def aba_order():
    """A B A at every position of a wave's 16 samples (and across its middle and its end), then A A B A A."""
    order = []
    for k in range(20):
        order += [2 * k, 2 * k + 1, 2 * k]
    return order + [50, 50, 51, 50, 50]


LATTICE_SPECS = {
    "sweep_v1_m1000": dict(V=1, HW=(5, 9), dhw=VOLS_A, order=list(range(1000)), gran=16),
    "sweep_v2_m257": dict(V=2, HW=(9, 17), dhw=VOLS_B, order=list(range(257)), gran=8),
    "sweep_v3_m255": dict(V=3, HW=(5, 9), dhw=VOLS_C, order=list(range(255)), gran=16),
    "sweep_v8_m256": dict(V=8, HW=(9, 17), dhw=VOLS_A, order=list(range(256)), gran=8),
    "runs_v2": dict(V=2, HW=(5, 9), dhw=VOLS_A, order=run_order(), gran=8),
    "a_b_a_v1": dict(V=1, HW=(5, 9), dhw=VOLS_C, order=aba_order(), gran=16),
    "one_cell_v1_m257": dict(V=1, HW=(5, 9), dhw=VOLS_B, order=[5] * 257, gran=16),
}
for _m, _V in ((1, 1), (7, 2), (8, 3), (9, 8), (15, 1), (16, 2), (17, 3)):
    LATTICE_SPECS["small_m%d_v%d" % (_m, _V)] = dict(V=_V, HW=(5, 9), dhw=VOLS_A if _m % 2 else VOLS_B, order=list(range(40, 40 + _m)), gran=16)
LATTICE_NAMES = tuple(LATTICE_SPECS)

# derived coordinates: S swept, n * S never a multiple of 256, the last two with per-ray near / far ranges
DERIVED_SPECS = {"derived_S%d%s" % (S, "_ranges" if pr else ""): dict(n=n, S=S, V=V, per_ray=pr)
                 for S, n, V, pr in ((1, 37, 1, False), (2, 37, 2, False), (3, 21, 3, True), (5, 13, 2, False), (30, 7, 8, False), (90, 5, 2, True),
                                     (192, 3, 1, False))}
DERIVED_NAMES = tuple(DERIVED_SPECS)


@functools.lru_cache(maxsize=None)
def lattice(name):
    """(case, float64 feats, float64 grads) of a lattice or derived case, built and checked once per process."""
    if name in LATTICE_SPECS:
        case = lattice_case(name, seed=LATTICE_NAMES.index(name), **LATTICE_SPECS[name])
    else:
        case = derived_case(name, seed=100 + DERIVED_NAMES.index(name), **DERIVED_SPECS[name])
    feats, grads = check_lattice(case)
    return case, feats, grads


def lattice_state_dict(V):
    """The network the gather-fused route is compared on.  The lattice features are integers up to 8 where a live scene's are of order 1, and the
    two bias nets multiply the trunk at every layer: with unscaled weights |sigma| reaches 5e5 on these scenes and the float32 ORACLE is 0.3 away
    from the float64 one -- nothing can be read off a render then.  Their first layers are divided by 8, which gives the bias nets the inputs
    they see on a live scene: sigma of order 1, float32 oracle within 2e-6 of float64 (asserted on the CPU,
    test_gather_cases_host.py), a fifth of the tightest bar the device comparison uses."""
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    sd = init_ucnerf_state_dict(seed=5, n_src=V, sigma_scale=0.1, sigma_bias=0.02)
    for k in ("nerf.pts_bias_depth_fine.weight", "nerf.pts_bias_confidence.weight"):
        sd[k] = sd[k] / 8
    return sd


# ------------------------------------------------------------------------------------------------ the continuous cases
CONTINUOUS_SPECS = {
    "cont_v3_quarter": dict(V=3, HW=(12, 20), dhw=[(5, 3, 5), (3, 6, 10), (2, 12, 20)], m=1500, wild=False),
    "cont_v6_wild": dict(V=6, HW=(16, 12), dhw=[(1, 2, 3), (3, 5, 2), (8, 3, 5)], m=1111, wild=True),
    "cont_v1_wild_m257": dict(V=1, HW=(9, 7), dhw=[(7, 1, 2), (1, 8, 3), (2, 3, 1)], m=257, wild=True),
    "cont_v8_half": dict(V=8, HW=(8, 12), dhw=[(3, 2, 3), (4, 4, 6), (1, 8, 12)], m=700, wild=False),
}
CONTINUOUS_NAMES = tuple(CONTINUOUS_SPECS)
EDGE_EPS, PLANE_EPS, EXCLUDED_CAP = 1e-4, 1e-2, 0.02


def continuous_case(name, V, HW, dhw, m, wild, seed):
    from fuzz_render import pose
    H, W = HW
    rng = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    ar, at = (0.5, 0.5) if wild else (0.08, 0.08)
    fx = float(rng.uniform(0.6, 1.6)) * W
    K = torch.tensor([[fx, 0, W / 2.0 + rng.uniform(-1, 1)], [0, fx * rng.uniform(0.9, 1.1), H / 2.0 + rng.uniform(-1, 1)], [0, 0, 1]], dtype=torch.float32)
    intr = K.repeat(V, 1, 1).clone()
    intr[:, 0, 0] *= torch.tensor(rng.uniform(0.9, 1.1, V), dtype=torch.float32)
    w2cs = torch.stack([pose(rng, ar, at) for _ in range(V)])
    rn = lambda *s: torch.randn(*s, generator=gen)       # noqa: E731
    pts = torch.rand(m, 1, 3, generator=gen) * torch.tensor([3.0, 3.0, 8.0]) - torch.tensor([1.5, 1.5, 3.0])      # depth -3 .. 5: a third behind
    case = dict(name=name, kind="continuous", V=V, H=H, W=W, dhw=[tuple(s) for s in dhw], m=m, w2cs=w2cs.double(), intrinsics=intr.double(),
                vols=[rn(1, 8, *s).double() for s in dhw], confidence=torch.rand(H, W, generator=gen).double(),
                imgs=torch.rand(1, V, 3, H, W, generator=gen).double(), img_feat=rn(V, 1, 8, H, W).double(), pts=pts.double())
    for s in range(3):
        case["stage%d" % (s + 1)] = (torch.rand(m, 1, 3, generator=gen) * 1.6 - 0.3).double()
    # (every input is a float32 value held in float64: the device and both oracles see the same numbers)
    v = geometry(case)["view"]
    near_edge = ((v["gx"].abs() - 1).abs() < EDGE_EPS) | ((v["gy"].abs() - 1).abs() < EDGE_EPS)        # [V,m]
    near_plane = v["cz"].abs() < PLANE_EPS
    case["skip_mask"], case["skip_view"] = (near_edge | near_plane).T.contiguous(), near_plane.T.contiguous()      # [m,V]
    case["skip_feats"] = case["skip_mask"]
    share = case["skip_mask"].double().mean().item()
    assert share <= EXCLUDED_CAP, "%s: %.2f %% of the (sample, view) pairs excluded" % (name, 100 * share)
    case["excluded_share"] = share
    case["census"] = dict(behind=int((v["cz"] < 0).sum()), front=int((v["cz"] > 0).sum()), outside=int(((v["gx"].abs() > 1) | (v["gy"].abs() > 1)).sum()))
    g = rn(m, 1, 24 + 12 * V + 1)
    F = g.shape[-1]
    for vi in range(V):                                        # an excluded (sample, view) pair takes no part in the gradients either
        g[case["skip_feats"][:, vi], 0, 24 + 4 * V + 8 * vi:24 + 4 * V + 8 * vi + 8] = 0
    assert F == 24 + 12 * V + 1
    case["g_feats"] = g.double()
    return case


def keep_columns(case):
    """[m,F] bool: the feature entries of a continuous case that are compared."""
    V, m = case["V"], case["m"]
    keep = torch.ones(m, 24 + 12 * V + 1, dtype=torch.bool)
    for v in range(V):
        keep[:, 24 + 4 * v + 3] &= ~case["skip_mask"][:, v]
        for c in list(range(24 + 4 * v, 24 + 4 * v + 3)) + list(range(24 + 4 * V + 8 * v, 24 + 4 * V + 8 * v + 8)):
            keep[:, c] &= ~case["skip_feats"][:, v]
    return keep


def distances(case, ref_feats, ref_grads, feats, grads):
    """Max distance from the float64 reference per column group and gradient tensor (compared entries only); in-mask bits -> number unequal."""
    keep = keep_columns(case)
    d = ((feats.double().reshape(case["m"], -1) - ref_feats.reshape(case["m"], -1)).abs() * keep)
    cols = columns(case["V"])
    out = {k: d[:, cols[k]].max().item() for k in ("volumes", "colours", "view_feats", "confidence")}
    out["mask_flips"] = int((d[:, cols["mask"]] != 0).sum())
    for k in GRADS:
        if grads.get(k) is not None:
            out[k] = (grads[k].double().reshape(-1) - ref_grads[k].reshape(-1)).abs().max().item()
    return out


def scales(case, ref_feats, ref_grads):
    cols = columns(case["V"])
    f = ref_feats.reshape(case["m"], -1)
    out = {k: f[:, cols[k]].abs().max().item() for k in ("volumes", "colours", "view_feats", "confidence")}
    out.update({k: ref_grads[k].abs().max().item() for k in GRADS})
    return out


@functools.lru_cache(maxsize=None)
def continuous(name, bf16_sources=False):
    """(case, float64 feats, float64 grads, the float32 oracle's own distances, max|reference| per group), built once per process."""
    case = continuous_case(name, seed=1000 + CONTINUOUS_NAMES.index(name), **CONTINUOUS_SPECS[name])
    feats, grads = reference(case, bf16_sources=bf16_sources)
    f32, g32 = reference(case, torch.float32, bf16_sources=bf16_sources)
    return case, feats, grads, distances(case, feats, grads, f32, g32), scales(case, feats, grads)


def bar(oracle_distance, scale):
    """What the device may differ from the float64 reference by: 4 x the float32 oracle's own distance (another, equally legitimate summation
    order and fused multiply-adds) + 1e-6 of the group's largest reference value."""
    return 4.0 * oracle_distance + 1e-6 * scale
