"""Non-finite depths, logits, features and upstream gradients for the MVS stage kernels (csrc/mvs.hip): the cases and their CPU reference, shared by
tests/test_mvs_nonfinite_host.py (which proves on the CPU that the cases are what they claim) and tests/test_hip_mvs_nonfinite.py (which runs the
kernels on them).  Every case is a CLEAN input of tests/mvs_cases.py's builders plus one POISON (kind x site); what is expected of the device is what
torch's own ops give on the CPU, in float32 (the pattern: where NaN, +inf and -inf land) and in float64 (the finite values).

THE REFERENCE.  cost volume: oracle.mvs_oracle.cost_volume_variance with F.grid_sample(nearest, border, align_corners=True) -- the op the reference
calls, utils/utils.py:1160 -- in the place of the oracle's sample_nearest_border, whose .long() of a NaN is no index (`cv_restatement`; the host test
holds the two to each other on the clean cases).  torch's CPU grid_sample sends a NaN coordinate to index 0 and +-inf to the clamped ends, each axis
on its own; `cv_index` / `cv_explicit` spell that rule out as index arithmetic, the second witness and the source of the predicted sets.
depth regression: oracle.mvs_oracle.depth_regress as it stands (`dr_restatement`), with autograd for the three backward kernels.  Its .long() of a NaN
expectation is the most negative integer on the CPUs this suite runs on, which clamp(0, D - 1) makes 0: the window of a NaN pixel is the first one.

COST-VOLUME CLEAN INPUTS.  The exact lattice of mvs_cases (integer features, dyadic coordinates), H x W = 5 x 9, D = 9: with pad 1 the padded plane
has 7 x 11 x 9 = 693 voxels, no multiple of 32 or 256.  A poisoned depth keeps the lattice: +-inf makes T / depth = +-0, a negative depth is -1, the
smallest denormal makes T / depth +-inf in float32 and +-7e44 in float64 -- the same clamped end --, NaN and +-0 make every coordinate NaN
(0 / 0 in the homogeneous row, whose T entry is 0 on the lattice; view 6 has T = 0 in all three rows).

DEPTH-REGRESSION CLEAN INPUTS.  Random logits and depth values as the continuous cases of mvs_cases draw them (the lattice's -200 logits are exactly 0
after exp in float32 and 1.4e-87 in float64: 0 * inf against 1.4e-87 * inf would have no single right answer), planes 5 x 9 (pad 0) and 7 x 11
(pad 1): two and three blocks of 32 pixels, the last one partial.

Our own code; nothing here is needed by the package."""
import functools

import torch
import torch.nn.functional as F

import mvs_cases as G
from oracle import mvs_oracle as M

F64, F32 = G.F64, G.F32
NAN, INF = float("nan"), float("inf")
DENORMAL = 2.0 ** -149                                  # float32's smallest
HW, CV_D = (5, 9), 9


def classes(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, per element."""
    return torch.isnan(t).long() + 2 * torch.isposinf(t).long() + 3 * torch.isneginf(t).long()


def changed(a, b):
    """Elements of `a` that are not `b`'s: another value, or NaN on one side only."""
    return ~((a == b) | (torch.isnan(a) & torch.isnan(b)))


# ------------------------------------------------------------------------------------------------ cost volume: the reference
def cv_restatement(case, dtype=F64):
    """-> dict(variance [C,D,Hp,Wp], count [D,Hp,Wp], g_feats [V,C,H,W]) in `dtype`."""
    feats = case["feats"].to(dtype).clone().requires_grad_(True)
    proj, dv, pad = case["proj"].to(dtype), case["depth_values"].to(dtype), case["pad"]
    V, C, H, W = feats.shape
    D, Hp, Wp = dv.shape
    vsum = torch.zeros(C, D, Hp * Wp, dtype=dtype)
    vsq = torch.zeros_like(vsum)
    msum = torch.ones(D, Hp * Wp, dtype=dtype)
    for i in range(V):
        grid = M.homo_warp_grid(proj[i], dv, H, W, pad)
        warped = F.grid_sample(feats[i][None], grid[None], mode="nearest", padding_mode="border", align_corners=True)[0]
        inside = ((grid > -1.0) * (grid < 1.0))
        msum = msum + (inside[..., 0] * inside[..., 1]).to(dtype)
        vsum = vsum + warped
        vsq = vsq + warped ** 2
    count = 1.0 / msum
    var = (vsq * count - (vsum * count) ** 2).reshape(C, D, Hp, Wp)
    var.backward(case["g_variance"].to(dtype))
    return dict(variance=var.detach(), count=count.reshape(D, Hp, Wp), g_feats=feats.grad.detach())


def cv_index(case, dtype=F64):
    """The source pixel of every voxel per view, [V, D*plane], by the rule spelled out: unnormalise, NaN -> 0, clip, round half to even; and the mask."""
    H, W, pad = case["H"], case["W"], case["pad"]
    dv = case["depth_values"].to(dtype)
    idx, inside = [], []
    for v in range(case["V"]):
        g = M.homo_warp_grid(case["proj"][v].to(dtype), dv, H, W, pad).reshape(-1, 2)
        ix, iy = ((g[:, 0] + 1) / 2) * (W - 1), ((g[:, 1] + 1) / 2) * (H - 1)
        ix = torch.where(torch.isnan(ix), torch.zeros_like(ix), ix).clamp(0, W - 1).round().long()
        iy = torch.where(torch.isnan(iy), torch.zeros_like(iy), iy).clamp(0, H - 1).round().long()
        idx.append(iy * W + ix)
        inside.append((g[:, 0] > -1) & (g[:, 0] < 1) & (g[:, 1] > -1) & (g[:, 1] < 1))
    return torch.stack(idx), torch.stack(inside)


def cv_explicit(case, dtype=F64):
    """variance and count from cv_index and a plain gather: the geometry's own prediction of the forward."""
    idx, inside = cv_index(case, dtype)
    feats = case["feats"].to(dtype)
    V, C, H, W = feats.shape
    D, Hp, Wp = case["depth_values"].shape
    vsum = torch.zeros(C, D * Hp * Wp, dtype=dtype)
    vsq = torch.zeros_like(vsum)
    for i in range(V):
        w = feats[i].reshape(C, H * W)[:, idx[i]]
        vsum = vsum + w
        vsq = vsq + w ** 2
    count = 1.0 / (1 + inside.sum(0).to(dtype))
    return dict(variance=(vsq * count - (vsum * count) ** 2).reshape(C, D, Hp, Wp), count=count.reshape(D, Hp, Wp))


# ------------------------------------------------------------------------------------------------ cost volume: the cases
CV_LAYOUTS = {                                          # narrow: cost_volume_narrow_kernel (C <= 16); wide: cost_volume_wide_kernel, V = 8 uses every projecting lane
    "narrow_v1": dict(views=[0], C=3),
    "narrow_v3": dict(views=[0, 6, 1], C=3),
    "wide_v3": dict(views=[2, 3, 5], C=17),
    "wide_v8": dict(views=[0, 1, 2, 3, 4, 6, 7, 8], C=17),
}
CV_KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF, "+0": 0.0, "-0": -0.0, "negative": -1.0, "denormal": DENORMAL}
CV_SITES = ("voxel0", "last_voxel", "border_voxel", "plane", "column")
FEAT_KINDS = {"nan": NAN, "+inf": INF}
FEAT_PIXELS = {"pixel0": 0, "middle": 2 * HW[1] + 4}
GRAD_KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF}


@functools.lru_cache(maxsize=None)
def cv_clean(layout, pad):
    spec = CV_LAYOUTS[layout]
    case = G.cv_lattice_case("%s_pad%d" % (layout, pad), spec["views"], spec["C"], HW, CV_D, pad, seed=7100 + 2 * list(CV_LAYOUTS).index(layout) + pad)
    G.check_cv_lattice(case)
    return case


def cv_site(site, pad):
    """[D,Hp,Wp] bool: the voxels of a poison site."""
    Hp, Wp = HW[0] + 2 * pad, HW[1] + 2 * pad
    m = torch.zeros(CV_D, Hp, Wp, dtype=torch.bool)
    if site == "voxel0":
        m[0, 0, 0] = True
    elif site == "last_voxel":                          # the voxel the wide kernel's ghost lanes (t >= total) copy
        m[-1, -1, -1] = True
    elif site == "border_voxel":
        assert pad > 0
        m[4, 0, 5] = True
    elif site == "plane":
        m[3] = True
    elif site == "column":
        m[:, pad + 2, pad + 4] = True
    else:
        raise KeyError(site)
    return m


def _cv_poisoned(base, name, **over):
    case = dict(base, name=name, clean=base, **over)
    return case


def cv_depth_case(layout, pad, kind, site):
    """One kind of poison in depth_values at one site.  predicted: the site's voxels."""
    base = cv_clean(layout, pad)
    m = cv_site(site, pad)
    dv = base["depth_values"].clone()
    dv[m] = CV_KINDS[kind]
    return _cv_poisoned(base, "cv/%s_pad%d/depth_%s/%s" % (layout, pad, kind, site), depth_values=dv, poison=("depth", kind, site), voxels=m)


def cv_feat_case(layout, pad, kind, pixel):
    """NaN or +inf at one source pixel of one view and one channel.  The clean side already has a NaN depth plane, so every view sends a whole
    plane of NaN coordinates to pixel 0.  predicted: the voxels whose lookup in that view lands on the pixel, in that channel."""
    plane = cv_depth_case(layout, pad, "nan", "plane")
    base = dict(plane, name=plane["name"] + " (clean side)")
    del base["clean"]
    view, ch = min(base["V"] - 1, 2), base["C"] - 1
    feats = base["feats"].clone()
    feats[view, ch].view(-1)[FEAT_PIXELS[pixel]] = FEAT_KINDS[kind]
    case = _cv_poisoned(base, "cv/%s_pad%d/feats_%s/%s" % (layout, pad, kind, pixel), feats=feats, poison=("feats", kind, pixel), view=view, channel=ch,
                        pixel=FEAT_PIXELS[pixel])
    idx, _ = cv_index(case)
    case["voxels"] = (idx[view] == FEAT_PIXELS[pixel]).reshape(base["depth_values"].shape)
    return case


def cv_grad_case(layout, pad, kind):
    """Clean inputs, one NaN or inf in g_variance (last channel, a voxel of the middle plane)."""
    base = cv_clean(layout, pad)
    g = base["g_variance"].clone()
    m = torch.zeros(base["depth_values"].shape, dtype=torch.bool)
    m[4, pad + 1, pad + 3] = True
    g[-1][m] = GRAD_KINDS[kind]
    return _cv_poisoned(base, "cv/%s_pad%d/g_variance_%s" % (layout, pad, kind), g_variance=g, poison=("g_variance", kind, "voxel"), voxels=m,
                        channel=base["C"] - 1)


def _cv_specs():
    out = {}
    narrow, wide = ("narrow_v1", "narrow_v3"), ("wide_v3", "wide_v8")
    # One voxel in a corner of the plane is seen by no view of narrow_v1 (count 1, variance 0 wherever it looks): the single-voxel sites go to the
    # layouts and pads on which they move an output -- the host test asserts that every case's poison is visible.
    single_pad = {"voxel0": 0, "last_voxel": 1, "border_voxel": 1}
    k = 0
    for kind in CV_KINDS:
        for site in CV_SITES:
            for family in (narrow, wide):                # every (kind, site) pair on both layouts; V and pad rotate
                layout, pad = family[k % 2], (k // 2) % 2
                if site in single_pad:
                    layout = "narrow_v3" if family is narrow else layout
                    pad = single_pad[site] if layout != "wide_v8" or site == "border_voxel" else pad
                out["cv/%s_pad%d/depth_%s/%s" % (layout, pad, kind, site)] = (cv_depth_case, (layout, pad, kind, site))
            k += 1
    for i, layout in enumerate(CV_LAYOUTS):
        for kind in FEAT_KINDS:
            for pixel in FEAT_PIXELS:
                out["cv/%s_pad%d/feats_%s/%s" % (layout, i % 2, kind, pixel)] = (cv_feat_case, (layout, i % 2, kind, pixel))
        for j, kind in enumerate(("nan", "+inf")):
            out["cv/%s_pad%d/g_variance_%s" % (layout, (i + j) % 2, kind)] = (cv_grad_case, (layout, (i + j) % 2, kind))
    return out


CV_SPECS = _cv_specs()
REFUSED_SIZES = {"W1": ((5, 1), r"cost_volume: bad sizes C=3 H=5 W=1 D=9 pad=0"), "H1": ((1, 9), r"cost_volume: bad sizes C=3 H=1 W=9 D=9 pad=0")}


def cv_predicted(case):
    """{output: bool mask} -- where a poisoned case may differ from its clean side."""
    base = case["clean"]
    C = case["C"]
    vox = case["voxels"]
    what = case["poison"][0]
    var = torch.zeros(C, *vox.shape, dtype=torch.bool)
    cells = torch.zeros(case["feats"].shape, dtype=torch.bool).reshape(case["V"], C, -1)
    hit = vox.reshape(-1)
    channels = range(C) if what == "depth" else [case["channel"]]
    for src in (base, case):
        idx, _ = cv_index(src)
        for i in range(case["V"]):
            for c in channels:
                cells[i, c, idx[i][hit]] = True
    if what == "depth":
        var[:] = vox
        count = vox.clone()
    else:
        count = torch.zeros_like(vox)
        if what == "feats":
            var[case["channel"]] = vox
    return dict(variance=var, count=count, g_feats=cells.reshape(case["feats"].shape))


@functools.lru_cache(maxsize=None)
def cv_case(name):
    """(case, float64 restatement, float32 restatement, predicted sets), built once per process."""
    fn, args = CV_SPECS[name]
    case = fn(*args)
    assert case["name"] == name
    return case, cv_restatement(case, F64), cv_restatement(case, F32), cv_predicted(case)


_CV_CLEAN = {}


def cv_clean_reference(case):
    """(float64, float32) restatement of the case's clean side, computed once per clean side and process."""
    base = case["clean"]
    if base["name"] not in _CV_CLEAN:
        _CV_CLEAN[base["name"]] = (cv_restatement(base, F64), cv_restatement(base, F32))
    return _CV_CLEAN[base["name"]]


# ------------------------------------------------------------------------------------------------ depth regression: the reference
DR_FWD = ("prob_volume", "depth", "confidence")
DR_BWD = ("g_prob_pre", "g_depth_values")
DR_OUTPUTS = DR_FWD + DR_BWD


def dr_restatement(case, dtype=F64):
    """depth_regress in `dtype` with autograd -> dict of DR_OUTPUTS (g_prob_init is g_prob_pre: the logits are their sum)."""
    x = case["prob_pre"].to(dtype).clone().requires_grad_(True)
    dv = case["depth_values"].to(dtype).clone().requires_grad_(True)
    init = None if case["prob_init"] is None else case["prob_init"].to(dtype)
    p, depth, conf = M.depth_regress(x, dv, init, case["pad"])
    g_x, g_dv = torch.autograd.grad([depth, conf], [x, dv], [case["g_depth"].to(dtype), case["g_confidence"].to(dtype)])
    return dict(prob_volume=p.detach(), depth=depth.detach(), confidence=conf.detach(), g_prob_pre=g_x, g_depth_values=g_dv)


# ------------------------------------------------------------------------------------------------ depth regression: the cases
DR_SHAPES = {                                           # D: a depth lane owns 1, 2 or 3 depths; D = 4 is the whole confidence window
    "d4_pad0": (4, 0, False), "d9_pad0": (9, 0, True), "d17_pad0": (17, 0, False),
    "d4_pad1": (4, 1, True), "d9_pad1": (9, 1, False), "d17_pad1": (17, 1, True),
}
DR_KINDS = ("nan", "+inf", "-inf", "-inf_all")
DR_DEPTH_SITES = ("d0", "d8", "d_last")
DR_PIXEL_SITES = ("pixel0", "last_live_pixel", "border_pixel", "first_inner_pixel")
DV_KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF}


@functools.lru_cache(maxsize=None)
def dr_clean(shape):
    D, pad, init = DR_SHAPES[shape]
    Hp, Wp = HW[0] + 2 * pad, HW[1] + 2 * pad
    g = torch.Generator().manual_seed(7300 + list(DR_SHAPES).index(shape))
    r = lambda *s: torch.randn(*s, generator=g).double()        # noqa: E731   (float32 numbers held in float64)
    dv = (1.0 + torch.linspace(0, 2.0, D).view(D, 1, 1) + 0.05 * torch.rand(D, Hp, Wp, generator=g)).double()
    return dict(name="dr/" + shape, D=D, Hp=Hp, Wp=Wp, pad=pad, prob_pre=r(D, Hp, Wp), prob_init=r(D, Hp, Wp) if init else None, depth_values=dv,
                g_depth=r(*HW), g_confidence=r(*HW))


def dr_pixel(site, pad):
    """(y, x) in the padded plane."""
    Hp, Wp = HW[0] + 2 * pad, HW[1] + 2 * pad
    if site == "pixel0":
        return 0, 0
    if site == "last_live_pixel":                       # pixel plane - 1: the one the second block's dead lanes copy
        return Hp - 1, Wp - 1
    if site == "border_pixel":
        assert pad > 0
        return 2, 0
    if site == "first_inner_pixel":                     # next to the pad border
        assert pad > 0
        return pad, pad
    raise KeyError(site)


def _row(base, y, x):
    m = torch.zeros(base["Hp"], base["Wp"], dtype=torch.bool)
    m[y, x] = True
    return m


def dr_logit_case(shape, kind, depth_site, pixel_site, target):
    base = dr_clean(shape)
    D, pad = base["D"], base["pad"]
    y, x = dr_pixel(pixel_site, pad)
    t = base[target].clone()
    if kind == "-inf_all":
        t[:, y, x] = -INF
    else:
        d = {"d0": 0, "d8": 8, "d_last": D - 1}[depth_site]
        t[d, y, x] = {"nan": NAN, "+inf": INF, "-inf": -INF}[kind]
    name = "dr/%s/%s_%s/%s/%s" % (shape, target, kind, depth_site, pixel_site)
    return dict(base, name=name, clean=base, poison=("logits", kind, depth_site, pixel_site), pixels=_row(base, y, x), **{target: t})


def dr_values_case(shape, kind):
    """NaN or inf in depth_values at one depth of one kept pixel: depth is non-finite there, prob_volume and confidence do not move."""
    base = dr_clean(shape)
    y, x = base["pad"] + 2, base["pad"] + 4
    dv = base["depth_values"].clone()
    dv[base["D"] // 2, y, x] = DV_KINDS[kind]
    return dict(base, name="dr/%s/depth_values_%s" % (shape, kind), clean=base, poison=("depth_values", kind), pixels=_row(base, y, x), depth_values=dv)


def dr_grad_case(shape, which, kind, inner_yx):
    """Clean inputs, one NaN or inf in g_depth or g_confidence at the kept pixel inner_yx."""
    base = dr_clean(shape)
    g = base[which].clone()
    g[inner_yx] = GRAD_KINDS[kind]
    return dict(base, name="dr/%s/%s_%s" % (shape, which, kind), clean=base, poison=(which, kind),
                pixels=_row(base, inner_yx[0] + base["pad"], inner_yx[1] + base["pad"]), **{which: g})


def _dr_specs():
    out = {}
    k = 0
    for shape, (D, pad, init) in DR_SHAPES.items():
        depth_sites = [s for s in DR_DEPTH_SITES if s != "d8" or D > 8]
        pixel_sites = [s for s in DR_PIXEL_SITES if pad > 0 or s in ("pixel0", "last_live_pixel")]
        for kind in DR_KINDS:
            for pixel_site in pixel_sites:
                depth_site = "all" if kind == "-inf_all" else depth_sites[k % len(depth_sites)]
                target = "prob_init" if init and k % 2 else "prob_pre"
                out["dr/%s/%s_%s/%s/%s" % (shape, target, kind, depth_site, pixel_site)] = (dr_logit_case, (shape, kind, depth_site, pixel_site, target))
                k += 1
    for shape in ("d9_pad0", "d17_pad1"):
        for kind in DV_KINDS:
            out["dr/%s/depth_values_%s" % (shape, kind)] = (dr_values_case, (shape, kind))
    for shape, yx in (("d9_pad0", (2, 4)), ("d17_pad1", (0, 0)), ("d4_pad1", (4, 8))):       # (0, 0) and (4, 8) of a padded plane: next to the pad border
        for kind in ("nan", "+inf"):
            out["dr/%s/g_depth_%s" % (shape, kind)] = (dr_grad_case, (shape, "g_depth", kind, yx))
    for shape, yx in (("d4_pad0", (2, 4)), ("d9_pad1", (2, 4))):          # pixels whose window sum is well below 1: the clamp's gradient switch is no coin toss
        for kind in GRAD_KINDS:
            out["dr/%s/g_confidence_%s" % (shape, kind)] = (dr_grad_case, (shape, "g_confidence", kind, yx))
    return out


DR_SPECS = _dr_specs()


def dr_predicted(case):
    """{output: bool mask} -- where a poisoned case may differ from its clean side."""
    D, pad, Hp, Wp = case["D"], case["pad"], case["Hp"], case["Wp"]
    px = case["pixels"]
    rows = px[None].expand(D, Hp, Wp).clone()
    inner = px[pad:Hp - pad, pad:Wp - pad].clone()
    none3, none2 = torch.zeros_like(rows), torch.zeros_like(inner)
    what = case["poison"][0]
    if what == "logits":
        return dict(prob_volume=rows, depth=inner, confidence=inner, g_prob_pre=rows, g_depth_values=rows)
    if what == "depth_values":
        return dict(prob_volume=none3, depth=inner, confidence=none2, g_prob_pre=rows, g_depth_values=none3)
    if what == "g_depth":
        return dict(prob_volume=none3, depth=none2, confidence=none2, g_prob_pre=rows, g_depth_values=rows)
    if what == "g_confidence":
        return dict(prob_volume=none3, depth=none2, confidence=none2, g_prob_pre=rows, g_depth_values=none3)
    raise KeyError(what)


@functools.lru_cache(maxsize=None)
def dr_case(name):
    """(case, float64 restatement, float32 restatement, predicted sets), built once per process."""
    fn, args = DR_SPECS[name]
    case = fn(*args)
    assert case["name"] == name
    return case, dr_restatement(case, F64), dr_restatement(case, F32), dr_predicted(case)


@functools.lru_cache(maxsize=None)
def dr_clean_reference(shape):
    base = dr_clean(shape)
    return dr_restatement(base, F64), dr_restatement(base, F32)


# ------------------------------------------------------------------------------------------------ the removal rule
def patterns_agree(r64, r32):
    """The outputs on which the float32 and the float64 restatement put NaN, +inf and -inf at other positions (empty: the case has one right answer)."""
    return [k for k in r64 if not torch.equal(classes(r64[k]), classes(r32[k]))]


# Cases whose float32 and float64 restatements disagree on a non-finite position have no single right answer; tests/test_mvs_nonfinite_host.py
# asserts that this list is exactly those, and that every (kind, site) pair survives without them.
REMOVED = ()
CV_NAMES = tuple(n for n in CV_SPECS if n not in REMOVED)
DR_NAMES = tuple(n for n in DR_SPECS if n not in REMOVED)


def finite_bar(r64, r32, inside):
    """The rule of mvs_cases.bar on the finite elements of `inside`: (bar, the float32 restatement's own distance, elements compared)."""
    keep = inside & torch.isfinite(r64) & torch.isfinite(r32.double())
    if not bool(keep.any()):
        return 0.0, 0.0, keep
    own = (r32.double() - r64)[keep].abs().max().item()
    scale = r64[torch.isfinite(r64)].abs().max().item()
    return G.bar(own, scale), own, keep
