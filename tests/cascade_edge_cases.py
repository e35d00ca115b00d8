"""Cases and the reference for the FORWARD of the cascade link (ucnerf_depth_hypotheses, map and row mode), shared by
tests/test_cascade_edges_host.py (which proves on the CPU that the cases are what they claim) and tests/test_hip_cascade_edges.py (which runs the
kernel on them).  CPU only; imports neither the package nor oracle/.

The reference is `chain`: the op chain written out from the formulas of include/ucnerf_hip.h (the ucnerf_depth_hypotheses comment) in a chosen
dtype -- bilinear up-sampling under the align_corners=False source rule, the two clamps (torch.clamp: NaN propagates), lo + d * (hi - lo) / (D - 1),
bilinear down-sampling, replicate padding.  float64 is the yardstick; cascade_stubs.hypotheses_chain (float32 torch ops, pinned to fixture G19) is
the cross-check, and the host test holds the two to each other within cascade_stubs.bar(far).

  LATTICE   every intermediate is a dyadic number float32 holds exactly (size ratios powers of two, cur_depth in multiples of 2^-6, near / far /
            half dyadic, D - 1 a power of two): any summation order and any contraction give the same bits, the device is held with torch.equal
  FOOTPRINT k = 0 and clamps that cannot bind: every plane is the composed bilinear map of cur_depth; one-hot inputs read the taps out
  CONTINUOUS the five map cases of tests/test_hip_cascade.py and three more, against float64 within cascade_stubs.bar(far)
  NONFINITE one NaN, one +inf and one -inf pixel in cur_depth

Our own code; nothing here is needed by the package.
"""
import torch
import torch.nn.functional as F

import cascade_stubs as S
from test_hip_cascade import FAR as C_FAR, MAP_CASES, NEAR as C_NEAR


# ------------------------------------------------------------------------------------------------ the reference
def taps(n_in, n_out, dtype):
    """One axis of torch's align_corners=False rule: src = max(scale * (dst + 0.5) - 0.5, 0), scale = n_in / n_out formed in `dtype`;
    -> (i0, i1, l0, l1): taps floor(src) and min(floor(src) + 1, n_in - 1), weights 1 - l and l."""
    scale = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    src = (scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def resize(x, out_hw):
    """Bilinear resize of the last two axes of x, every tap computed (a zero weight still multiplies its tap, as torch's kernels do)."""
    y0, y1, ly0, ly1 = taps(x.shape[-2], int(out_hw[0]), x.dtype)
    x0, x1, lx0, lx1 = taps(x.shape[-1], int(out_hw[1]), x.dtype)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    top, bottom = x[..., y0, :], x[..., y1, :]
    return ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bottom[..., x0] + lx1 * bottom[..., x1])


def chain(cur, near, far, interval_pixel, D, HW, hw, pad=0, dtype=torch.float64):
    """cur [h0, w0] -> dict(c, lo, hi, step [H, W]; samples [D, H, W]; out [D, h + 2 pad, w + 2 pad]; half) in `dtype` on the CPU."""
    cur = cur.to(dtype)
    near, far = torch.as_tensor(near, dtype=dtype), torch.as_tensor(far, dtype=dtype)
    half = torch.as_tensor(D / 2, dtype=dtype) * torch.as_tensor(interval_pixel, dtype=dtype)
    c = resize(cur, HW)
    lo = torch.clamp(c - half, min=near)
    hi = torch.clamp(c + half, max=far)
    step = (hi - lo) / (D - 1)
    samples = lo[None] + torch.arange(D, dtype=dtype).reshape(-1, 1, 1) * step[None]
    planes = resize(samples, hw)
    # the depth axis of the reference's trilinear interpolation keeps its size: taps d and min(d + 1, D - 1) with the weights 1 and 0 -- the same
    # values wherever plane d + 1 is finite, NaN where it is not (0 * inf)
    out = 1 * planes + 0 * planes[(torch.arange(D) + 1).clamp(max=D - 1)]
    if pad > 0:
        out = F.pad(out[None], (pad,) * 4, "replicate")[0]
    return {"c": c, "lo": lo, "hi": hi, "step": step, "samples": samples, "out": out, "half": half}


def row_chain(row, D, hw, pad=0, dtype=torch.float64):
    row = row.to(dtype)
    step = (row[-1] - row[0]) / (D - 1)
    s = row[0] + torch.arange(D, dtype=dtype) * step
    return s.reshape(-1, 1, 1).repeat(1, int(hw[0]) + 2 * pad, int(hw[1]) + 2 * pad)


def interval_pixel_of(c):
    """What the case's (k, interval, near, far) mean, in exact arithmetic on python floats: k * interval, or k * (far - near)."""
    return c["k"] * (c["interval"] if c["interval"] is not None else c["far"] - c["near"])


def reference(c, dtype=torch.float64, **over):
    c = dict(c, **over)
    return chain(c["cur"], c["near"], c["far"], interval_pixel_of(c), c["D"], c["HW"], c["hw"], c["pad"], dtype)


def stub_chain(c, **over):
    """The float32 torch op chain (cascade_stubs.hypotheses_chain) on the case: the cross-check and the second witness."""
    c = dict(c, **over)
    ip = torch.tensor(c["k"]) * (torch.tensor(c["interval"]) if c["interval"] is not None else torch.tensor(c["far"]) - torch.tensor(c["near"]))
    return S.hypotheses_chain(c["cur"].float(), torch.tensor(c["near"]), torch.tensor(c["far"]), ip, c["D"], c["HW"], c["hw"], c["pad"])[0]


def _case(name, cur, near, far, k, interval, D, HW, hw, pad):
    return {"name": name, "cur": cur.float(), "near": float(near), "far": float(far), "k": float(k), "interval": interval, "D": D, "HW": tuple(HW),
            "hw": tuple(hw), "pad": pad}


# ------------------------------------------------------------------------------------------------ A: the exact lattice
# name: cur (h0, w0), full (H, W), out (h, w), D, pad, (near, far), k, interval   (interval_pixel = k * interval, half = D / 2 * interval_pixel)
LATTICE = {
    "up4_down2_D5": ((4, 5), (16, 20), (8, 10), 5, 0, (2.0, 10.0), 0.25, 4.0),                 # half 2.5
    "two_blocks_up4_down2_D9_pad1": ((8, 10), (32, 40), (16, 20), 9, 1, (2.0, 10.0), 0.125, 4.0),   # half 2.25; the padded plane has 18 * 22 = 396 pixels
    "up2_down2_D17_pad1": ((6, 7), (12, 14), (6, 7), 17, 1, (1.0, 3.0), 0.0625, 1.0),          # half 0.53125; three depth chunks, the last of one plane
    "up_only_D9_pad3": ((4, 4), (8, 8), (8, 8), 9, 3, (2.0, 6.0), 0.25, 1.0),                  # h == H; half 1.125
    "down_only_D3_pad3_wider_than_h": ((8, 8), (8, 8), (2, 4), 3, 3, (2.0, 6.0), 0.5, 1.0),    # h0 == H; half 0.75; pad 3 > h = 2
    "all_identity_D2_pad1": ((5, 6), (5, 6), (5, 6), 2, 1, (2.0, 6.0), 1.0, 1.0),              # neither; half 1
    "one_pixel_map_D5": ((1, 1), (4, 4), (2, 2), 5, 0, (2.0, 6.0), 0.25, 1.0),                 # h0 = w0 = 1: every up-sampling tap clamps
    "h0_is_1_D3": ((1, 8), (4, 16), (2, 8), 3, 0, (2.0, 6.0), 0.5, 1.0),
    "w0_is_1_D3_pad1": ((8, 1), (16, 4), (8, 2), 3, 1, (2.0, 6.0), 0.5, 1.0),
    "h_is_1_D9_pad3": ((2, 8), (4, 16), (1, 8), 9, 3, (2.0, 6.0), 0.25, 1.0),                  # h = 1 < pad; half 1.125
    "w_is_1_D5": ((8, 2), (16, 4), (8, 1), 5, 0, (2.0, 6.0), 0.25, 1.0),
}
# each clamp must bite on more than none and fewer than all full-resolution pixels of these
LATTICE_CLAMPS_PARTIAL = ("up4_down2_D5", "two_blocks_up4_down2_D9_pad1", "up2_down2_D17_pad1", "up_only_D9_pad3", "down_only_D3_pad3_wider_than_h",
                          "all_identity_D2_pad1", "h0_is_1_D3", "w0_is_1_D3_pad1", "h_is_1_D9_pad3", "w_is_1_D5")


def lattice_case(name):
    hw0, HW, hw, D, pad, (near, far), k, interval = LATTICE[name]
    g = torch.Generator().manual_seed(5100 + list(LATTICE).index(name))
    cur = near + torch.randint(0, int((far - near) * 64) + 1, hw0, generator=g).double() / 64          # multiples of 2^-6 in [near, far]
    if hw0[0] * hw0[1] >= 4:                                               # the extremes are present whatever the draw: both clamps bite somewhere
        cur.view(-1)[0], cur.view(-1)[-1] = near, far
    return _case(name, cur, near, far, k, interval, D, HW, hw, pad)


def clamp_shares(ref, near, far):
    """Shares of the full-resolution pixels on which the lower / the upper clamp bites."""
    return (ref["c"] - ref["half"] < near).double().mean().item(), (ref["c"] + ref["half"] > far).double().mean().item()


def inexact_parts(c):
    """Names of the float64 chain's intermediates that do NOT survive a round trip through float32 (empty: the case is on the lattice), plus
    'float32 chain' where the chain run in float32 differs from the float64 one."""
    ref = reference(c)
    bad = [key for key in ("half", "c", "lo", "hi", "step", "samples", "out") if not torch.equal(ref[key].float().double(), ref[key])]
    ref32 = reference(c, torch.float32)
    if any(not torch.equal(ref32[key].double(), ref[key]) for key in ("c", "lo", "hi", "step", "samples", "out")):
        bad.append("float32 chain")
    # the kernel forms half = (D / 2) * (k * interval) in float32: both products must be exact too
    k32, i32 = torch.tensor(c["k"]), torch.tensor(c["interval"] if c["interval"] is not None else c["far"] - c["near"])
    if (torch.tensor(c["D"] / 2) * (k32 * i32)).double() != ref["half"] or (k32 * i32).double().item() != interval_pixel_of(c):
        bad.append("device half")
    return bad


# ------------------------------------------------------------------------------------------------ B: the footprint read-out
# name: cur, full, out, D, pad.  k = 0 and near / far beyond reach: lo = hi = c, every plane is the composed bilinear map of cur_depth
FOOTPRINT = {
    "power_of_two_D9_pad1": ((3, 4), (12, 16), (6, 8), 9, 1),
    "non_integer_D3": ((5, 7), (20, 28), (9, 11), 3, 0),
}
FOOT_NEAR, FOOT_FAR = -1024.0, 1024.0
FOOT_BAR = S.bar(1.0)              # the data of a one-hot (and of the all-ones) map is bounded by 1: cascade_stubs.bar with that bound in far's place


def footprint_case(name, hot=None):
    """hot = (i, j): the one-hot map; None: all ones."""
    hw0, HW, hw, D, pad = FOOTPRINT[name]
    cur = torch.ones(hw0) if hot is None else torch.zeros(hw0)
    if hot is not None:
        cur[hot] = 1.0
    return _case(name, cur, FOOT_NEAR, FOOT_FAR, 0.0, None, D, HW, hw, pad)


# ------------------------------------------------------------------------------------------------ C: depth chunks
CHUNK_DEPTHS = (7, 8, 9, 16, 17, 49)
CHUNK_LATTICE = ("two_blocks_up4_down2_D9_pad1", "up2_down2_D17_pad1", "h_is_1_D9_pad3")          # D = 9 and 17: the formula of planes 0 and D - 1 is exact
GUARD_CASES = ("two_blocks_up4_down2_D9_pad1", "up2_down2_D17_pad1")                               # D = 9 and D = 17 with pad 1


def chunk_case(D):
    """One continuous case at depth count D: the non-integer ratio with pad 1."""
    cur = C_NEAR + (C_FAR - C_NEAR) * torch.rand(9, 11, generator=torch.Generator().manual_seed(5300))
    return _case("chunks_D%d" % D, cur, C_NEAR, C_FAR, 1 / 48, None, D, (32, 40), (8, 10), 1)


def line_through_the_ends(planes):
    """lo + d * (hi - lo) / (D - 1) from planes 0 and D - 1 of a [D, ., .] volume, in float64."""
    D = planes.shape[0]
    first, last = planes[0].double(), planes[-1].double()
    return first[None] + torch.arange(D, dtype=torch.float64).reshape(-1, 1, 1) * ((last - first) / (D - 1))[None]


# ------------------------------------------------------------------------------------------------ F: continuous cases
CONTINUOUS = list(MAP_CASES) + ["both_clamps_everywhere", "near_equals_far", "step_edge"]


def continuous_case(name):
    if name in MAP_CASES:                                                  # the inputs of tests/test_hip_cascade.py's map_refs, seed for seed
        hw0, HW, hw, D, ratio, pad = MAP_CASES[name]
        cur = C_NEAR + (C_FAR - C_NEAR) * torch.rand(*hw0, generator=torch.Generator().manual_seed(190 + list(MAP_CASES).index(name)))
        return _case(name, cur, C_NEAR, C_FAR, ratio / 48.0, None, D, HW, hw, pad)
    g = torch.Generator().manual_seed(5600 + CONTINUOUS.index(name))
    if name == "both_clamps_everywhere":                                   # half = 8 / 2 * 16 * 9 / 48 = 12 > far - near = 9: the band is [near, far] everywhere
        cur = C_NEAR + (C_FAR - C_NEAR) * torch.rand(7, 9, generator=g)
        return _case(name, cur, C_NEAR, C_FAR, 16 / 48.0, None, 8, (28, 36), (13, 17), 1)
    if name == "near_equals_far":                                          # the interval is 0: lo = max(c, near), hi = min(c, far)
        cur = 3.0 + 4.0 * torch.rand(7, 9, generator=g)
        return _case(name, cur, 5.0, 5.0, 2 / 48.0, None, 9, (28, 36), (14, 18), 1)
    if name == "step_edge":                                                # a step of (far - near) / 2 across the middle of the map; the two axes'
        cur = C_NEAR + (C_FAR - C_NEAR) * (0.2 + 0.1 * torch.rand(10, 12, generator=g))      # down-sampling ratios differ and neither is an integer
        cur[5:] += (C_FAR - C_NEAR) / 2
        return _case(name, cur, C_NEAR, C_FAR, 2 / 48.0, None, 17, (40, 48), (17, 21), 1)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ E: non-finite depths
# name: cur, full, out, D, pad, ratio
NONFINITE = {
    "integer_ratio_pad1": ((6, 8), (24, 32), (12, 16), 5, 1, 2),
    "non_integer_ratio_pad1": ((9, 11), (32, 40), (8, 10), 9, 1, 3),
}
NONFINITE_KINDS = ("nan", "+inf", "-inf")
NONFINITE_SPOTS = ("interior", "corner")


def nonfinite_case(name, kind, spot):
    """One pixel of cur_depth is NaN, +inf or -inf: in the interior or at the (0, 0) corner."""
    hw0, HW, hw, D, pad, ratio = NONFINITE[name]
    cur = C_NEAR + (C_FAR - C_NEAR) * torch.rand(*hw0, generator=torch.Generator().manual_seed(5500 + list(NONFINITE).index(name)))
    at = (hw0[0] // 2, hw0[1] // 2) if spot == "interior" else (0, 0)
    cur[at] = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[kind]
    c = _case("%s/%s/%s" % (name, kind, spot), cur, C_NEAR, C_FAR, ratio / 48.0, None, D, HW, hw, pad)
    c["at"] = at
    return c


def nonfinite_all_three(name):
    """NaN, +inf and -inf in one map, far enough apart that each keeps a footprint of its own."""
    hw0, HW, hw, D, pad, ratio = NONFINITE[name]
    cur = C_NEAR + (C_FAR - C_NEAR) * torch.rand(*hw0, generator=torch.Generator().manual_seed(5550 + list(NONFINITE).index(name)))
    cur[0, 0], cur[hw0[0] // 2, hw0[1] // 2], cur[-1, -1] = float("nan"), float("inf"), float("-inf")
    return _case(name + "/all_three", cur, C_NEAR, C_FAR, ratio / 48.0, None, D, HW, hw, pad)


def classes(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, per element."""
    return torch.isnan(t).long() + 2 * torch.isposinf(t).long() + 3 * torch.isneginf(t).long()


def chain_grad64(c, g_out):
    """torch float64 autograd through cascade_stubs.hypotheses_chain on the case (the reference of tests/test_hip_cascade_grad.py)."""
    x = c["cur"].double().clone().requires_grad_(True)
    ip = torch.tensor(interval_pixel_of(c), dtype=torch.float64)
    out, _ = S.hypotheses_chain(x, torch.tensor(c["near"], dtype=torch.float64), torch.tensor(c["far"], dtype=torch.float64), ip, c["D"], c["HW"], c["hw"], c["pad"])
    out.backward(g_out.double())
    return x.grad.detach()
