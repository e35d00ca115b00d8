"""Cases for the gradient chain depth regression -> depth_values -> depth hypotheses -> previous depth (ucnerf_depth_hypotheses_bwd,
ucnerf_depth_regress_bwd_values), shared by tests/test_cascade_grad_host.py (which proves on the CPU that the cases are what they claim) and
tests/test_hip_cascade_grad.py (which runs the kernels on them).

The reference of every hypothesis gradient is torch autograd through cascade_stubs.hypotheses_chain (pinned to fixture G19 by
tests/test_cascade_host.py) in float64 on the CPU; the same function in float32 on the CPU is the second witness.

  LATTICE cases: cur_depth in multiples of 1/4, near / far / half dyadic, all three size ratios powers of two, D - 1 a power of two, g_out small
  integers.  Every product and every partial sum of the gradient is then a dyadic number that float32 holds exactly, whatever the order of the
  sums: the builder asserts float32 autograd == float64 autograd and that the sum of |contributions| per cell times 2^(fraction bits) stays below
  2^24.  The device is compared with torch.equal.
  CONTINUOUS cases: random cur_depth in [near, far], random normal g_out.  A full-resolution pixel whose float64 c - half lies within 4 eps of
  near (or c + half of far), eps = the float32 chain's largest error in c on the case, may take either side of the clamp in float32: it is
  excluded, and g_out is zeroed on every column whose taps touch one, so EVERY gradient element is compared.

Our own code; nothing here is needed by the package.
"""
import math

import torch
import torch.nn.functional as F

import cascade_stubs as S

NEAR, FAR = 2.0, 10.0              # lattice cases (dyadic)
C_NEAR, C_FAR = 2.0, 11.0          # continuous cases (as tests/test_hip_cascade.py)

# name: cur (h0, w0), full (H, W), out (h, w), D, pad, interval (half = D / 2 * interval)
LATTICE = {
    "x4_x2_D5": ((5, 7), (20, 28), (10, 14), 5, 0, 0.5),                  # half 1.25: ties at c = 3.25 and c = 8.75
    "chunks_D33_pad1": ((6, 6), (24, 24), (6, 6), 33, 1, 0.125),          # half 2.0625 (no multiple of 1/4: no tie); several depth chunks
    "wide_band_D3_pad1": ((6, 6), (24, 24), (12, 12), 3, 1, 3.0),         # half 4.5 > (far - near) / 2: one clamp at least bites, both in between
    "identity_down_D9_pad2": ((16, 20), (32, 40), (32, 40), 9, 2, 0.5),   # half 2.25: ties at 4.25 and 7.75
    "one_pixel_D2_pad1": ((1, 1), (4, 4), (2, 2), 2, 1, 1.25),            # every tap clamps; cur = near + half: a tie on every pixel
    "row_map_D3": ((1, 7), (4, 28), (2, 14), 3, 0, 0.5),                  # half 0.75
    "column_map_D3_pad2": ((7, 1), (28, 4), (14, 2), 3, 2, 0.5),
    "all_scales_one_D5_pad1": ((6, 5), (6, 5), (6, 5), 5, 1, 0.5),
}
# name: cur, full, out, D, pad, ratio (interval_pixel = ratio * (far - near) / 48, as CascadeMVSNet forms it)
CONTINUOUS = {
    "no_multiple_of_anything": ((5, 7), (20, 28), (10, 14), 4, 0, 1),
    "non_integer_ratio_pad1": ((9, 11), (32, 40), (8, 10), 5, 1, 3),
    "chunks_rows_narrower_than_a_wave": ((6, 6), (24, 24), (6, 6), 48, 0, 0.5),          # (half = 24 * 0.5 * 9 / 48 = 2.25: the band fits)
    "identity_down_pad2": ((16, 20), (32, 40), (32, 40), 8, 2, 1),
}


def chain_grad(cur, g_out, near, far, interval_pixel, D, HW, hw, pad, dtype):
    """autograd through the restated chain in `dtype` on the CPU -> (g_cur_depth, c): the reference (float64) or the second witness (float32)."""
    x = cur.to(dtype).clone().requires_grad_(True)
    out, (_, _, c) = S.hypotheses_chain(x, torch.tensor(near, dtype=dtype), torch.tensor(far, dtype=dtype), torch.tensor(interval_pixel, dtype=dtype),
                                        D, HW, hw, pad)
    out.backward(g_out.to(dtype))
    return x.grad.detach(), c.detach()


def _log2_exact(q):
    b = int(round(math.log2(q)))
    assert 2 ** b == q, "ratio %r is not a power of two" % (q,)
    return b


def _fraction_bits(hw0, HW, hw, D):
    """Bits behind the binary point of any contribution g * (1 - d/(D-1) or d/(D-1)) * ly * lx * uy * ux: an interpolation weight of a
    power-of-two ratio r > 1 is a multiple of 1 / (2 r), of ratio 1 it is 0 or 1."""
    bits = _log2_exact(D - 1)
    for big, small in ((HW[0], hw[0]), (HW[1], hw[1]), (HW[0], hw0[0]), (HW[1], hw0[1])):
        r = _log2_exact(big / small)
        bits += r + 1 if r else 0
    return bits


def lattice_case(name):
    hw0, HW, hw, D, pad, interval = LATTICE[name]
    g = torch.Generator().manual_seed(4150 + list(LATTICE).index(name))
    half = D / 2 * interval
    assert half * 1024 == int(half * 1024) and NEAR * 4 == int(NEAR * 4) and FAR * 4 == int(FAR * 4)
    ties = half * 4 == int(half * 4)                                       # (cur_depth is in multiples of 1/4: a tie needs half to be one too)
    cur = NEAR + torch.randint(0, int((FAR - NEAR) * 4) + 1, hw0, generator=g).double() / 4
    # constant patches (>= 2 x 2 where the map has the room): full-resolution pixels inside them sample exactly the patch's value
    ph, pw = min(2, hw0[0]), min(3, hw0[1])
    if ties and NEAR + half <= FAR:
        cur[:ph, :pw] = NEAR + half                                        # c - half == near: a tie of the lower clamp
    if ties and hw0[0] * hw0[1] > 1 and FAR - half >= NEAR:
        cur[-ph:, -pw:] = FAR - half                                       # c + half == far: a tie of the upper clamp
    if hw0[0] >= 5 and hw0[1] >= 5:                                        # both clamps idle / the lower one biting / the upper one biting
        cur[2, 3], cur[3, 1], cur[2, 4] = (NEAR + FAR) / 2, NEAR, FAR
    top = 2 if D < 33 else 1                                               # (33 depths: smaller integers keep the mass bound below)
    g_out = torch.randint(-top, top + 1, (D, hw[0] + 2 * pad, hw[1] + 2 * pad), generator=g).double()
    if pad:                                                                # nonzero on border and corner cells, whatever the draw
        g_out[0, 0, 0], g_out[-1, -1, -1], g_out[0, 0, pad + 1], g_out[-1, pad + 1, -1] = 1.0, -1.0, 1.0, 1.0
    want, c = chain_grad(cur, g_out, NEAR, FAR, interval, D, HW, hw, pad, torch.float64)
    want32, c32 = chain_grad(cur, g_out, NEAR, FAR, interval, D, HW, hw, pad, torch.float32)
    assert torch.equal(want32.double(), want) and torch.equal(c32.double(), c), name + ": float32 autograd differs from float64: not a lattice case"
    mass, _ = chain_grad(cur, g_out.abs(), NEAR, FAR, interval, D, HW, hw, pad, torch.float64)
    # (with |g_out| every contribution is >= 0 -- the weights, d/(D-1) and 1 - d/(D-1) are --, so the gradient IS the sum of |contributions|;
    #  where a clamp blocks a term the mass is smaller, never larger, than what any partial sum can reach)
    bits = _fraction_bits(hw0, HW, hw, D)
    assert mass.max().item() * 2.0 ** bits < 2.0 ** 24, (name, mass.max().item(), bits)
    lo_on, hi_on = c - half < NEAR, c + half > FAR
    census = {"tie_lo": int((c - half == NEAR).sum()), "tie_hi": int((c + half == FAR).sum()), "both": int((lo_on & hi_on).sum()),
              "one": int((lo_on ^ hi_on).sum()), "none": int((~lo_on & ~hi_on).sum()),
              "border_nonzero": int((g_out[:, :pad].ne(0).sum() + g_out[:, :, :pad].ne(0).sum()) if pad else 0),
              "corner_nonzero": int((g_out[:, :pad, :pad].ne(0).sum() + g_out[:, -pad:, -pad:].ne(0).sum()) if pad else 0)}
    return {"name": name, "cur": cur.float(), "g_out": g_out.float(), "near": NEAR, "far": FAR, "interval": interval, "k": 1.0, "D": D, "HW": HW, "hw": hw,
            "pad": pad, "want": want, "census": census, "mass_bits": (mass.max().item(), bits)}


def continuous_case(name):
    hw0, HW, hw, D, pad, ratio = CONTINUOUS[name]
    g = torch.Generator().manual_seed(4200 + list(CONTINUOUS).index(name))
    cur = (C_NEAR + (C_FAR - C_NEAR) * torch.rand(*hw0, generator=g)).float()
    g_out = torch.randn(D, hw[0] + 2 * pad, hw[1] + 2 * pad, generator=g).float()
    interval_pixel = ratio * ((C_FAR - C_NEAR) / 48)
    half = D / 2 * interval_pixel
    zeros = torch.zeros_like(g_out)
    _, c64 = chain_grad(cur, zeros, C_NEAR, C_FAR, interval_pixel, D, HW, hw, pad, torch.float64)
    _, c32 = chain_grad(cur, zeros, C_NEAR, C_FAR, interval_pixel, D, HW, hw, pad, torch.float32)
    eps = (c32.double() - c64).abs().max().item()
    excluded = ((c64 - half - C_NEAR).abs() <= 4 * eps) | ((c64 + half - C_FAR).abs() <= 4 * eps)
    # the columns whose down-sampling taps touch an excluded pixel: where the interpolated mask is not 0, under the float32 and the float64 tap rule
    touched = torch.zeros(hw, dtype=torch.bool)
    for dt in (torch.float32, torch.float64):
        touched |= F.interpolate(excluded.to(dt)[None, None], list(hw), mode="bilinear", align_corners=False)[0, 0] > 0
    if pad:
        touched = F.pad(touched.double()[None, None], (pad,) * 4, "replicate")[0, 0] > 0
    g_out = g_out * (~touched).float()
    want, _ = chain_grad(cur, g_out, C_NEAR, C_FAR, interval_pixel, D, HW, hw, pad, torch.float64)
    want32, _ = chain_grad(cur, g_out, C_NEAR, C_FAR, interval_pixel, D, HW, hw, pad, torch.float32)
    witness = (want32.double() - want).abs().max().item()
    lo_on, hi_on = c64 - half < C_NEAR, c64 + half > C_FAR
    return {"name": name, "cur": cur, "g_out": g_out, "near": C_NEAR, "far": C_FAR, "interval": None, "k": ratio / 48.0, "D": D, "HW": HW, "hw": hw,
            "pad": pad, "want": want, "witness": witness, "bar": 4 * witness + 1e-6 * want.abs().max().item(), "eps": eps,
            "excluded_share": excluded.double().mean().item(), "zeroed_columns": int(touched.sum()),
            "clamp_shares": (lo_on.double().mean().item(), hi_on.double().mean().item())}


# ------------------------------------------------------------------------------------------------ depth regression: the gradient of depth_values
# name: D, inner plane (H, W), pad, hot depths k
REGRESS = {
    "D1_one_pixel": (1, (1, 1), 0, 1),
    "D2_one_pixel_pad1": (2, (1, 1), 1, 2),
    "D8_33_pixels_pad3": (8, (3, 11), 3, 3),
    "D9_99_pixels_pad1": (9, (9, 11), 1, 5),
    "D128_33_pixels": (128, (3, 11), 0, 7),
    "D128_99_pixels_pad3": (128, (9, 11), 3, 128),
}


def regress_case(name):
    """prob = float32(1/k) on k hot depths per pixel (the border included: it must not leak), integer g_depth.  One product per element: `want`
    is that product in float64, where it is exact, and want.float() its correct rounding -- what a float32 multiplication returns."""
    D, (H, W), pad, k = REGRESS[name]
    g = torch.Generator().manual_seed(4300 + list(REGRESS).index(name))
    Hp, Wp = H + 2 * pad, W + 2 * pad
    hot = torch.rand(D, Hp, Wp, generator=g).argsort(0) < k               # k depths per pixel
    prob = (hot.float() / k)                                               # float32 1/k
    g_depth = torch.randint(-3, 4, (H, W), generator=g).float()
    g_depth[0, 0] = 2.0
    dv = torch.zeros(D, Hp, Wp, dtype=torch.float64, requires_grad=True)
    depth = (prob.double() * dv).sum(0)[pad:Hp - pad, pad:Wp - pad]
    depth.backward(g_depth.double())
    want = dv.grad
    assert int(hot.sum(0).min()) == int(hot.sum(0).max()) == k
    return {"name": name, "prob": prob, "g_depth": g_depth, "pad": pad, "want": want}
