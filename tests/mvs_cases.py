"""Cases and float64 reference for the MVS stage kernels' edge tests (tests/test_mvs_cases_host.py, tests/test_hip_mvs_edges.py).

The reference is oracle.mvs_oracle.cost_volume_variance / depth_regress run in float64, with autograd through them for the gradients; the same
functions in float32 are the second witness.

COST-VOLUME LATTICE.  proj[v] = [R | T] with third row (0, 0, c, 0), c in {1, 2, 0.5, -1}: the homogeneous coordinate is the constant c, so the source
pixel of a voxel is ix = (r00 x + r01 y + r02 + T0 / depth) / c -- small integers, a power-of-two T, depth in {0.5, 1, 2, 4} chosen PER VOXEL, W - 1 and
H - 1 powers of two: every coordinate is dyadic (multiples of 1/8 at the finest) and float32 computes it without rounding (check_cv_lattice asserts
float32 grid == float64 grid per view).  Features are integers |v| <= 8, g_variance integers |g| <= 2.
  class P: 1 + (views that see the voxel) is a power of two for every voxel (V = 1; V views that share one projection, 3 or 7 of them; views that never
           see anything).  count = 2^-k, and variance, count and g_feats are exact: float32 oracle == float64 oracle element for element, and
           2 * (sum of |contribution| per g_feats cell) * 2^(fraction bits of the contributions) < 2^24 bounds every partial sum of the atomics,
           whatever their order, for one call and for two into the same array.
  class Q: any count.  Coordinates, pixel indices and 1 + views-in-view are still exact; count = 1 / msum and the variance round, in the same
           operation order on both sides, so they are compared with the FLOAT32 oracle bit for bit; g_feats is compared with float64 under bar().
  runs:    the backward combines runs of equal source pixel along the 8 depth positions of a wave.  depth_values of the "runs" cases follow
           per-pixel schedules: a run of every length in RUN_LENGTHS starting at every position in RUN_STARTS of a wave's 8 (census counts
           them from the float64 indices, per view).

DEPTH-REGRESSION LATTICE.  Logits 0 on k hot depths and -200 elsewhere, k in {1, 2, 4, 8}: expf(-200) is 0 in float32, so p = 1 / k exactly;
depth_values are multiples of 1/4, g_depth and g_confidence small integers: probabilities, depth, E[d], the window sum and the whole backward are
exact.  (In float64 exp(-200) = 1.4e-87 is not 0: the float64 reference is compared after rounding it to float32, which turns those entries, and
nothing else, into 0 -- check_dr_lattice asserts that every other entry is a float32 number already.)

CONTINUOUS cases: random poses as tests/fuzz_mvs.py draws them.  A voxel is left out where a float64 coordinate of some view sits within
4 x (the float32 oracle's own largest coordinate error on that case) of a decision: unclamped ix / iy at a half-integer inside the map, gx / gy at
+-1; a depth-regression pixel where float64 E[d] is that close to an integer, or the window sum that close to 1 (the clamp's gradient switches
there).  At most 2 % per case (asserted).  g_variance on the excluded voxels and g_confidence on the excluded pixels are 0 on both sides, so the
gradients are compared on every element."""
import functools

import numpy as np
import torch

from oracle import mvs_oracle as M

F64, F32 = torch.float64, torch.float32
DEPTH_SET = (0.5, 1.0, 2.0, 4.0)
RUN_LENGTHS = (1, 2, 7, 8, 9)
RUN_STARTS = (0, 1, 7)
EXCLUDED_CAP = 0.02


def bar(oracle_distance, scale):
    """What the device may differ from the float64 reference by: 4 x the float32 oracle's own distance + 1e-6 of the output's largest reference value
    (the rule of gather_cases.bar and composite_cases)."""
    return 4.0 * oracle_distance + 1e-6 * scale


def _frac_bits(x):
    """Smallest b with x * 2^b integer for every element (float64 input)."""
    for b in range(0, 40):
        y = x * 2.0 ** b
        if bool((y == torch.floor(y)).all()):
            return b
    raise AssertionError("value is not dyadic")


# ------------------------------------------------------------------------------------------------ cost volume: geometry
def view_pool(H, W):
    """(row 0 of R, row 1 of R, (T0, T1), c) per lattice view."""
    return [
        ((1, 0, 0), (0, 1, 0), (2, 0), 1.0),            # 0: ix = x + {4, 2, 1, 0.5}: x.5 on even and odd x, the right border and past it
        ((1, 0, 0), (0, 1, 0), (0, 1), 2.0),            # 1: ix = x / 2, iy = (y + 1 / depth) / 2: halves and quarters
        ((-1, 0, W - 1), (0, 1, 0), (-1, 2), 1.0),      # 2: mirrored in x, moving left and down
        ((0, 1, 0), (1, 0, 0), (1, -2), 1.0),           # 3: x and y swapped, moving up
        ((-1, 0, 0), (0, -1, 0), (-2, -1), -1.0),       # 4: behind the camera, landing in view: ix = x + 2 / depth
        ((1, 1, 0), (0, 1, -1), (0, 2), 0.5),           # 5: c = 0.5: coordinates doubled, mostly far outside
        ((0, 0, 0), (0, 0, 0), (0, 0), 1.0),            # 6: T = 0 and no x, y: pixel (0, 0) receives EVERY voxel; gx = gy = -1, never in view
        ((1, 0, -1), (0, 1, 1), (-2, 2), 1.0),          # 7: shifted, moving left and down
        ((1, 0, 0), (0, 1, 0), (4, 4), -1.0),           # 8: behind the camera, landing past the left and top borders
    ]


def lattice_proj(view_ids, H, W):
    pool = view_pool(H, W)
    out = torch.zeros(len(view_ids), 3, 4, dtype=F64)
    for k, i in enumerate(view_ids):
        r0, r1, t, c = pool[i]
        out[k, 0, :3], out[k, 1, :3] = torch.tensor(r0, dtype=F64), torch.tensor(r1, dtype=F64)
        out[k, 0, 3], out[k, 1, 3], out[k, 2, 2] = t[0], t[1], c
    return out


def cv_coords(case, dtype=F64):
    """Per view and voxel: gx, gy (normalised), ix, iy (unnormalised, unclamped), idx (the pixel picked), inside (the mask) -- each [V, D*plane]."""
    H, W, pad = case["H"], case["W"], case["pad"]
    dv = case["depth_values"].to(dtype)
    gx, gy = [], []
    for v in range(case["V"]):
        g = M.homo_warp_grid(case["proj"][v].to(dtype), dv, H, W, pad).reshape(-1, 2)
        gx.append(g[:, 0]); gy.append(g[:, 1])
    gx, gy = torch.stack(gx), torch.stack(gy)
    ix, iy = ((gx + 1) / 2) * (W - 1), ((gy + 1) / 2) * (H - 1)
    idx = torch.round(iy.clamp(0, H - 1)).long() * W + torch.round(ix.clamp(0, W - 1)).long()
    return dict(gx=gx, gy=gy, ix=ix, iy=iy, idx=idx, inside=(gx > -1) & (gx < 1) & (gy > -1) & (gy < 1))


def cv_reference(case, dtype=F64, g_variance=None):
    """cost_volume_variance in `dtype` -> (variance [C,D,Hp,Wp], count [D,Hp,Wp], g_feats [V,C,H,W])."""
    feats = case["feats"].to(dtype).clone().requires_grad_(True)
    var, cnt = M.cost_volume_variance(feats, case["proj"].to(dtype), case["depth_values"].to(dtype), case["pad"])
    var.backward((case["g_variance"] if g_variance is None else g_variance).to(dtype))
    return var.detach(), cnt.detach(), feats.grad.detach()


def _run_schedules(D):
    """Depth-value index per depth for one pixel: s single-depth runs, one run of L, singles to the end -- values cycling through three of
    DEPTH_SET so that neighbouring runs differ; then A B A B .. and one value for the whole column."""
    out = []
    for s in RUN_STARTS:
        for L in RUN_LENGTHS:
            lens = [1] * s + [L]
            col = [k % 3 for k, n in enumerate(lens) for _ in range(n)]
            k = len(lens)
            while len(col) < D:
                col.append(k % 3); k += 1
            out.append(col[:D])
    out.append([d % 2 for d in range(D)])
    out.append([3] * D)
    return out


def cv_lattice_case(name, views, C, HW, D, pad, runs=False, seed=0):
    H, W = HW
    V, Hp, Wp = len(views), H + 2 * pad, W + 2 * pad
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).to(F64)      # noqa: E731
    if runs:
        sched = _run_schedules(D)
        which = torch.tensor([[sched[p % len(sched)][d] for p in range(Hp * Wp)] for d in range(D)])
    else:
        which = torch.randint(0, 4, (D, Hp * Wp), generator=gen)
    dv = torch.tensor(DEPTH_SET, dtype=F64)[which].reshape(D, Hp, Wp)
    return dict(name=name, kind="lattice", V=V, C=C, H=H, W=W, D=D, pad=pad, views=tuple(views), proj=lattice_proj(views, H, W), depth_values=dv,
                feats=ri(-8, 8, V, C, H, W), g_variance=ri(-2, 2, C, D, Hp, Wp))


def cv_class(case):
    """"P" when 1 + views-in-view is a power of two on every voxel, else "Q"."""
    msum = 1 + cv_coords(case)["inside"].sum(0)
    return "P" if bool(((msum & (msum - 1)) == 0).all()) else "Q"


def check_cv_lattice(case):
    """The exactness conditions (module docstring).  Returns (class, float64 (variance, count, g_feats), float32 (variance, count, g_feats))."""
    name = case["name"]
    assert all(float(d) in DEPTH_SET for d in case["depth_values"].unique().tolist())
    assert case["feats"].abs().max() <= 8 and case["g_variance"].abs().max() <= 2
    assert bool((case["proj"][:, 2, [0, 1, 3]] == 0).all()) and all(c in (1.0, 2.0, 0.5, -1.0) for c in case["proj"][:, 2, 2].tolist())
    c64, c32 = cv_coords(case), cv_coords(case, F32)
    for k in ("gx", "gy", "ix", "iy"):
        assert torch.equal(c32[k].double(), c64[k]), "%s: float32 %s != float64" % (name, k)
        assert _frac_bits(c64[k]) <= (3 if k in ("ix", "iy") else 8), (name, k)      # pixels: multiples of 1/8; gx = ix / ((W - 1) / 2) - 1
    assert torch.equal(c32["idx"], c64["idx"]) and torch.equal(c32["inside"], c64["inside"])
    ref, f32 = cv_reference(case), cv_reference(case, F32)
    cls = cv_class(case)
    if cls == "P":
        for k, a, b in zip(("variance", "count", "g_feats"), f32, ref):
            assert torch.equal(a.double(), b), "%s: float32 oracle != float64 oracle (%s)" % (name, k)
        # every partial sum of the atomics: sum of |2 count g (v_i - mean)| per g_feats cell, twice (the call-twice test), at the contributions' grain
        V, C, H, W = case["feats"].shape
        n = case["D"] * (H + 2 * case["pad"]) * (W + 2 * case["pad"])
        cnt = ref[1].reshape(1, n)
        g = case["g_variance"].reshape(C, n)
        picked = [case["feats"][i].reshape(C, H * W)[:, c64["idx"][i]] for i in range(V)]          # [C, n] per view
        mean = sum(picked) * cnt
        bits, worst = 0, 0.0
        for i in range(V):
            contrib = 2 * cnt * g * (picked[i] - mean)
            bits = max(bits, _frac_bits(contrib))
            cell = torch.zeros(C, H * W, dtype=F64).index_add_(1, c64["idx"][i], contrib.abs())
            assert bool((ref[2][i].reshape(C, H * W).abs() <= cell).all())
            worst = max(worst, cell.max().item())
        assert 2 * worst * 2.0 ** bits < 2 ** 24, (name, worst, bits)
        assert ref[0].abs().max().item() * 2.0 ** _frac_bits(ref[0]) < 2 ** 24
    else:
        msum32 = 1.0 / f32[1].double()
        assert torch.equal(torch.round(msum32), (1 + c64["inside"].sum(0)).double().reshape(msum32.shape)), name
    return cls, ref, f32


def cv_census(case):
    """What a cost-volume case holds, from its float64 coordinates: counts of (view, voxel) pairs, and the runs along depth per (view, pixel)."""
    c = cv_coords(case)
    H, W, D, V = case["H"], case["W"], case["D"], case["V"]
    plane = (H + 2 * case["pad"]) * (W + 2 * case["pad"])
    gx, gy, ix, iy = c["gx"], c["gy"], c["ix"], c["iy"]
    in_x, in_y = (gx > -1) & (gx < 1), (gy > -1) & (gy < 1)

    def half(t, size, parity):
        return (t >= 0) & (t <= size - 1) & (t - t.floor() == 0.5) & (t.floor() % 2 == parity)
    out = {"half_x_even": half(ix, W, 0), "half_x_odd": half(ix, W, 1), "half_y_even": half(iy, H, 0), "half_y_odd": half(iy, H, 1),
           "edge_x_lo": (gx == -1) & in_y, "edge_x_hi": (gx == 1) & in_y, "edge_y_lo": (gy == -1) & in_x, "edge_y_hi": (gy == 1) & in_x,
           "out_x_lo": gx < -1, "out_x_hi": gx > 1, "out_y_lo": gy < -1, "out_y_hi": gy > 1,
           "behind": (case["proj"][:, 2, 2] < 0).view(V, 1).expand_as(gx), "in_view": c["inside"]}
    out = {k: int(t.sum()) for k, t in out.items()}
    idx = c["idx"].reshape(V, D, plane).numpy()
    runs, crossing, aba, all_different, one_pixel = set(), 0, 0, 0, 0
    for v in range(V):
        one_pixel += int((idx[v] == idx[v].flat[0]).all())
        heads = np.ones((D, plane), dtype=bool)
        heads[1:] = idx[v][1:] != idx[v][:-1]
        for p in range(plane):
            starts = np.flatnonzero(heads[:, p]).tolist() + [D]
            for a, b in zip(starts[:-1], starts[1:]):
                runs.add((a % 8, b - a))
                crossing += int(a // 8 != (b - 1) // 8)
        if D >= 3:
            same_wave = (np.arange(D - 2) // 8 == (np.arange(D - 2) + 2) // 8)[:, None]
            aba += int(((idx[v][2:] == idx[v][:-2]) & (idx[v][1:-1] != idx[v][:-2]) & same_wave).sum())
        for w in range(D // 8):                                              # a wave of the backward: 8 pixels x 8 depths, all live
            for g in range(plane // 8):
                marks = heads[w * 8 + 1:w * 8 + 8, g * 8:g * 8 + 8]         # (position 0 is a head in every column)
                all_different += int(len({tuple(col) for col in marks.T.tolist()}) == 8)
    out.update(runs=runs, run_crossing_a_wave=crossing, a_b_a=aba, wave_of_8_different_columns=all_different, one_pixel_for_every_voxel=one_pixel)
    return out


CV_LATTICE_SPECS = {
    # class P
    "p_v1_c1_d1_plane4": dict(views=[0], C=1, HW=(2, 2), D=1, pad=0),
    "p_v1_c3_d2_pad1": dict(views=[1], C=3, HW=(3, 3), D=2, pad=1),
    "p_v1_c16_d5": dict(views=[2], C=16, HW=(5, 9), D=5, pad=0),
    "p_v1_c17_d7_pad3": dict(views=[3], C=17, HW=(9, 5), D=7, pad=3),
    "p_v1_c24_d8_pad1": dict(views=[4], C=24, HW=(3, 5), D=8, pad=1),
    "p_v1_c33_d9_plane6": dict(views=[5], C=33, HW=(2, 3), D=9, pad=0),
    "p_v1_c3_d33": dict(views=[7], C=3, HW=(5, 17), D=33, pad=0),
    "p_v1_c3_d9_behind_pad1": dict(views=[8], C=3, HW=(5, 9), D=9, pad=1),
    "p_v3_c16_d16_pad1": dict(views=[1, 1, 1], C=16, HW=(5, 5), D=16, pad=1),
    "p_v7_c17_d17": dict(views=[3] * 7, C=17, HW=(3, 9), D=17, pad=0),
    "p_v8_c24_d31": dict(views=[0] * 7 + [6], C=24, HW=(3, 5), D=31, pad=0),
    "p_v2_c1_d32_pad1": dict(views=[2, 6], C=1, HW=(9, 33), D=32, pad=1),
    "p_runs_v3_c3_d40": dict(views=[0, 6, 6], C=3, HW=(3, 17), D=40, pad=0, runs=True),
    "p_runs_v1_c17_d17_pad1": dict(views=[4], C=17, HW=(3, 17), D=17, pad=1, runs=True),
    # class Q
    "q_v2_c3_d5_pad1": dict(views=[0, 1], C=3, HW=(5, 9), D=5, pad=1),
    "q_v3_c17_d9": dict(views=[2, 3, 5], C=17, HW=(5, 5), D=9, pad=0),
    "q_v7_c16_d8_pad3": dict(views=[0, 1, 2, 3, 4, 5, 6], C=16, HW=(9, 9), D=8, pad=3),
    "q_v8_c33_d17_pad1": dict(views=[0, 1, 2, 3, 4, 5, 7, 8], C=33, HW=(3, 17), D=17, pad=1),
    "q_runs_v8_c1_d40": dict(views=[0, 1, 2, 3, 4, 6, 7, 8], C=1, HW=(3, 17), D=40, pad=0, runs=True),
}
CV_LATTICE_NAMES = tuple(CV_LATTICE_SPECS)


@functools.lru_cache(maxsize=None)
def cv_lattice(name):
    """(case, class, float64 (variance, count, g_feats), float32 (variance, count, g_feats)), built and checked once per process."""
    case = cv_lattice_case(name, seed=CV_LATTICE_NAMES.index(name), **CV_LATTICE_SPECS[name])
    cls, ref, f32 = check_cv_lattice(case)
    assert cls == name[0].upper(), (name, cls)
    return case, cls, ref, f32


# ------------------------------------------------------------------------------------------------ depth regression: lattice
COLD = -200.0
DR_MODES = ("both", "depth", "confidence")


def dr_reference(case, dtype=F64, mode="both", g_confidence=None):
    """depth_regress in `dtype` -> (prob_volume, depth, confidence, g_prob_pre, g_prob_init or None)."""
    x = case["prob_pre"].to(dtype).clone().requires_grad_(True)
    init = case["prob_init"].to(dtype).clone().requires_grad_(True) if case.get("prob_init") is not None else None
    p, depth, conf = M.depth_regress(x, case["depth_values"].to(dtype), init, case["pad"])
    gc = (case["g_confidence"] if g_confidence is None else g_confidence).to(dtype)
    loss = 0
    if mode in ("both", "depth"):
        loss = loss + (depth * case["g_depth"].to(dtype)).sum()
    if mode in ("both", "confidence"):
        loss = loss + (conf * gc).sum()
    loss.backward()
    return p.detach(), depth.detach(), conf.detach(), x.grad.detach(), None if init is None else init.grad.detach()


def _hot_patterns(D):
    """Sets of hot depths (sizes 1, 2, 4, 8) that fit D hypotheses."""
    m = D // 2
    sets = [(0,), (D - 1,), (D - 2,), (m,),                                             # window index 0, D-1, D-2, the middle
            (0, 1), (D - 2, D - 1), (m, m + 1), (m - 1, m),                            # E[d] = d + 0.5 (truncated: 0, D-2, ..)
            (0, 2), (D - 3, D - 1), (m, m + 2), (m - 1, m + 1),                        # E[d] an integer exactly; window sum 1
            (0, 8), (1, 9), (D - 9, D - 1), (0, 16), (3, 11),                          # both owned by ONE depth lane; window sum 0
            (0, 3), (0, 7), (D - 8, D - 1), (2, 7),                                    # different lanes; the window holds one or none of them
            (0, 1, 2, 3), (D - 4, D - 3, D - 2, D - 1), (0, 2, 9, 11), (1, 3, 5, 7), (0, 8, 16, 24), (0, 1, D - 2, D - 1),
            tuple(range(8)), tuple(range(D - 8, D)), tuple(range(0, 16, 2)), tuple(range(0, 64, 8)), (0, 1, 2, 3, D - 4, D - 3, D - 2, D - 1)]
    out = []
    for s in sets:
        if all(0 <= d < D for d in s) and len(set(s)) == len(s) and tuple(sorted(s)) not in out:
            out.append(tuple(sorted(s)))
    return out


def dr_lattice_case(name, D, HpWp, pad, init, seed=0):
    Hp, Wp = HpWp
    gen = torch.Generator().manual_seed(seed)
    plane = Hp * Wp
    pats = _hot_patterns(D)
    logits = torch.full((D, plane), COLD, dtype=F64)
    hot = []
    for p in range(plane):
        s = pats[(p * 5 + seed) % len(pats)]
        hot.append(s)
        logits[list(s), p] = 0.0
    d, p = torch.meshgrid(torch.arange(D), torch.arange(plane), indexing="ij")
    dv = (0.5 + 0.25 * ((3 * d + p + seed) % 16)).to(F64)
    case = dict(name=name, kind="lattice", D=D, Hp=Hp, Wp=Wp, pad=pad, hot=hot, depth_values=dv.reshape(D, Hp, Wp), prob_init=None)
    if init:
        case["prob_init"] = torch.randint(-3, 4, (D, Hp, Wp), generator=gen).to(F64)
        case["prob_pre"] = logits.reshape(D, Hp, Wp) - case["prob_init"]
    else:
        case["prob_pre"] = logits.reshape(D, Hp, Wp)
    H, W = Hp - 2 * pad, Wp - 2 * pad
    case["g_depth"] = torch.randint(-3, 4, (H, W), generator=gen).to(F64)
    case["g_confidence"] = torch.randint(-3, 4, (H, W), generator=gen).to(F64)
    case["g_confidence"][case["g_confidence"] == 0] = 2.0                         # (every pixel's window takes part in the backward)
    return case


def _as_f32(t):
    """A float64 reference rounded to float32; asserts that only entries below 1e-30 (exp(-200) and its products) change."""
    r = t.float()
    changed = r.double() != t
    assert bool((t[changed].abs() < 1e-30).all()) and bool((r[changed] == 0).all())
    return r


def check_dr_lattice(case):
    """Float32 oracle == float64 oracle on every output and every backward mode.  Returns {mode: (prob, depth, conf, g_pre, g_init)} in float32."""
    out = {}
    for mode in DR_MODES:
        r64, r32 = dr_reference(case, F64, mode), dr_reference(case, F32, mode)
        for k, a, b in zip(("prob_volume", "depth", "confidence", "g_prob_pre", "g_prob_init"), r64, r32):
            if a is not None:
                assert torch.equal(_as_f32(a), b), "%s %s: float32 oracle != float64 oracle (%s)" % (case["name"], mode, k)
        if r32[4] is not None:
            assert torch.equal(r32[3], r32[4])
        out[mode] = r32
    k = torch.tensor([len(s) for s in case["hot"]], dtype=F32).reshape(case["Hp"], case["Wp"])
    assert torch.equal(out["both"][0].sum(0), torch.ones_like(k)) and torch.equal(out["both"][0].max(0)[0], 1 / k)       # p = 1 / k exactly
    return out


def dr_census(case):
    """What a depth-regression case holds, from float64: per INNER pixel (the ones whose depth and confidence are kept)."""
    D, Hp, Wp, pad = case["D"], case["Hp"], case["Wp"], case["pad"]
    out = dict.fromkeys(("e_integer_two_hot", "e_half", "window_0", "window_d_minus_2", "window_d_minus_1", "window_sum_1", "window_sum_below_1",
                         "hot_in_one_lane", "hot_in_different_lanes", "border_pixels"), 0)
    for p, s in enumerate(case["hot"]):
        y, x = p // Wp - pad, p % Wp - pad
        if not (0 <= y < Hp - 2 * pad and 0 <= x < Wp - 2 * pad):
            out["border_pixels"] += 1
            continue
        e = sum(s) / len(s)
        di = min(max(int(e), 0), D - 1)
        wsum = sum(1 for d in s if di - 1 <= d <= di + 2) / len(s)
        out["e_integer_two_hot"] += int(len(s) == 2 and s[1] == s[0] + 2)
        out["e_half"] += int(e - int(e) == 0.5)
        out["window_0"] += int(di == 0)
        out["window_d_minus_2"] += int(di == D - 2 and D >= 2)
        out["window_d_minus_1"] += int(di == D - 1)
        out["window_sum_1"] += int(wsum == 1)
        out["window_sum_below_1"] += int(wsum < 1)
        out["hot_in_one_lane"] += int(len(s) >= 2 and len({d % 8 for d in s}) == 1)
        out["hot_in_different_lanes"] += int(len(s) >= 2 and len({d % 8 for d in s}) == len(s))
    return out


DR_LATTICE_SPECS = {
    "d1_plane1": dict(D=1, HpWp=(1, 1), pad=0, init=False),
    "d2_plane31": dict(D=2, HpWp=(1, 31), pad=0, init=True),
    "d3_plane32": dict(D=3, HpWp=(4, 8), pad=0, init=False),
    "d7_plane33": dict(D=7, HpWp=(3, 11), pad=0, init=True),
    "d8_pad1_plane35": dict(D=8, HpWp=(5, 7), pad=1, init=False),
    "d9_pad3_plane72": dict(D=9, HpWp=(8, 9), pad=3, init=True),
    "d16_plane33": dict(D=16, HpWp=(11, 3), pad=0, init=False),
    "d17_pad1_plane45": dict(D=17, HpWp=(5, 9), pad=1, init=True),
    "d127_plane70": dict(D=127, HpWp=(7, 10), pad=0, init=False),
    "d128_pad1_plane99": dict(D=128, HpWp=(9, 11), pad=1, init=True),
}
DR_LATTICE_NAMES = tuple(DR_LATTICE_SPECS)


@functools.lru_cache(maxsize=None)
def dr_lattice(name):
    """(case, {mode: float32 reference}) of a depth-regression lattice case, built and checked once per process."""
    case = dr_lattice_case(name, seed=DR_LATTICE_NAMES.index(name), **DR_LATTICE_SPECS[name])
    return case, check_dr_lattice(case)


# ------------------------------------------------------------------------------------------------ the continuous cases
CONTINUOUS_SPECS = {
    "cont_near_v1_c8": dict(V=1, C=8, HW=(16, 24), D=8, pad=0, amp=0.01, logit_scale=0.3, init=False),
    "cont_mid_v4_c32_pad1": dict(V=4, C=32, HW=(20, 33), D=12, pad=1, amp=0.05, logit_scale=1.0, init=True),
    "cont_far_v8_c8_pad3": dict(V=8, C=8, HW=(13, 21), D=9, pad=3, amp=0.3, logit_scale=1.0, init=False),
    "cont_far_v8_c32": dict(V=8, C=32, HW=(24, 40), D=12, pad=0, amp=0.3, logit_scale=2.0, init=True),
}
CONTINUOUS_NAMES = tuple(CONTINUOUS_SPECS)


def continuous_case(name, V, C, HW, D, pad, amp, logit_scale, init, seed):
    """Cameras, maps and hypotheses as tests/fuzz_mvs.py draws them (every input a float32 number held in float64)."""
    from fuzz_render import pose
    H, W = HW
    Hp, Wp = H + 2 * pad, W + 2 * pad
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    f = float(rng.uniform(0.5, 1.5)) * W
    K4 = torch.eye(4)
    K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = f, f * float(rng.uniform(0.9, 1.1)), W / 2.0, H / 2.0
    w2c = torch.stack([torch.eye(4)] + [pose(rng, amp, amp) for _ in range(V)])
    affine = K4 @ w2c
    proj = (affine[1:] @ torch.inverse(affine)[0:1])[:, :3].contiguous()
    near = float(rng.uniform(0.5, 2.0))
    dv = (near + torch.linspace(0, float(rng.uniform(0.5, 4.0)), D).view(D, 1, 1) + 0.05 * torch.rand(D, Hp, Wp, generator=g)).contiguous()
    case = dict(name=name, kind="continuous", V=V, C=C, H=H, W=W, D=D, pad=pad, Hp=Hp, Wp=Wp, proj=proj.double(), depth_values=dv.double(),
                feats=torch.randn(V, C, H, W, generator=g).double(), g_variance=torch.randn(C, D, Hp, Wp, generator=g).double(),
                prob_pre=(torch.randn(D, Hp, Wp, generator=g) * logit_scale).double(),
                prob_init=torch.randn(D, Hp, Wp, generator=g).double() if init else None,
                g_depth=torch.randn(H, W, generator=g).double(), g_confidence=torch.randn(H, W, generator=g).double())
    # ---- cost volume: voxels next to a decision.  The float32 oracle's coordinate error is measured where a decision can lie: within a pixel of the map
    c64, c32 = cv_coords(case), cv_coords(case, F32)
    eps = {}
    for a, g_, size in (("ix", "gx", W), ("iy", "gy", H)):
        near_map = (c64[a] >= -1) & (c64[a] <= size)
        e_pix = (c32[a].double() - c64[a]).abs()[near_map]
        e_norm = ((c32[g_].double() - c64[g_]).abs() * (size - 1) / 2)[near_map]              # (in pixels as well)
        eps[a] = max(e_pix.max().item() if e_pix.numel() else 0.0, e_norm.max().item() if e_norm.numel() else 0.0)
    case["coord_error"] = eps
    near_decision = torch.zeros_like(c64["inside"])
    for a, size in (("ix", W), ("iy", H)):
        t, m = c64[a], 4 * eps[a]
        frac = t - t.floor()
        near_decision |= ((frac - 0.5).abs() <= m) & (t > -m) & (t < size - 1 + m)            # a half-integer, where the clamp leaves it one
        near_decision |= (t.abs() <= m) | ((t - (size - 1)).abs() <= m)                       # gx, gy = -1 and +1
    case["skip_voxel"] = near_decision.any(0).reshape(D, Hp, Wp)
    case["excluded_voxels"] = case["skip_voxel"].double().mean().item()
    assert case["excluded_voxels"] <= EXCLUDED_CAP, "%s: %.2f %% of the voxels excluded" % (name, 100 * case["excluded_voxels"])
    case["g_variance"] = case["g_variance"] * (~case["skip_voxel"]).double()
    case["census"] = dict(in_view=int(c64["inside"].sum()), outside=int((~c64["inside"]).sum()),
                          clamped=int(((c64["ix"] < 0) | (c64["ix"] > W - 1) | (c64["iy"] < 0) | (c64["iy"] > H - 1)).sum()))
    # ---- depth regression: pixels whose E[d] is next to an integer, or whose window sum is next to 1
    steps = torch.arange(D).view(D, 1, 1)
    logits = case["prob_pre"] if case["prob_init"] is None else case["prob_pre"] + case["prob_init"]
    p64, p32 = torch.softmax(logits, 0), torch.softmax(logits.float(), 0)
    e64, e32 = (p64 * steps.double()).sum(0), (p32 * steps.float()).sum(0)
    case["e_error"] = (e32.double() - e64).abs().max().item()
    di = e64.long().clamp(0, D - 1)
    pp = torch.cat([torch.zeros(1, Hp, Wp, dtype=F64), p64, torch.zeros(2, Hp, Wp, dtype=F64)], 0)
    w64 = torch.gather(pp[0:D] + pp[1:D + 1] + pp[2:D + 2] + pp[3:D + 3], 0, di.unsqueeze(0)).squeeze(0)
    skip = ((e64 - torch.round(e64)).abs() <= 4 * case["e_error"]) | ((w64 - 1).abs() <= 4 * 2.0 ** -23)
    case["skip_pixel"] = skip[pad:Hp - pad, pad:Wp - pad]
    case["excluded_pixels"] = case["skip_pixel"].double().mean().item()
    assert case["excluded_pixels"] <= EXCLUDED_CAP, "%s: %.2f %% of the pixels excluded" % (name, 100 * case["excluded_pixels"])
    case["g_confidence"] = case["g_confidence"] * (~case["skip_pixel"]).double()
    return case


CV_OUTPUTS = ("variance", "count", "g_feats")
DR_OUTPUTS = ("prob_volume", "depth", "confidence", "g_prob_pre")


def distances(case, ref, got):
    """Max distance from the float64 reference per output, over what is compared: variance and count off the excluded voxels, confidence off the
    excluded pixels, everything else on every element.  `ref`, `got`: dicts of the outputs present."""
    out = {}
    for k, r in ref.items():
        d = (got[k].double().reshape(r.shape) - r).abs()
        if k in ("variance", "count"):
            d = d * (~case["skip_voxel"]).double()
        if k == "confidence":
            d = d * (~case["skip_pixel"]).double()
        out[k] = d.max().item()
    return out


@functools.lru_cache(maxsize=None)
def continuous(name):
    """(case, float64 reference {output: tensor}, the float32 oracle's own distances, max|reference| per output), built once per process."""
    case = continuous_case(name, seed=2000 + CONTINUOUS_NAMES.index(name), **CONTINUOUS_SPECS[name])
    ref = dict(zip(CV_OUTPUTS, cv_reference(case)))
    ref.update(zip(DR_OUTPUTS, dr_reference(case)[:4]))
    f32 = dict(zip(CV_OUTPUTS, cv_reference(case, F32)))
    f32.update(zip(DR_OUTPUTS, dr_reference(case, F32)[:4]))
    scale = {k: v.abs().max().item() for k, v in ref.items()}
    return case, ref, distances(case, ref, f32), scale
