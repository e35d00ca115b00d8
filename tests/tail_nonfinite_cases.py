"""Cases and CPU references for the non-finite tests of the renderer's ray tail: compositing, inverse-CDF re-sampling, the sorted merge and the
merged compositing (tests/test_tail_nonfinite_host.py, tests/test_hip_tail_nonfinite.py).

A case is a small batch (n <= 16 rays) of ordinary random rows in which some rays carry one poison each; case["clean"] holds the same batch
before the poison went in, case["poisoned"] the bool mask of the rays that differ.  A ray is one wave on every route, so the clean rays of the
poisoned batch must come out bit-identical to the same rays of the clean batch.

Position classes of a poison inside its row: "first", "last", "inside" (the second element of a lane's run; with one element per lane an element
in the middle of the row) and "boundary" (the first element of a lane's run: index 64 of a row a wave strides over, index k * E of a compositing
row with E samples per lane; rows too short for one take the middle).

RE-SAMPLING.  Row lengths are the smallest that reach each code path of csrc/sample_pdf_device.h: L = 5 bin edges (4 weights: the scalar row sum),
9 (8 weights: the 8-lane sum), 70 (more than one 64-lane scan chunk), 130 (past the 128-bin instantiation); M = 7 and 65 draws; in the
from_coarse form S = 6, 66 and 132 coarse depths (S - 1 bin edges).  Groups of poison:
  weights   one NaN, one +inf, one NaN next to exact zeros (each at the four positions), all NaN
  depths    one NaN bin edge / coarse depth at the four positions, +inf as the last one
  draws     per-ray unsorted rows: one NaN draw at the four positions; u = 1.0 exactly, u > 1 and u < 0 at first and last
  shared    ONE sorted row of draws for all rays (u_stride = 0), linspace(0, 1, M) whose last entry is 1.0 exactly; the poison is a NaN weight, so
            the clean rays take the merge's binary-search branch and the poisoned ones its counting branch
References: cdf, inds and samples are the reference's own lines run by torch on the CPU (fuzz_sampling.torch_cpu_sample_pdf); on the clean rays
oracle.sample_pdf, which restates ATen's accumulation order, must give the same bits (asserted by the host test).  z_sorted is
torch.sort(cat(samples, z_merge)), NaN last; which NaN payload sits in which NaN slot is free.  The oracle's counting form of inds (#{cdf <= u})
is NOT used on poisoned rows: it disagrees with torch.searchsorted under NaN.

COMPOSITING.  S = 3, 65, 257, 1024: the lane splits E = 1, 2, 8, 16 of composite_lane_samples (65 and 257 end in a ragged lane).  Groups:
  sigma     NaN density, +inf density at the four positions                                            (both variants)
  colour_nan, colour_inf   NaN in one colour channel; +inf colour under a zero weight (density 0 there)    (both variants)
  geometry  helpers variant only: a zero-length interval under +inf density (inf * 0) at the four positions, a NaN ray direction
The reference is the float64 oracle of tests/composite_cases.py on the poisoned rows.  NaN, +inf and -inf must sit on the same elements;
finite elements are held to composite_cases.bars() -- 4 x the float32 oracle's own distance from the float64 one on that module's continuous
cases, whose value ranges these rows share (densities 0.25 .. 1.75, colours in [-1, 2], depths in [1, 4]).  Every element of every ray is
compared: the "kept rays" filter of composite_cases.fwd_distances is not applied.  A candidate case on which the float32 and float64 oracles
themselves disagree about a non-finite position is not a case: DROPPED names it with the reason, and the host test asserts both halves."""
import functools

import numpy as np
import torch

import composite_cases as CC
from fuzz_sampling import torch_cpu_sample_pdf
from oracle import ucnerf_oracle as O

NAN, INF = float("nan"), float("inf")
F32, F64 = torch.float32, torch.float64
POSITIONS = ("first", "last", "inside", "boundary")


def position(length, cls, E=None):
    """Index of position class `cls` in a row of `length` elements; E: samples per lane of a compositing row (None: a row a wave strides over)."""
    if cls == "first":
        return 0
    if cls == "last":
        return length - 1
    if E is None:
        return {"inside": max(length // 3, min(1, length - 1)), "boundary": 64 if length > 64 else length // 2}[cls]
    k = max(1, (length // E) // 2)                                          # a lane in the middle of the row
    if cls == "boundary":
        return min(k * E, length - 1)
    return min(k * E + 1, length - 1)


# ------------------------------------------------------------------------------------------------ the kernels' dispatch, restated
def pdf_instantiation(n_bins, n_merge, n_samples):
    """PdfShared<MAXB, MAXS> a launch takes (csrc/sample_pdf.hip)."""
    return (128, 512) if n_bins <= 128 and n_merge + n_samples <= 512 else (1024, 2048)


def composite_lane_samples(S):
    e = (S + 63) // 64
    return (1 if e < 1 else e) if e <= 4 else 8 if e <= 8 else 16


def sum_path(n_weights):
    return "scalar" if n_weights < 8 else "lanes8"


# ------------------------------------------------------------------------------------------------ re-sampling cases
PDF_L = (5, 9, 70, 130)
PDF_M = (7, 65)
PDF_S = (6, 66, 132)
PDF_GROUPS = ("weights", "depths", "draws", "shared")
N_MERGE_BINS = 9                                    # length of the second sorted list of the `bins` form


def _pdf_plan(group):
    """[(kind, position class or None)] -- one poisoned ray each -- and the number of clean rays that follow them."""
    if group == "weights":
        return [(k, c) for k in ("w_nan", "w_inf", "w_nan_zeros") for c in POSITIONS] + [("w_all_nan", None)], 3
    if group == "depths":
        return [("z_nan", c) for c in POSITIONS] + [("z_inf_last", "last")], 5
    if group == "draws":
        return [("u_nan", c) for c in POSITIONS] + [(k, c) for k in ("u_one", "u_above", "u_below") for c in ("first", "last")], 4
    return [("w_nan", c) for c in POSITIONS], 4


def pdf_names():
    out = []
    for g in PDF_GROUPS:
        out += ["bins_L%d_M%d_%s" % (L, M, g) for L in PDF_L for M in PDF_M]
        out += ["coarse_S%d_M%d_%s" % (S, M, g) for S in PDF_S for M in PDF_M]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pdf_case(name):
    form, a, b, group = name.split("_", 3)
    from_coarse, size, M = form == "coarse", int(a[1:]), int(b[1:])
    plan, n_clean = _pdf_plan(group)
    n = len(plan) + n_clean
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    rnd = lambda *s: torch.rand(*s, generator=gen)      # noqa: E731
    if from_coarse:
        S = size
        L = S - 1
        z = torch.sort(0.5 + 4.0 * rnd(n, S), -1)[0]
        w = rnd(n, S) * 0.2                               # the S coarse weights: w[1:-1] are the S - 2 the re-sampling reads
        w_lo, w_len, d_len = 1, S - 2, S
    else:
        L = size
        z = torch.sort(rnd(n, L) * 4.0, -1)[0]            # the bin edges
        w = rnd(n, L - 1) * 0.2
        w_lo, w_len, d_len = 0, L - 1, L
    shared = group == "shared"
    u = torch.linspace(0., 1., M) if shared else rnd(n, M)
    zm = z if from_coarse else torch.sort(rnd(n, N_MERGE_BINS) * 4.0, -1)[0]
    clean = dict(w=w.clone(), z=z.clone(), u=u.clone())
    rays = []
    for r, (kind, cls) in enumerate(plan):
        if kind.startswith("w_"):
            i = w_lo + (position(w_len, cls) if cls else 0)
            if kind == "w_all_nan":
                w[r] = NAN
            elif kind == "w_inf":
                w[r, i] = INF
            else:
                if kind == "w_nan_zeros":
                    w[r, ::2] = 0.0
                w[r, i] = NAN
        elif kind == "z_nan":
            z[r, position(d_len, cls)] = NAN
        elif kind == "z_inf_last":
            z[r, d_len - 1] = INF
        else:
            u[r, position(M, cls)] = {"u_nan": NAN, "u_one": 1.0, "u_above": 1.5, "u_below": -0.25}[kind]
        rays.append(dict(ray=r, kind=kind, cls=cls))
    poisoned = torch.zeros(n, dtype=torch.bool)
    poisoned[:len(plan)] = True
    case = dict(name=name, form=form, group=group, n=n, L=L, M=M, S=size if from_coarse else None, from_coarse=from_coarse, shared=shared,
                w=w, z=z, u=u, zm=z if from_coarse else zm, clean=clean, rays=rays, poisoned=poisoned, n_merge=zm.shape[1])
    case["clean"]["zm"] = clean["z"] if from_coarse else zm
    return case


def pdf_inputs(case, which="poisoned"):
    """(bins [n,L], weights [n,L-1], u [n,M]) as the reference's lines take them."""
    src = case if which == "poisoned" else case["clean"]
    w, z, u = src["w"], src["z"], src["u"]
    if case["from_coarse"]:
        bins, w = 0.5 * (z[:, :-1] + z[:, 1:]), w[:, 1:-1].contiguous()
    else:
        bins = z
    return bins, w, (u.expand(case["n"], case["M"]).contiguous() if case["shared"] else u)


@functools.lru_cache(maxsize=None)
def pdf_reference(name, which="poisoned"):
    """dict(samples, inds, cdf, cat, z_sorted) by torch on the CPU."""
    case = pdf_case(name)
    bins, w, u = pdf_inputs(case, which)
    samples, inds, cdf = torch_cpu_sample_pdf(bins, w, u)
    cat = torch.cat([samples, (case if which == "poisoned" else case["clean"])["zm"]], -1)
    return dict(samples=samples, inds=inds, cdf=cdf, cat=cat, z_sorted=torch.sort(cat, -1)[0])


def oracle_pdf(name, which="poisoned"):
    bins, w, u = pdf_inputs(pdf_case(name), which)
    return O.sample_pdf(bins, w, u)


def same_bits(a, b):
    """NaN on the same elements, every other element bit-equal, the sign of zero included."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    an, bn = a != a, b != b
    if not torch.equal(an, bn):
        return False
    a, b = torch.where(an, torch.zeros_like(a), a), torch.where(bn, torch.zeros_like(b), b)
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def first_difference(a, b):
    a, b = a.cpu(), b.cpu()
    bad = ~((a == b) | ((a != a) & (b != b)))
    idx = bad.nonzero()
    return "%d of %d differ, first at %s: %r against %r" % (len(idx), a.numel(), idx[0].tolist(), a[tuple(idx[0])].item(), b[tuple(idx[0])].item()) \
        if len(idx) else "signs of zero or shapes differ"


# ------------------------------------------------------------------------------------------------ the device's search and merge, restated
def search_restated(cdf, u, fixed=True):
    """The binary search of sample_pdf_ray over rows cdf [n,L] and draws u [n,M]: steps on !(cdf[mid] > u) (fixed: ATen's upper bound) or on
    cdf[mid] <= u (the form it had)."""
    cdf, u = cdf.numpy(), u.numpy()
    n, L = cdf.shape
    out = np.zeros(u.shape, dtype=np.int64)
    for r in range(n):
        for m in range(u.shape[1]):
            lo, hi = 0, L
            while lo < hi:
                mid = (lo + hi) >> 1
                right = (not cdf[r, mid] > u[r, m]) if fixed else bool(cdf[r, mid] <= u[r, m])
                lo, hi = (mid + 1, hi) if right else (lo, mid)
            out[r, m] = lo
    return torch.from_numpy(out)


def merge_rank_restated(cat, M, fixed=True):
    """merge_rank of sample_pdf_ray for rows cat [n, M + n_merge] = cat(samples, z_merge): the binary-search branch when both lists are sorted,
    else the counting branch; fixed=False restates both as they were before NaN had a rank."""
    x = cat.numpy()
    n, tot = x.shape
    out = np.zeros((n, tot), dtype=np.int64)
    idx = np.arange(tot)
    for r in range(n):
        row = x[r]
        with np.errstate(invalid="ignore"):
            pair = row[:-1] <= row[1:]
            if M - 1 < tot - 1 and M >= 1:
                pair[M - 1] = (not (np.isnan(row[M - 1]) or np.isnan(row[M]))) if fixed else True
            if pair.all():
                for i in range(tot):                                        # the device's own loops (numpy's searchsorted has a rule for NaN)
                    lo, hi = (M, tot) if i < M else (0, M)
                    while lo < hi:
                        mid = (lo + hi) >> 1
                        lo, hi = (mid + 1, hi) if (row[mid] < row[i] if i < M else row[mid] <= row[i]) else (lo, mid)
                    out[r, i] = i + (lo - M) if i < M else (i - M) + lo
                continue
            less = row[None, :] < row[:, None]                              # [i, j]: v_j < x_i
            tie = (row[None, :] == row[:, None]) & (idx[None, :] < idx[:, None])
            rank = (less | tie).sum(1)
            if fixed:
                xn = np.isnan(row)
                rank = rank + (xn[:, None] & (~xn[None, :] | (idx[None, :] < idx[:, None]))).sum(1)
        out[r] = rank
    return torch.from_numpy(out)


def is_permutation(rank):
    rank = rank.cpu().long()
    return torch.equal(torch.sort(rank, -1)[0], torch.arange(rank.shape[1]).expand_as(rank))


def placed(cat, rank):
    """cat scattered by rank (slots no rank names keep -7)."""
    return torch.full_like(cat, -7.0).scatter_(-1, rank.cpu().long().clamp(0, cat.shape[1] - 1), cat)


# ------------------------------------------------------------------------------------------------ compositing cases
COMP_S = (3, 65, 257, 1024)
COMP_GROUPS = {0: ("sigma", "colour_nan", "colour_inf"), 1: ("sigma", "colour_nan", "colour_inf", "geometry")}
# candidate name -> why it is not a case (see the module docstring).  Both: the density gradient of the sample under the +inf colour is
# gw_i T_i - ... with gw_i = g_rgb * inf; 128 and more samples of density >= 0.25 in front of it take T_i below the smallest float32 denormal,
# so the float32 oracle has inf * 0 = NaN where the float64 oracle (T_i ~ 1e-56 and smaller, not 0) has -inf.  The forward of the same rows
# stays covered by helpers_S257_colour_inf / helpers_S1024_colour_inf, the lane splits of the backward by colour_nan and sigma.
DROPPED = {"live_S257_colour_inf": "float32 transmittance underflows to 0 in front of the +inf colour: g_density NaN in float32, -inf in float64",
           "live_S1024_colour_inf": "float32 transmittance underflows to 0 in front of the +inf colour: g_density NaN in float32, -inf in float64"}


def _comp_plan(group):
    if group == "sigma":
        return [(k, c) for k in ("sigma_nan", "sigma_inf") for c in POSITIONS], 4
    if group in ("colour_nan", "colour_inf"):
        return [("colour_nan" if group == "colour_nan" else "colour_inf_zero_weight", c) for c in POSITIONS], 4
    return [("zero_interval_inf_sigma", c) for c in POSITIONS] + [("rays_d_nan", None)], 4


def comp_candidates():
    return tuple("%s_S%d_%s" % ("helpers" if v else "live", S, g) for v in (0, 1) for S in COMP_S for g in COMP_GROUPS[v])


def comp_names():
    return tuple(c for c in comp_candidates() if c not in DROPPED)


@functools.lru_cache(maxsize=None)
def comp_case(name):
    vname, s, group = name.split("_", 2)
    variant, S = int(vname == "helpers"), int(s[1:])
    E = composite_lane_samples(S)
    plan, n_clean = _comp_plan(group)
    n = len(plan) + n_clean
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    rnd = lambda *s_: torch.rand(*s_, generator=gen)      # noqa: E731
    case = dict(name=name, kind="nonfinite", variant=variant, n=n, S=S, E=E, group=group)
    # drawn as composite_cases.continuous_case draws its rows (the density scale 1 of the live variant), so that its bars are bars for these
    sig = 0.25 + 1.5 * rnd(n, S)
    case["z"] = torch.sort(1.0 + 3.0 * rnd(n, S), -1)[0]
    case["u"] = rnd(n, S)
    if variant:
        case["raw"] = 8.0 * rnd(n, S, 4) - 4.0
        case["noise"] = torch.randn(n, S, generator=gen)
        case["rays_d"] = torch.randn(n, 3, generator=gen) * 1.7
        case["raw"][:, -1, 3] = case["raw"][:, -1, 3].abs() + 0.5          # the 1e10 last distance closes every ray
        case["noise"][:, -1] = case["noise"][:, -1].abs()
    else:
        case["raw"] = torch.cat([3.0 * rnd(n, S, 3) - 1.0, sig[..., None]], -1)
        case.update(g_rgb=torch.randn(n, 3, generator=gen), g_depth=torch.randn(n, generator=gen), g_acc=torch.randn(n, generator=gen),
                    g_weights=torch.randn(n, S, generator=gen))
    keys = ("raw", "z", "rays_d", "noise")
    case["clean"] = {k: case[k].clone() for k in keys if k in case}
    rays = []
    for r, (kind, cls) in enumerate(plan):
        i = position(S, cls, E) if cls else 0
        if kind == "sigma_nan":
            case["raw"][r, i, 3] = NAN
        elif kind == "sigma_inf":
            case["raw"][r, i, 3] = INF
        elif kind == "colour_nan":
            case["raw"][r, i, r % 3] = NAN
        elif kind == "colour_inf_zero_weight":
            case["raw"][r, i, r % 3] = INF
            case["raw"][r, i, 3] = 0.0                                    # alpha = 0: the weight is exactly 0 (live variant; helpers: relu(0 + noise))
            if variant:
                case["noise"][r, i] = -1.0
        elif kind == "zero_interval_inf_sigma":
            i = min(i, S - 2)                                             # an interval, not a sample: the last one is the 1e10 behind the ray
            case["z"][r, i + 1] = case["z"][r, i]
            case["raw"][r, i, 3] = INF
        else:
            case["rays_d"][r, 1] = NAN
        rays.append(dict(ray=r, kind=kind, cls=cls, index=i))
    case["rays"] = rays
    case["poisoned"] = torch.zeros(n, dtype=torch.bool)
    case["poisoned"][:len(plan)] = True
    return case


def clean_of(case):
    out = dict(case)
    out.update(case["clean"])
    return out


def classes(t):
    """int8 tensor: 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.detach()
    return (t != t).to(torch.int8) + 2 * (t == INF).to(torch.int8) + 3 * (t == -INF).to(torch.int8)


@functools.lru_cache(maxsize=None)
def comp_reference(name, white):
    """(float64 outputs, float32 outputs, float64 g_raw or None, float32 g_raw or None) of the oracle on the poisoned rows; the backward (live
    variant) takes all four upstream gradients together."""
    case = comp_case(name)
    f64, f32 = CC.forward(case, F64, white), CC.forward(case, F32, white)
    g64 = g32 = None
    if case["variant"] == 0:
        g64, g32 = CC.backward(case, F64, white, CC.TARGETS), CC.backward(case, F32, white, CC.TARGETS)
    return f64, f32, g64, g32


def oracle_disagreements(name):
    """Outputs on which the float32 and float64 oracles put NaN / +inf / -inf on different elements."""
    out = []
    for white in (False, True):
        f64, f32, g64, g32 = comp_reference(name, white)
        out += ["%s white=%s" % (k, white) for k in f64 if not torch.equal(classes(f64[k]), classes(f32[k]))]
        if g64 is not None and not torch.equal(classes(g64), classes(g32)):
            out.append("g_raw white=%s" % white)
    return out


def held(got, ref64, bar, what):
    """Failure lines: NaN / +inf / -inf of `got` on other elements than the float64 reference's, or a finite element further than `bar` from it.
    Every element counts."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    cg, cr = classes(got), classes(ref64)
    if not torch.equal(cg, cr):
        bad = (cg != cr).nonzero()
        return ["%s: %d non-finite positions differ, first at %s: got %r, reference %r"
                % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])].item(), ref64[tuple(bad[0])].item())]
    fin = cr == 0
    d = (got[fin] - ref64[fin]).abs().max().item() if bool(fin.any()) else 0.0
    return [] if d <= bar else ["%s: %.3e > bar %.3e" % (what, d, bar)]


def comp_fwd_failures(got, name, white, what):
    f64 = comp_reference(name, white)[0]
    bars, fails = CC.bars(), []
    assert set(got) == set(f64), (set(got), set(f64))
    for k, r in f64.items():
        fails += held(got[k], r, bars[k], "%s %s %s white=%s" % (name, what, k, white))
    return fails


def comp_bwd_failures(g_raw, name, white, what):
    g64 = comp_reference(name, white)[2]
    bars = CC.bars()
    g = g_raw.detach().cpu()
    return held(g[..., :3], g64[..., :3], bars["g_colour"], "%s %s g_colour white=%s" % (name, what, white)) + \
        held(g[..., 3], g64[..., 3], bars["g_density"], "%s %s g_density white=%s" % (name, what, white))
