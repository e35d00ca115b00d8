"""Cases, float64 restatement and bars for the gradient fold of the compositing's extra maps (ucnerf_composite_fold_grads, ops.composite_maps,
ops.composite_merged_maps): tests/test_composite_maps_host.py and tests/test_hip_composite_maps.py.

The reference is oracle.ucnerf_oracle.raw2outputs_live with torch autograd through ALL of its maps -- var (torch.var, unbiased), disp
(1 / maximum(1e-10, depth / acc)) and wu = sum_i w_i u_i -- in float64.  fold64() restates the kernel's formulas (include/ucnerf_hip.h); the
host test shows that fold64 followed by the oracle's backward through rgb / depth / acc / weights alone is that autograd.

Losses are random linear functionals: sum(map * g_map) with g_map ~ N(0, 1), of one extra map alone (COMBOS_ALONE) or of all seven maps
(ALL).  g_var is N(0, 1) * S: d var / d w_i = 2 (w_i - mean) / (S - 1) is of the size of a weight over S, and the factor keeps what the
functional sends to a weight at the size of the weight instead of vanishing below the other maps' share as S grows.

Densities: ray r has an expected optical depth TAUS[r % 4] spread over its S samples (sigma_i = tau / S * (0.25 + 1.5 rand)), every fifth ray a
surface (three samples of density + 5) on top: acc stays above ACC_MIN on every ray (asserted), so disp is compared on EVERY ray and no
element of any gradient is left out of a comparison.

Bars.  distance = max |got - float64 reference| over a whole gradient (colour channels, density channel, g_u).  BASE[combo][name] is the
largest distance of the float32 ORACLE (the same autograd, run in float32 on the CPU) from the float64 one over all cases -- measured, and
re-measured by the host test, which holds every constant below to the measurement (another CPU sums a row in other pieces: its
measurement may be up to a quarter above the constant, which makes the bar stricter, and not below a tenth of it).  The device gets FACTOR = 4
times that: a wave's shuffle reductions and per-lane products against sequential sums and a sequential cumprod, device against host expf."""
import functools
import warnings

import torch

import composite_cases as CC
import composite_merged_bwd_cases as MB
from oracle import ucnerf_oracle as O

F32, F64 = torch.float32, torch.float64
S_VALUES = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 257, 513, 1024)
N_VALUES = (1, 5, 67)
TAUS = (0.3, 1.0, 3.0, 10.0)
ACC_MIN = 1e-3
MAPS = ("rgb", "depth", "acc", "weights", "disp", "var", "wu")
EXTRA = ("var", "disp", "wu")
COMBOS_ALONE = tuple((m,) for m in EXTRA)
ALL = MAPS
DIST_NAMES = ("g_colour", "g_density", "g_u")
FACTOR = 4.0
# measured on the CPU (float32 oracle against float64 oracle, worst over dense_names() + merged_specs()), rounded up to two digits
BASE = {
    "var": dict(g_colour=0.0, g_density=8.1e-06, g_u=0.0),
    "disp": dict(g_colour=0.0, g_density=1.4e-05, g_u=0.0),
    "wu": dict(g_colour=0.0, g_density=3.4e-06, g_u=2.4e-06),
    "all": dict(g_colour=3.9e-06, g_density=3.2e-05, g_u=2.4e-06),
}


def combo_name(combo):
    return combo[0] if len(combo) == 1 else "all"


def combos_of(S):
    """The losses a case of S samples has: var exists from S = 2 on."""
    alone = tuple(c for c in COMBOS_ALONE if S >= 2 or c != ("var",))
    return alone + (tuple(m for m in ALL if S >= 2 or m != "var"),)


def bar(combo, name):
    return FACTOR * BASE[combo_name(combo)][name]


# ------------------------------------------------------------------------------------------------ the fold in float64
def fold64(weights, depth, acc, u=None, g_var=None, g_disp=None, g_wu=None, g_depth=None, g_acc=None, g_weights=None):
    """(g_depth', g_acc', g_weights', g_u) of ucnerf_composite_fold_grads in the dtype of `weights` (None upstream = zero; g_u None without u)."""
    n, S = weights.shape
    zero = lambda g, like: torch.zeros_like(like) if g is None else g.to(weights.dtype)      # noqa: E731
    gd, ga, gw = zero(g_depth, depth), zero(g_acc, acc), zero(g_weights, weights)
    if g_var is not None:
        assert S >= 2
        gw = gw + g_var[:, None] * (2.0 * (weights - weights.sum(-1, keepdim=True) / S) / (S - 1))
    if g_wu is not None:
        gw = gw + g_wu[:, None] * u
    if g_disp is not None:
        q = depth / acc
        live = (q > 1e-10) & torch.isfinite(q)
        d = 1.0 / torch.where(live, q, torch.ones_like(q))
        t = d * d / acc
        gd = gd + torch.where(live, g_disp * -t, torch.zeros_like(q))
        ga = ga + torch.where(live, g_disp * (t * q), torch.zeros_like(q))
    g_u = None if u is None else (g_wu[:, None] * weights if g_wu is not None else torch.zeros_like(weights))
    return gd, ga, gw, g_u


# ------------------------------------------------------------------------------------------------ cases
def dense_case(S, n):
    gen = torch.Generator().manual_seed(9000 + 7 * S + n)
    rnd = lambda *s: torch.rand(*s, generator=gen)                                # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=gen)                                # noqa: E731
    tau = torch.tensor(TAUS)[torch.arange(n) % 4]
    sig = tau[:, None] / S * (0.25 + 1.5 * rnd(n, S))
    for r in range(4, n, 5):                                                      # a surface: three dense samples somewhere on the ray
        i0 = int(torch.randint(0, max(S - 2, 1), (1,), generator=gen))
        sig[r, i0:i0 + 3] += 5.0
    case = dict(name="maps_S%d_n%d" % (S, n), S=S, n=n, white=bool((S + n) % 2))
    case["raw"] = torch.cat([3.0 * rnd(n, S, 3) - 1.0, sig[..., None]], -1)
    case["z"] = torch.sort(1.0 + 3.0 * rnd(n, S), -1)[0]
    case["u"] = rnd(n, S)
    case.update(g_rgb=rn(n, 3), g_depth=rn(n), g_acc=rn(n), g_weights=rn(n, S), g_disp=rn(n), g_var=rn(n) * S, g_wu=rn(n))
    return case


def dense_names():
    return tuple("maps_S%d_n%d" % (S, n) for S in S_VALUES for n in N_VALUES)


def merged_specs():
    """(na, nb) of the issue's four kinds: everything in b, everything in a, one row in a, and the renderer's 128 new + 64 coarse rows."""
    return ((0, 65), (65, 0), (0, 2), (2, 0), (1, 1), (1, 64), (1, 192), (128, 64))


def losses(outs, case, combo, dtype):
    return sum((outs[m] * case["g_" + m].to(dtype)).sum() for m in combo)


def oracle_maps(raw, z, u, white):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                          # (torch.var over one sample, S = 1: not used)
        rgb, disp, acc, w, depth, _, var = O.raw2outputs_live(raw, z, white)
    return dict(rgb=rgb, depth=depth, acc=acc, weights=w, disp=disp, var=var, wu=(w * u).sum(-1))


def reference(case, dtype, combo):
    """(g_raw [n,S,4], g_u [n,S]) by torch autograd through every map of the oracle in `dtype`."""
    raw = case["raw"].to(dtype).clone().requires_grad_(True)
    u = case["u"].to(dtype).clone().requires_grad_(True)
    losses(oracle_maps(raw, case["z"].to(dtype), u, case["white"]), case, combo, dtype).backward()
    return raw.grad.detach(), (torch.zeros_like(u) if u.grad is None else u.grad.detach())


def folded_reference(case, dtype, combo):
    """The same by the route the device takes: fold64 on the oracle's forward outputs, then the oracle's backward through rgb, depth, acc and
    weights ALONE, on the folded gradients."""
    raw = case["raw"].to(dtype).clone().requires_grad_(True)
    o = oracle_maps(raw, case["z"].to(dtype), case["u"].to(dtype), case["white"])
    g = {m: (case["g_" + m].to(dtype) if m in combo else None) for m in MAPS}
    gd, ga, gw, g_u = fold64(o["weights"].detach(), o["depth"].detach(), o["acc"].detach(), case["u"].to(dtype), g["var"], g["disp"], g["wu"],
                             g["depth"], g["acc"], g["weights"])
    outs, grads = [o["depth"], o["acc"], o["weights"]], [gd, ga, gw]
    if g["rgb"] is not None:
        outs.append(o["rgb"])
        grads.append(g["rgb"])
    torch.autograd.backward(outs, grads)
    return raw.grad.detach(), g_u


def distances(g_raw, g_u, ref_raw, ref_u):
    d = CC.bwd_distances(g_raw, ref_raw)
    d["g_u"] = (g_u.double().reshape(ref_u.shape) - ref_u).abs().max().item()
    return d


@functools.lru_cache(maxsize=None)
def dense(name):
    """(case, {combo: float64 (g_raw, g_u)}, {combo: the float32 oracle's distances}), built once per process; acc > ACC_MIN asserted."""
    S, n = (int(x[1:]) for x in name.split("_")[1:])
    case = dense_case(S, n)
    acc = oracle_maps(case["raw"].double(), case["z"].double(), case["u"].double(), False)["acc"]
    assert float(acc.min()) > ACC_MIN, "%s: acc %.3e" % (name, float(acc.min()))
    ref, dist = {}, {}
    for combo in combos_of(S):
        ref[combo] = reference(case, F64, combo)
        assert bool(torch.isfinite(ref[combo][0]).all()) and bool(torch.isfinite(ref[combo][1]).all()), name
        dist[combo] = distances(*reference(case, F32, combo), *ref[combo])
    return case, ref, dist


@functools.lru_cache(maxsize=None)
def merged(na, nb):
    """(m, case, {combo: float64 (g_raw_a, g_raw_b, g_u)}, {combo: the float32 oracle's distances}): dense_case(na + nb, 5) with its rows handed
    out to raw_a / raw_b by a random rank; u, the maps and their gradients stay in merged order."""
    case = dense_case(na + nb, 5)
    case["name"] = "maps_merged_%d_%d" % (na, nb)
    m = MB.split(case, na, "random")
    ref, dist = {}, {}
    for combo in combos_of(na + nb):
        g_raw, g_u = reference(case, F64, combo)
        ref[combo] = MB.unmerge(g_raw, m["rank"], na) + (g_u,)
        dist[combo] = distances(*reference(case, F32, combo), g_raw, g_u)
    return m, case, ref, dist


@functools.lru_cache(maxsize=None)
def measured_base():
    """{combo name: {distance name: the float32 oracle's largest distance from the float64 oracle over every case}}."""
    worst = {c: dict.fromkeys(DIST_NAMES, 0.0) for c in BASE}
    for dist in [dense(name)[2] for name in dense_names()] + [merged(na, nb)[3] for na, nb in merged_specs()]:
        for combo, d in dist.items():
            for k, v in d.items():
                worst[combo_name(combo)][k] = max(worst[combo_name(combo)][k], v)
    return worst


def over_the_bar(dist, combo, what):
    return ["%s %s: %.3e > bar %.3e" % (what, k, v, bar(combo, k)) for k, v in dist.items() if not v <= bar(combo, k)]


# ------------------------------------------------------------------------------------------------ exact cases
EXACT_S = (2, 3, 64, 65, 129, 193, 257, 513, 1024)       # every lane split: 1, 1, 1, 2, 3, 4, 8, 16, 16 samples per lane


def expected_fold_one_hot(w, u, g_var, g_wu, g_weights=None):
    """(g_weights', g_u) in float32, operation by operation as the header states them, for rows w that are one-hot: the row sum is exactly 1
    in any order, so every step below has one possible float32 result."""
    n, S = w.shape
    assert w.dtype == F32 and bool(((w == 0) | (w == 1)).all()) and bool((w.sum(-1) == 1).all())
    mean = torch.ones(n, 1) / torch.tensor(float(S))
    g = torch.zeros(n, S) if g_weights is None else g_weights.clone()
    g = g + g_var[:, None] * ((2.0 * (w - mean)) / torch.tensor(float(S - 1)))
    g = g + g_wu[:, None] * u
    return g, g_wu[:, None] * w
