"""Cases and float64 reference for the compositing kernels' edge tests (tests/test_composite_cases_host.py, tests/test_hip_composite_edges.py).

The reference is oracle.ucnerf_oracle.raw2outputs_live / raw2outputs_helpers, run in float64 and in float32, with autograd through
raw2outputs_live for the backward.

EXACT ("one-hit") cases.  Densities are 0.0, -0.0 or 200.0 (variant 1: whatever makes relu(sigma + noise) * dist exactly 0 or > 100), so
exp(-.) is exactly 1 or 0 in float32, alpha exactly 0 or 1 and every transmittance factor exactly 1.0f or 1e-10f.  Colours, depths, u and the
upstream gradients are small integers and a ray has at most two opaque samples: at most two nonzero weights (1.0f and 1e-10f), at most three
non-unit factors, so every product and every sum of the float32 computation is a sum / product of at most two non-trivial terms and does not
depend on the association order -- a 64-lane scan, a per-lane loop and a sequential cumprod give the same bits.  check_exact asserts
  * the structure: exponents 0 or > 100, at most two opaque samples per ray, integer inputs, every integer intermediate below 2^24;
  * the float32 oracle's weights equal the closed form (first opaque sample 1.0f, second 1e-10f, everything else 0) on every ray;
  * the float32 oracle equals the float64 oracle rounded to float32 on rgb, depth, acc, disp, weights, wu, both backgrounds, for every ray
    whose opaque samples all lie below position 256, and is within 2^-21 relative of it everywhere.
The last split is forced by the oracle itself: in float64 a transparent sample's factor is 1 + 1e-10, not 1, and (1 + 1e-10)^h passes half a
float32 ulp of 1e-10f (3.5e-8 relative) at h = 347 and half an ulp of 1 at h = 597.  A float32 computation -- the reference's, the kernels' --
has the factor at exactly 1.0f; past those positions the float64 result rounded to float32 is one ulp above the float32 result, which is what
the kernels must produce.  The expected values of an exact case are therefore the float32 oracle's, with the closed-form weights as their
independent check.  Colours and u are nonzero integers: the float64 oracle's 1 - acc = -h e-10 and its 1e-10 (1 + h e-10) second weight
would otherwise be the whole value of an output instead of vanishing below its leading integer.  `var` is not association-free: it goes under
the continuous bar.

Exact backward.  expected_g_raw gives the float32 closed form and the mask of the entries it is exact on, with gw_i = g_rgb . rgb_i + g_depth z_i
+ g_acc' + g_weights_i (all integers; g_acc' = g_acc - sum(g_rgb) with a white background):
  colour channels     w_i * g_rgb, on every ray (one rounding where w_i = 1e-10f);
  density channel     (gw_i T_i - (sum_{k>i} gw_k w_k) / f_i) exp(-sigma_i) with T_i in {1, 1e-10f, 1e-20f}, f_i in {1, 1e-10f}, exp(-sigma_i) in
                      {1, 0}: with one opaque sample h that is gw_i - gw_h before it, 0 on it, gw_i * 1e-10f behind it, and gw_i on an empty
                      ray.  The sum has at most two nonzero terms, so each float32 operation of the expression has one possible result.
Every entry is declared exact.  The float64 autograd cannot confirm them to the bit -- before the hit it carries
gw_i (1 + 1e-10)^i - gw_h (1 + 1e-10)^(h-1), which is not 0 where gw_i = gw_h, and is 7e-6 from the integer at |gw| = 400 (measured on the
device: the first version of the test held the two-hit density entries to the continuous bar against the float64 autograd and read 7.3e-6
at S = 192 with g_depth alone, all of it this drift).  check_exact_backward asserts the closed form within 4e-7 * max|gw| of the float64
autograd, which any slip in the closed form (an O(1) error) would miss by six orders of magnitude.

CONTINUOUS cases: random data, 7 rays per case (densities on scales 0.01, 1, 10, 50; an all-zero ray; a ray with 30 % of its samples at 200;
a ray opaque at sample 0), float64 and float32 oracle results, backward targets from the float64 autograd.  The bar of an output name is
4 x the largest distance between the two oracles over all continuous cases (bars()): the margin of tests/gather_cases.py, for the same reason
-- per-lane products and a 64-lane scan against a sequential cumprod, device against host expf.  disp is compared where the float64 acc > 1e-3
(at most one ray in seven left out, asserted), NaN positions must agree."""
import functools
import warnings

import torch

from oracle import ucnerf_oracle as O

F32, F64 = torch.float32, torch.float64
TINY = torch.tensor(1e-10, dtype=F32)                # 1e-10f: the factor behind an opaque sample, and the weight of a second one
FWD_NAMES = ("rgb", "depth", "acc", "disp", "weights", "wu")
HIT_S = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1023, 1024)
HIT_KINDS = ("one", "last", "adjacent")             # one opaque sample at position r; a second on S - 1; a second on r + 1
TARGETS = ("g_rgb", "g_depth", "g_acc", "g_weights")
COMBOS = tuple((t,) for t in TARGETS) + (TARGETS,)   # each upstream gradient alone (the other three null), then all four
DRIFT_FREE = 256                                     # (1 + 1e-10)^256 - 1 = 2.6e-8 < half an ulp of 1e-10f: the float64 oracle still rounds to the float32 result


# ------------------------------------------------------------------------------------------------ references
def forward(case, dtype, white):
    """Oracle outputs of a case in `dtype`: dict rgb, depth, acc, disp, weights, wu (+ var: live variant, S >= 2)."""
    c = lambda k: case[k].to(dtype)      # noqa: E731
    if case["variant"] == 0:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (torch.var over one sample, S = 1: not used)
            rgb, disp, acc, w, depth, _, var = O.raw2outputs_live(c("raw"), c("z"), white)
    else:
        rgb, disp, acc, w, depth = O.raw2outputs_helpers(c("raw"), c("z"), c("rays_d"), c("noise") if "noise" in case else None, white)
        var = None
    out = dict(rgb=rgb, depth=depth, acc=acc, disp=disp, weights=w, wu=(w * c("u")).sum(-1))
    if var is not None and case["S"] >= 2:
        out["var"] = var
    return out


def backward(case, dtype, white, combo, rays=None):
    """g_raw [n,S,4] of the live variant by autograd through the oracle in `dtype`, for the upstream gradients named in `combo`."""
    sel = (lambda t: t) if rays is None else (lambda t: t[rays])      # noqa: E731
    raw = sel(case["raw"]).to(dtype).clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rgb, _, acc, w, depth, _, _ = O.raw2outputs_live(raw, sel(case["z"]).to(dtype), white)
    outs = dict(g_rgb=rgb, g_depth=depth, g_acc=acc, g_weights=w)
    loss = sum((outs[t] * sel(case[t]).to(dtype)).sum() for t in combo)
    loss.backward()
    return raw.grad.detach()


def same_or_both_nan(a, b):
    return bool(((a == b) | ((a != a) & (b != b))).all())


# ------------------------------------------------------------------------------------------------ exact cases
def opaque_mask(case):
    """[n,S] bool from the inputs alone; asserts every exponent is exactly 0 or beyond the float32 underflow of exp (> 100)."""
    if case["variant"] == 0:
        s = case["raw"][..., 3]
        assert bool(((s == 0) | (s == 200)).all()), case["name"]
        return s == 200
    z, S = case["z"], case["S"]
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((case["n"], 1), 1e10, dtype=F32)], -1).double()
    dist = dist * case["rays_d"].double().norm(dim=-1, keepdim=True)
    x = torch.relu(case["raw"][..., 3].double() + case["noise"].double()) * dist
    assert bool(((x == 0) | (x > 100)).all()), case["name"]
    assert tuple(x.shape) == (case["n"], S)
    return x > 100


def closed_form_weights(opaque):
    """First opaque sample of a ray 1.0f, second 1e-10f, everything else 0 (at most two: asserted)."""
    k = opaque.long().cumsum(-1)
    assert int(k.max()) <= 2
    w = torch.zeros(opaque.shape, dtype=F32)
    w[opaque & (k == 1)] = 1.0
    w[opaque & (k == 2)] = TINY
    return w


def _integers(t, bound):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= bound


def check_exact(case):
    """The exactness conditions of the module docstring; returns {white: float32 expected outputs}."""
    name, S = case["name"], case["S"]
    opaque = opaque_mask(case)
    want_w = closed_form_weights(opaque)
    assert _integers(case["z"], 2048) and _integers(case["u"], 8) and bool((case["u"] != 0).all()), name
    if case["variant"] == 0:
        assert _integers(case["raw"][..., :3], 8) and bool((case["raw"][..., :3] != 0).all()), name
    else:
        assert bool((case["raw"][..., :3] == 0).all()), name             # sigmoid(0) = 0.5 exactly
    # every sum the forward forms is bounded by 8 * 2048 * (1 + 1e-10); the backward's integers by check_exact_backward
    assert 2 * 8 * 2048 < 2 ** 24
    last = torch.where(opaque, torch.arange(S).expand_as(opaque), torch.full_like(opaque, -1, dtype=torch.long)).max(-1)[0]      # last opaque position
    confirmable = last < DRIFT_FREE if S > DRIFT_FREE else torch.ones(case["n"], dtype=torch.bool)
    out = {}
    for white in (False, True):
        f32, f64 = forward(case, F32, white), forward(case, F64, white)
        assert torch.equal(f32["weights"], want_w), "%s: float32 oracle weights are not the closed form" % name
        for k in FWD_NAMES:
            a, b = f32[k], f64[k].float()
            assert same_or_both_nan(a[confirmable], b[confirmable]), "%s: float32 oracle != float64 oracle rounded (%s, white=%s)" % (name, k, white)
            fin = a == a
            assert bool(((a != a) == (b != b)).all()) and bool(((a[fin].double() - f64[k][fin]).abs() <= 2.0 ** -21 * f64[k][fin].abs()).all()), (name, k)
        if "var" in f32:
            f32["var64"] = f64["var"]
        out[white] = f32
    case["opaque"], case["confirmable_rays"] = opaque, int(confirmable.sum())
    return out


def expected_g_raw(case, white, combo):
    """(float32 closed-form g_raw [n,S,4], bool mask of the entries declared exact) of an exact live-variant case; see the module docstring."""
    n, S = case["n"], case["S"]
    opaque = case["opaque"]
    w = closed_form_weights(opaque)
    zero3, zero1 = torch.zeros(n, 3), torch.zeros(n)
    g_rgb = case["g_rgb"] if "g_rgb" in combo else zero3
    g_depth = case["g_depth"] if "g_depth" in combo else zero1
    g_acc = case["g_acc"] if "g_acc" in combo else zero1
    if white:
        g_acc = g_acc - g_rgb.sum(-1)
    gw = (case["raw"][..., :3] * g_rgb[:, None, :]).sum(-1) + g_depth[:, None] * case["z"] + g_acc[:, None]      # integers: exact in float32
    if "g_weights" in combo:
        gw = gw + case["g_weights"]
    assert gw.dtype == F32 and _integers(gw, 2 ** 22)                   # (a difference of two stays below 2^24)
    k = opaque.long().cumsum(-1) - opaque.long()                         # opaque samples in front of i: 0, 1 or 2
    T = torch.stack([torch.ones(()), TINY, TINY * TINY])[k]              # transmittance in front of i (1e-20f: one rounding, whatever the order)
    gww = gw * w
    after = torch.flip(torch.cumsum(torch.flip(gww, [1]), 1), [1])       # sum_{k >= i} gw_k w_k: at most two nonzero terms, any order gives the same
    suffix = torch.cat([after[:, 1:], torch.zeros(n, 1)], -1)
    f = torch.where(opaque, TINY, torch.ones(()))
    ex = torch.where(opaque, torch.zeros(()), torch.ones(()))            # exp(-sigma): exactly 0 on an opaque sample, 1 elsewhere
    dens = (gw * T - suffix / f) * ex
    g = torch.cat([w[..., None] * g_rgb[:, None, :], dens[..., None]], -1)
    mask = torch.ones(n, S, 4, dtype=torch.bool)
    return g, mask, float(gw.abs().max())


def check_exact_backward(case, whites=(False, True), combos=COMBOS):
    """The closed-form gradients against the float64 autograd (within 4e-7 * max|gw|: the float64 oracle's 1 + 1e-10 factors, not a tolerance the
    device gets)."""
    for white in whites:
        for combo in combos:
            g, mask, scale = expected_g_raw(case, white, combo)
            ref = backward(case, F64, white, combo)
            d = ((g.double() - ref).abs() * mask).max().item()
            assert d <= 4e-7 * max(1.0, scale), "%s white=%s %s: closed form is %.3e from the float64 autograd" % (case["name"], white, combo, d)


def _exact_common(name, n, S, seed, variant=0):
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()      # noqa: E731
    case = dict(name=name, kind="exact", variant=variant, n=n, S=S)
    case["raw"] = torch.cat([ri(1, 3, n, S, 3) * (2 * ri(0, 1, n, S, 3) - 1), torch.zeros(n, S, 1)], -1)
    case["z"] = torch.arange(1, S + 1).float().expand(n, S).contiguous()
    case["u"] = ri(1, 4, n, S)
    case.update(g_rgb=ri(-2, 2, n, 3), g_depth=ri(-2, 2, n), g_acc=ri(-2, 2, n), g_weights=ri(-2, 2, n, S))
    return case, gen


def hit_case(S, kind):
    """n = S rays, ray r opaque at position r (+ a second opaque sample: `kind`); every fourth transparent density is -0.0."""
    case, _ = _exact_common("hit_S%d_%s" % (S, kind), S, S, 7 * S + HIT_KINDS.index(kind))
    sig = torch.zeros(S, S)
    sig[:, 3::4] = -0.0
    r = torch.arange(S)
    sig[r, r] = 200.0
    if kind == "last":
        sig[:, S - 1] = 200.0
    elif kind == "adjacent":
        sig[r[:-1], r[:-1] + 1] = 200.0
    case["raw"][..., 3] = sig
    return case


def empty_case():
    """Empty rays (density 0.0 and -0.0) between opaque ones in the same 4-ray block, and in the ragged last block."""
    case, _ = _exact_common("empty_S65", 6, 65, 11)
    sig = torch.zeros(6, 65)
    sig[3] = -0.0
    sig[0, 3] = sig[2, 64] = sig[4, 0] = 200.0
    case["raw"][..., 3] = sig
    return case


def small_n_case(n):
    case, _ = _exact_common("n%d_S65" % n, n, 65, 20 + n)
    r = torch.arange(n)
    case["raw"][r, (7 * r + 5) % 65, 3] = 200.0
    case["raw"][r[1::2], 64, 3] = 200.0
    return case


def helpers_case(S):
    """Variant 1 (utils/run_nerf_helpers.py): raw colours 0, unit-spaced integer depths, rays_d of norm 1 and 5, densities in {-5, 0, 1, 200} with
    integer noise.  Ray r runs scenario r % 8, positions shifted with r // 8."""
    n = 24 if S > 1 else 8
    case, _ = _exact_common("helpers_S%d" % S, n, S, 300 + S, variant=1)
    case["raw"][..., :3] = 0.0
    sig, noise, z = torch.zeros(n, S), torch.zeros(n, S), case["z"]
    rays_d = torch.tensor([[0.0, 0.0, 1.0], [3.0, 4.0, 0.0]])[torch.arange(n) % 2].clone()
    for r in range(n):
        sc, p = r % 8, (5 * (r // 8) + r) % max(S - 2, 1)
        q = min(p + 1 + (r // 8) * 31, S - 2) if S > 2 else 0
        if sc == 0:                                  # one opaque sample
            sig[r, p] = 200.0
        elif sc == 1 and S > 2:                      # noise turns the opaque sample off (200 - 200 = 0) and a transparent one on (0 + 200)
            sig[r, p], noise[r, p], noise[r, q] = 200.0, -200.0, 200.0
        elif sc == 1:
            sig[r, 0], noise[r, 0] = 200.0, -200.0
        elif sc == 2:                                # -5 everywhere, noise lifts some to exactly 0 and some to -2; last sample 0 * 1e10: an empty ray
            sig[r], noise[r, ::2], noise[r, 1::3] = -5.0, 5.0, 3.0
            sig[r, S - 1], noise[r, S - 1] = 0.0, 0.0
        elif sc == 3:                                # last sample of density 1: opaque through the 1e10 distance
            sig[r, S - 1] = 1.0
        elif sc == 4 and S > 2:                      # equal neighbouring depths under an opaque density (dist 0: alpha 0), a real hit behind
            z[r, p + 1:] = z[r, p + 1:] - 1.0
            sig[r, p] = 200.0
            if p + 1 < S - 1:
                sig[r, S - 2] = 200.0
        elif sc == 4:
            sig[r, S - 1] = 200.0
        elif sc == 5:                                # a hit, and the last sample opaque through 1e10 as the second
            sig[r, p], sig[r, S - 1] = 200.0, 1.0
        elif sc == 6:                                # noise drives the opaque density negative (200 - 205); the ray is empty up to its last sample
            sig[r, p], noise[r, p] = 200.0, -205.0
            sig[r, S - 1], noise[r, S - 1] = 0.0, 200.0
        else:                                        # -0.0 densities and negative noise: an empty ray
            sig[r], noise[r] = -0.0, -1.0
    case["raw"][..., 3] = sig
    case.update(noise=noise, rays_d=rays_d)
    return case


EXACT_BUILDERS = {}
for _S in HIT_S:
    for _k in HIT_KINDS:
        if not (_S == 1 and _k != "one"):
            EXACT_BUILDERS["hit_S%d_%s" % (_S, _k)] = functools.partial(hit_case, _S, _k)
EXACT_BUILDERS["empty_S65"] = empty_case
for _n in (1, 3, 4, 5):
    EXACT_BUILDERS["n%d_S65" % _n] = functools.partial(small_n_case, _n)
LIVE_EXACT_NAMES = tuple(EXACT_BUILDERS)
HELPERS_S = (1, 3, 65, 257, 1024)
for _S in HELPERS_S:
    EXACT_BUILDERS["helpers_S%d" % _S] = functools.partial(helpers_case, _S)
HELPERS_EXACT_NAMES = tuple("helpers_S%d" % s for s in HELPERS_S)
EXACT_NAMES = tuple(EXACT_BUILDERS)


@functools.lru_cache(maxsize=None)
def exact(name):
    """(case, {white: float32 expected outputs}) of an exact case, built and checked once per process."""
    case = EXACT_BUILDERS[name]()
    return case, check_exact(case)


# ------------------------------------------------------------------------------------------------ merged rows
MERGED_S = (2, 64, 65, 257, 1024)
RANK_KINDS = ("identity", "reversed", "interleaved", "random")


def merged_specs():
    out = []
    for S in MERGED_S:
        for na in sorted({0, 1, S // 2 + S % 2, S - 1, S}):
            for kind in RANK_KINDS:
                if kind != "interleaved" or na == S // 2 + S % 2:
                    out.append((S, na, kind))
    return out


def merged_case(S, na, kind):
    """The "last" hit sweep at S, its rows split into raw_a [n,na,4] and raw_b [n,S-na,4] with rank[r, j] = merged position of row j of
    cat(raw_a[r], raw_b[r]).  The expected outputs are the hit sweep's."""
    case, want = exact("hit_S%d_last" % S)
    n = case["n"]
    if kind == "identity":
        rank = torch.arange(S).expand(n, S)
    elif kind == "reversed":
        rank = torch.arange(S - 1, -1, -1).expand(n, S)
    elif kind == "interleaved":                      # a holds the even merged positions, b the odd ones
        assert na == S // 2 + S % 2
        rank = torch.cat([2 * torch.arange(na), 2 * torch.arange(S - na) + 1]).expand(n, S)
    else:
        gen = torch.Generator().manual_seed(1000 * S + na)
        rank = torch.stack([torch.randperm(S, generator=gen) for _ in range(n)])
    rank = rank.contiguous()
    assert bool((rank.sort(-1)[0] == torch.arange(S)).all())
    cat = torch.gather(case["raw"], 1, rank[..., None].expand(n, S, 4))          # cat[j] = merged[rank[j]]
    m = dict(name="merged_S%d_na%d_%s" % (S, na, kind), S=S, n=n, na=na, nb=S - na, rank=rank.int(), raw_a=cat[:, :na].contiguous(),
             raw_b=cat[:, na:].contiguous(), z=case["z"], u=case["u"])
    inv = rank.argsort(-1)                                                       # row of cat that lands on merged position i
    first = inv[torch.arange(n), torch.arange(n)]                                # ray r's own hit sits on merged position r
    m["hit_in_a"], m["hit_in_b"] = int((first < na).sum()), int((first >= na).sum())
    back = torch.empty_like(case["raw"])
    back.scatter_(1, rank[..., None].expand(n, S, 4), cat)
    assert torch.equal(back, case["raw"])
    return m, want


# ------------------------------------------------------------------------------------------------ continuous cases
CONT_S = (1, 2, 65, 193, 257, 513, 1024)
CONT_NAMES = tuple("cont_S%d" % s for s in CONT_S) + tuple("cont_helpers_S%d" % s for s in CONT_S)
DISP_ACC_MIN = 1e-3
BAR_NAMES = ("rgb", "depth", "acc", "weights", "disp", "var", "wu", "g_colour", "g_density")


def continuous_case(name):
    helpers = "helpers" in name
    S = int(name.rsplit("S", 1)[1])
    n = 7
    gen = torch.Generator().manual_seed((5000 if helpers else 4000) + S)
    rnd = lambda *s: torch.rand(*s, generator=gen)      # noqa: E731
    case = dict(name=name, kind="continuous", variant=int(helpers), n=n, S=S)
    sig = torch.zeros(n, S)
    for r, scale in enumerate((0.01, 1.0, 10.0, 50.0)):
        sig[r] = scale * (0.25 + 1.5 * rnd(S))
    sig[5] = 0.25 + 1.5 * rnd(S)
    sig[5][rnd(S) < 0.3] = 200.0                    # transmittance 1e-10, 1e-20, ... through the denormals to 0 mid-ray
    third = (sig[5] == 200.0).long().cumsum(0).eq(3).nonzero()
    if len(third):                                  # behind the third opaque sample (T ~ 1e-30) a dozen samples of factor 0.1: every decade down to 1e-42
        sig[5, int(third[0]) + 1:int(third[0]) + 13] = 2.3
    sig[6] = 0.25 + 1.5 * rnd(S)
    sig[6, 0] = 200.0                               # (ray 4 stays all zero: the empty ray)
    case["z"] = torch.sort(1.0 + 3.0 * rnd(n, S), -1)[0]
    case["u"] = rnd(n, S)
    if helpers:                                     # raw in +-4 (activations inside the kernel), N(0, 1) noise, rays_d of no particular length
        case["raw"] = 8.0 * rnd(n, S, 4) - 4.0
        case["noise"] = torch.randn(n, S, generator=gen)
        case["rays_d"] = torch.randn(n, 3, generator=gen) * 1.7
        case["raw"][:, -1, 3] = case["raw"][:, -1, 3].abs() + 0.5      # the 1e10 last distance closes every ray ...
        case["noise"][:, -1] = case["noise"][:, -1].abs()
        case["raw"][4, :, 3] = -4.0                                    # ... but the empty one: sigma + noise < 0 on all of it
        case["noise"][4] = case["noise"][4].clamp(max=3.0)
    else:
        case["raw"] = torch.cat([3.0 * rnd(n, S, 3) - 1.0, sig[..., None]], -1)      # rgb in [-1, 2]: the live variant takes it as given
        case.update(g_rgb=torch.randn(n, 3, generator=gen), g_depth=torch.randn(n, generator=gen), g_acc=torch.randn(n, generator=gen),
                    g_weights=torch.randn(n, S, generator=gen))
    return case


def disp_keep(ref64):
    """Rays whose disp is compared: float64 acc > 1e-3 (1 / (depth / acc) of an all but empty ray is 0 / 0 in the making)."""
    return ref64["acc"] > DISP_ACC_MIN


def fwd_distances(got, ref64):
    """Max |got - float64 reference| per output present in both; disp on the kept rays only, NaN positions required to agree (-> inf)."""
    d = {}
    for k, r in ref64.items():
        if k not in got:
            continue
        g = got[k].double().reshape(r.shape)
        if k == "disp":
            keep = disp_keep(ref64)
            if not bool(((g != g) == (r != r)).all()):
                d[k] = float("inf")
                continue
            g, r = g[keep], r[keep]
        d[k] = (g - r).abs().max().item() if r.numel() else 0.0
    return d


def bwd_distances(g_raw, ref64):
    e = (g_raw.double().reshape(ref64.shape) - ref64).abs()
    return dict(g_colour=e[..., :3].max().item(), g_density=e[..., 3].max().item())


@functools.lru_cache(maxsize=None)
def continuous(name):
    """(case, {white: float64 outputs}, {white: float32 oracle's distances}, {(white, combo): float64 g_raw},
    {(white, combo): float32 oracle's distances}), built once per process."""
    case = continuous_case(name)
    ref, dist, gref, gdist = {}, {}, {}, {}
    for white in (False, True):
        ref[white] = forward(case, F64, white)
        keep = disp_keep(ref[white])
        assert int((~keep).sum()) <= 1, "%s: %d of 7 rays outside the disp comparison" % (name, int((~keep).sum()))
        dist[white] = fwd_distances(forward(case, F32, white), ref[white])
        if case["variant"] == 0:
            for combo in COMBOS:
                gref[white, combo] = backward(case, F64, white, combo)
                assert bool(torch.isfinite(gref[white, combo]).all()), name
                g32 = backward(case, F32, white, combo)
                assert bool(torch.isfinite(g32).all()), name
                gdist[white, combo] = bwd_distances(g32, gref[white, combo])
    return case, ref, dist, gref, gdist


@functools.lru_cache(maxsize=None)
def bars():
    """{output name: 4 x the float32 oracle's largest distance from the float64 oracle over the continuous cases}."""
    worst = dict.fromkeys(BAR_NAMES, 0.0)
    for name in CONT_NAMES:
        _, _, dist, _, gdist = continuous(name)
        for d in list(dist.values()) + list(gdist.values()):
            for k, v in d.items():
                worst[k] = max(worst[k], v)
    assert all(0 < v < float("inf") for v in worst.values()), worst
    return {k: 4.0 * v for k, v in worst.items()}


def over_the_bar(dist, what):
    """Failure lines for the distances above their bars."""
    b = bars()
    return ["%s %s: %.3e > bar %.3e" % (what, k, v, b[k]) for k, v in dist.items() if not v <= b[k]]
