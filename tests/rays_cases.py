"""Cases, a float32 numpy restatement and the float64 reference for the eight stand-alone ray front-end entry points of csrc/rays.hip
(ucnerf_ray_gen, ucnerf_ray_gen_sample, ucnerf_ndc_rays, ucnerf_dir_feature, ucnerf_sample_stratified, ucnerf_sample_cascade,
ucnerf_ndc_project, ucnerf_embed).  Shared by tests/test_rays_cases_host.py (CPU) and tests/test_hip_ray_edges.py (GPU); everything here is
deterministic and cached, nothing touches a device.

The restatement says in elementary numpy float32 steps, in the kernel's operation order, what each kernel computes.  All kernel arithmetic is
+ - * /, sqrtf, fmaf, rintf and int/float conversions, the library is built with -ffp-contract=off and correctly rounded division and square
root, and numpy's float32 ufuncs round every single operation to nearest-even: the two agree bit for bit on ANY input.  The one operation numpy
lacks is a fused multiply-add; fma32() below is an exactly rounded one (proved against std::fmaf in the host test).  The one path that cannot be
restated is OCML's sincosf above |r| = 65536; those outputs are flagged (`slow`) and compared with float64 under an absolute bar.

The float64 reference is oracle/ucnerf_oracle.py fed float64 tensors: the independent witness for a formula error the restatement would copy.
Every case holds: kind, name, lattice (bool), the inputs, `want` {output: float32 restatement}, `ref` {output: float64 reference},
`dist` / `scale` {output: the restatement's largest distance from the reference / the reference's largest magnitude}."""
import functools
import itertools
import math

import numpy as np
import torch

from oracle import ucnerf_oracle as O

F32 = np.float32
F64 = np.float64
ONE, HALF = F32(1.0), F32(0.5)
GUARD = 64                     # floats of -7.0 the device test keeps behind every output
SINCOS_FAST_MAX = F32(65536.0)
CLAMP = F32(1e-4)              # 1e-4f of geometry_device.h: below the double 1e-4


def f32(a):
    return np.asarray(a, dtype=F32)


def bits(a):
    return np.ascontiguousarray(f32(a)).view(np.uint32)


def same_bits(a, b):
    """Bit for bit, -0.0 apart from +0.0; any NaN matches any NaN (image_cases.same_bits)."""
    a, b = f32(a), f32(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | ((a != a) & (b != b))).all())


def bar(oracle_distance, scale):
    """What the device may differ from the float64 reference by where a bit comparison has to fall back: 4 x the float32 restatement's own
    distance + 1e-6 of the output's largest reference value (the rule of gather_cases.bar and mvs_cases.bar)."""
    return 4.0 * oracle_distance + 1e-6 * scale


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=F64))


# ------------------------------------------------------------------------------------------------ exact fmaf
def fma32(a, b, c):
    """fmaf(a, b, c) exactly rounded.  The product of two float32 is exact in float64 (48 bits); the float64 sum p + c is rounded once, its
    residual e is recovered exactly (two-sum) and folded back as a sticky bit: when e != 0 the sum is moved to that neighbour of the exact value
    whose last mantissa bit is odd (rounding to odd), and a value rounded to odd at 53 bits rounds to 24 bits as the exact value does."""
    a, b, c = np.broadcast_arrays(f32(a), f32(b), f32(c))
    shape = a.shape
    with np.errstate(all="ignore"):
        p = a.astype(F64).reshape(-1) * b.astype(F64).reshape(-1)
        c64 = c.astype(F64).reshape(-1)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32).reshape(shape)


def fma32_double_rounded(a, b, c):
    """The WRONG emulation (float64(a*b + c) -> float32): kept for the host test, which shows that the std::fmaf sweep tells it from fma32."""
    with np.errstate(all="ignore"):
        return (f32(a).astype(F64) * f32(b).astype(F64) + f32(c).astype(F64)).astype(F32)


# ------------------------------------------------------------------------------------------------ sincos (sincos_cw.h)
def sincos_fast32(r, fma=fma32):
    """sincos_pe_fast: valid for |r| <= 65536."""
    r = f32(r)
    with np.errstate(all="ignore"):
        qf = np.rint(r * F32(0.63661977236758134))
        y = fma(qf, F32(-1.57079637050628662109375), r)
        y = fma(qf, F32(4.37113900018624283e-8), y)
        y = fma(qf, F32(1.71512451e-15), y)
        q = np.where(qf == qf, qf, F32(0)).astype(np.int32)
        z = y * y
        sp = fma(z, F32(-1.9515295891e-4), F32(8.3321608736e-3))
        sp = fma(sp, z, F32(-1.6666654611e-1))
        sn = fma(sp * z, y, y)
        cp = fma(z, F32(2.443315711809948e-5), F32(-1.388731625493765e-3))
        cp = fma(cp, z, F32(4.166664568298827e-2))
        cs = fma(cp * z, z, fma(z, F32(-0.5), ONE))
    swap = (q & 1) != 0
    s, c = np.where(swap, cs, sn), np.where(swap, sn, cs)
    s = np.where((q & 2) != 0, -s, s)
    c = np.where(((q + 1) & 2) != 0, -c, c)
    return f32(s), f32(c)


def is_slow(r):
    """sincos_pe's switch: fabsf(r) > 65536 (false for NaN, true for +-inf)."""
    with np.errstate(invalid="ignore"):
        return np.abs(f32(r)) > SINCOS_FAST_MAX


# ------------------------------------------------------------------------------------------------ raygen_device.h
def linspace01(i, S):
    """linspace01(i, S) of raygen_device.h for an integer array i."""
    i = np.asarray(i, dtype=np.int64)
    if S == 1:
        return np.zeros(i.shape, F32)
    step = ONE / F32(S - 1)
    return f32(np.where(i < S // 2, step * i.astype(F32), ONE - step * (S - 1 - i).astype(F32)))


def z_at(near, far, i, S, lindisp, linspace=linspace01):
    t = linspace(i, S)
    with np.errstate(all="ignore"):
        if lindisp:
            return f32(ONE / (ONE / near * (ONE - t) + ONE / far * t))
        return f32(near * (ONE - t) + far * t)


def stratified32(near, far, S, lindisp, perturb, noise, linspace=linspace01):
    """near, far [n,1] float32 -> z [n,S]: stratified_depth for every (ray, sample).  `linspace`: the host test hands in a deliberately wrong one."""
    near, far = f32(near).reshape(-1, 1), f32(far).reshape(-1, 1)
    s = np.arange(S)[None, :]
    z = z_at(near, far, s, S, lindisp, linspace) + np.zeros((near.shape[0], 1), F32)
    if perturb > 0:
        zl = z_at(near, far, np.maximum(s - 1, 0), S, lindisp, linspace)
        zu = z_at(near, far, np.minimum(s + 1, S - 1), S, lindisp, linspace)
        lower = np.where(s > 0, HALF * (zl + z), z)
        upper = np.where(s + 1 < S, HALF * (z + zu), z)
        z = lower + (upper - lower) * (F32(perturb) * f32(noise).reshape(-1, S))
    return f32(z)


def pinhole32(x, y, K, R):
    dx, dy = (x - K[2]) / K[0], (y - K[5]) / K[4]
    return [f32(dx * R[4 * r] + dy * R[4 * r + 1] + ONE * R[4 * r + 2]) for r in range(3)]


def view_dir32(wx, wy, wz, Q):
    with np.errstate(all="ignore"):
        c = np.sqrt(wx * wx + wy * wy + wz * wz)
        ux, uy, uz = wx / c, wy / c, wz / c
        return np.stack([ux * Q[4 * r] + uy * Q[4 * r + 1] + uz * Q[4 * r + 2] for r in range(3)], -1).astype(F32), f32(c)


# ------------------------------------------------------------------------------------------------ helpers for the inputs
def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def _pose(rng, scale=1.0):
    m = np.zeros((3, 4))
    m[:, :3] = _rotation(rng)
    m[:, 3] = rng.standard_normal(3) * scale
    return f32(m)


def _finish(case, want, ref):
    """Distances and scales per output; on a lattice case the restatement must EQUAL the float64 reference element for element."""
    case["want"] = {k: f32(v) for k, v in want.items()}
    case["ref"] = {k: np.asarray(v, F64) for k, v in ref.items()}
    assert set(case["want"]) == set(case["ref"]), (case["name"], set(want) ^ set(ref))
    case["dist"], case["scale"] = {}, {}
    for k, w in case["want"].items():
        r = case["ref"][k]
        assert w.shape == r.shape, (case["name"], k, w.shape, r.shape)
        skip = case.get("slow", {}).get(k)
        w64 = w.astype(F64)
        fin = np.isfinite(r) & np.isfinite(w64)
        if skip is not None:
            fin &= ~skip
        same_kind = (np.isnan(r) & np.isnan(w64)) | (np.isinf(r) & (r == w64))
        if skip is not None:
            same_kind |= skip
        assert bool((fin | same_kind).all()), (case["name"], k, "inf / NaN in different places")
        with np.errstate(invalid="ignore"):
            case["dist"][k] = float(np.abs(w64 - r)[fin].max()) if fin.any() else 0.0
        case["scale"][k] = float(np.abs(r)[fin].max()) if fin.any() else 0.0
        if case["lattice"]:
            assert case["dist"][k] == 0.0, (case["name"], k, case["dist"][k])
        _ro(w, r)
    for v in case.values():
        _ro(v)
    return case


# ================================================================================================ ray_gen
RAY_GEN_NAMES = tuple(["grid5x7_n%d%s" % (n, g) for n in (1, 2, 25) for g in ("", "_gl")] +
                      ["grid20x16_n%d" % n for n in (255, 256, 257)] + ["grid20x16_n257_gl", "pixels", "lattice", "lattice_gl"])
OUTPUT_SUBSETS = tuple(itertools.chain.from_iterable(itertools.combinations(("rays_o", "pix", "angle"), k) for k in range(4)))


def ray_gen32(c):
    n = c["n"]
    if c["xs"] is not None:
        x, y = c["xs"], c["ys"]
    else:
        idx = c["grid_start"] + np.arange(n)
        y, x = (idx // c["W"]).astype(F32), (idx % c["W"]).astype(F32)
    R = c["c2w"].reshape(-1)
    if c["opengl"]:
        f = c["K"].reshape(-1)[0]
        dx, dy, dz = (x - F32(c["W"]) * HALF) / f, -(y - F32(c["H"]) * HALF) / f, F32(-1.0)
        w = [f32(dx * R[4 * r] + dy * R[4 * r + 1] + dz * R[4 * r + 2]) for r in range(3)]
    else:
        w = pinhole32(x, y, c["K"].reshape(-1), R)
    out = {"rays_d": np.stack(w, -1), "rays_o": np.tile(R[[3, 7, 11]], (n, 1)), "pix": np.stack([y, x])}
    if not c["lattice"]:
        out["angle"] = view_dir32(w[0], w[1], w[2], c["w2c_dir"].reshape(-1))[0]
    return out


def ray_gen64(c):
    n, K, c2w = c["n"], _t64(c["K"]), _t64(c["c2w"])
    if c["xs"] is not None:
        xs, ys = _t64(c["xs"]), _t64(c["ys"])
    else:
        ys, xs = O.pixel_grid(c["H"], c["W"], torch.float64)
        ys, xs = ys[c["grid_start"]:c["grid_start"] + n], xs[c["grid_start"]:c["grid_start"] + n]
    if c["opengl"]:
        o, d = O.get_rays_opengl(c["H"], c["W"], float(c["K"][0, 0]), c2w)
        d = d.reshape(-1, 3)[c["grid_start"]:c["grid_start"] + n]
        o, pix = c2w[:3, 3], torch.stack((ys, xs))
    else:
        o, d, pix = O.get_rays_mvs_pixels(xs, ys, K, c2w)
    out = {"rays_d": d.numpy(), "rays_o": o.expand(n, 3).numpy(), "pix": pix.numpy()}
    if not c["lattice"]:
        out["angle"] = O.gen_dir_feature(_t64(c["w2c_dir"]), d / d.norm(dim=-1, keepdim=True)).numpy()
    return out


@functools.lru_cache(maxsize=None)
def ray_gen_case(name):
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    c = dict(kind="ray_gen", name=name, lattice=name.startswith("lattice"), opengl=name.endswith("_gl"), xs=None, ys=None, grid_start=0)
    if c["lattice"]:
        c.update(H=5, W=9, grid_start=7, n=38)                                                  # ends exactly at H*W
        c["K"] = f32([[4, 0, 2], [0, 8, 1], [0, 0, 1]])
        c["c2w"] = f32([[0, -2, 0, 3], [1, 0, 0, -5], [0, 0, 4, 0.5]])
        c["w2c_dir"] = f32(np.eye(4)[:3])
    else:
        c["K"] = f32([[37.5, 0, 9.3], [0, 41.25, 7.1], [0, 0, 1]])                              # K[0] != K[4], principal point off centre
        c["c2w"], c["w2c_dir"] = _pose(rng), _pose(rng)
        if name.startswith("grid5x7"):
            n = int(name.split("_n")[1].split("_")[0])
            c.update(H=5, W=7, grid_start=10, n=n)                                              # 10 % 7 = 3: mid-row; 10 + 25 = H*W
        elif name.startswith("grid20x16"):
            c.update(H=20, W=16, grid_start=3, n=int(name.split("_n")[1].split("_")[0]))
        else:                                                                                   # pixel list: fractional and negative
            c.update(H=0, W=0, n=70)
            c["xs"], c["ys"] = f32(rng.uniform(-6, 25, 70)), f32(rng.uniform(-6, 25, 70))
            c["xs"][:3], c["ys"][:3] = [-0.5, 0.0, 3.25], [2.75, -1.0, 0.0]
    return _finish(c, ray_gen32(c), ray_gen64(c))


# ================================================================================================ ray_gen_sample
RAY_GEN_SAMPLE_NAMES = tuple("n%d_S%d_p%d" % (n, S, p) for (n, S) in ((300, 1), (85, 3), (5, 257), (37, 7)) for p in (0, 1))


@functools.lru_cache(maxsize=None)
def ray_gen_sample_case(name):
    """ray_gen (pixel list, angle) and sample_stratified (scalar near / far) from one launch."""
    n, S, p = (int(t[1:]) for t in name.split("_"))
    rng = np.random.default_rng(n * 1000 + S + p)
    assert S == 1 or (n * S) % 256 != 0
    c = dict(kind="ray_gen_sample", name=name, lattice=False, opengl=False, grid_start=0, H=0, W=0, n=n, S=S, perturb=float(p), lindisp=0,
             near=F32(0.75), far=F32(5.5))
    c["K"] = f32([[37.5, 0, 9.3], [0, 41.25, 7.1], [0, 0, 1]])
    c["c2w"], c["w2c_dir"] = _pose(rng), _pose(rng)
    c["xs"], c["ys"] = f32(rng.uniform(-2, 20, n)), f32(rng.uniform(-2, 16, n))
    c["noise"] = f32(rng.random((n, S)))
    want = {k: v for k, v in ray_gen32(c).items() if k in ("rays_d", "angle")}
    ref = {k: v for k, v in ray_gen64(c).items() if k in ("rays_d", "angle")}
    near, far = np.full((n, 1), c["near"]), np.full((n, 1), c["far"])
    want["z"] = stratified32(near, far, S, 0, c["perturb"], c["noise"])
    rays = torch.zeros(n, 8, dtype=torch.float64)
    rays[:, 6], rays[:, 7] = float(c["near"]), float(c["far"])
    ref["z"] = O.ray_marcher(rays, S, False, c["perturb"], _t64(c["noise"]))[3].numpy()
    return _finish(c, want, ref)


# ================================================================================================ ndc_rays
NDC_RAYS_NAMES = ("v0", "v1", "v1_one_focal", "lattice_v0", "lattice_v1")


def ndc_rays32(c):
    o, d = c["rays_o"], c["rays_d"]
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    near = c["near"]
    t = -(near + oz) / dz
    ox, oy, oz = ox + t * dx, oy + t * dy, oz + t * dz
    sx, sy = F32(-1.0) / (F32(c["W"]) / (F32(2.0) * c["fx"])), F32(-1.0) / (F32(c["H"]) / (F32(2.0) * c["fy"]))
    ox_oz, oy_oz = ox / oz, oy / oz
    o2 = ONE + F32(2.0) * near / oz
    d2 = ONE - o2 if c["variant"] == 0 else F32(-2.0) * near / oz
    return {"out_o": np.stack([sx * ox_oz, sy * oy_oz, o2], -1), "out_d": np.stack([sx * (dx / dz - ox_oz), sy * (dy / dz - oy_oz), d2], -1)}


@functools.lru_cache(maxsize=None)
def ndc_rays_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(kind="ndc_rays", name=name, lattice=name.startswith("lattice"), variant=int(name.split("v")[1][0]))
    if c["lattice"]:
        c.update(n=64, H=4, W=8, fx=F32(2.0), fy=F32(8.0), near=F32(1.0))
        c["rays_o"] = f32(rng.integers(-8, 9, (64, 3)) / 4.0)
        c["rays_d"] = f32(np.stack([rng.integers(-8, 9, 64) / 4.0, rng.integers(-8, 9, 64) / 8.0, rng.choice([-4, -2, -1, -0.5, 0.5, 1, 2, 4], 64)], -1))
        c["rays_o"][:, 2] = rng.choice([-3, -2, 0, 1, 3], 64)         # o_z + t d_z = -near exactly: every division is by a power of two
    else:
        fx = 30.5
        c.update(n=300, H=15, W=20, fx=F32(fx), fy=F32(fx if name == "v1_one_focal" else 27.25), near=F32(0.75))
        c["rays_o"] = f32(rng.standard_normal((300, 3)))
        d = rng.standard_normal((300, 3))
        d[:, 2] = rng.uniform(0.25, 2.0, 300) * np.where(np.arange(300) % 2 == 0, 1, -1)      # dz of both signs, away from zero
        c["rays_d"] = f32(d)
    o, d = _t64(c["rays_o"]), _t64(c["rays_d"])
    ro, rd = O.get_ndc_rays(c["H"], c["W"], [float(c["fx"]), float(c["fy"])], float(c["near"]), o, d)
    if c["variant"] == 1:
        ho, hd = O.ndc_rays(c["H"], c["W"], float(c["fx"]), float(c["near"]), o, d)             # (d_z = -2 near / o_z does not depend on the focal)
        rd = torch.cat([rd[:, :2], hd[:, 2:]], -1)
        if c["fx"] == c["fy"]:
            ro, rd = ho, hd
    return _finish(c, ndc_rays32(c), {"out_o": ro.numpy(), "out_d": rd.numpy()})


# ================================================================================================ dir_feature
DIR_FEATURE_NAMES = tuple("rep%d" % r for r in (0, 1, 2, 5)) + ("zero_direction",)
DIR_ROUTES = ("none", "host", "device")


def dir_feature32(c, route):
    d = c["rays_d"]
    Q = (c["w2c_ref"] if route != "none" else f32(np.eye(4)[:3])).reshape(-1)
    with np.errstate(all="ignore"):
        if route == "none":
            cn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            a = np.stack([d[:, 0] / cn, d[:, 1] / cn, d[:, 2] / cn], -1)
        else:
            a, cn = view_dir32(d[:, 0], d[:, 1], d[:, 2], Q)
    return {"angle": np.repeat(f32(a), max(c["repeat"], 1), axis=0), "cos_angle": f32(cn)}


@functools.lru_cache(maxsize=None)
def dir_feature_case(name, route="host"):
    """n * repeat crosses a block edge (256) for every repeat; directions of length >= 0.1."""
    rng = np.random.default_rng(sum(map(ord, name)))
    rep = 2 if name == "zero_direction" else int(name[3:])
    n = {0: 257, 1: 257, 2: 129, 5: 52}[rep]
    assert (n * max(rep, 1)) > 256 and (n * max(rep, 1)) % 256 != 0
    d = rng.standard_normal((n, 3))
    d *= np.maximum(0.1 / np.linalg.norm(d, axis=1, keepdims=True), 1.0) * rng.uniform(1.0, 3, (n, 1))
    d = f32(d)
    if name == "zero_direction":
        d[40] = 0.0
    c = dict(kind="dir_feature", name=name, lattice=False, n=n, repeat=rep, rays_d=d, w2c_ref=_pose(rng), route=route)
    want = dir_feature32(c, route)
    d64 = _t64(d)
    with np.errstate(all="ignore"):
        norm = d64.norm(dim=-1, keepdim=True)
        unit = d64 / norm
        ang = O.gen_dir_feature(_t64(c["w2c_ref"]), unit) if route != "none" else unit
    ref = {"angle": np.repeat(ang.numpy(), max(rep, 1), axis=0), "cos_angle": norm[:, 0].numpy()}
    return _finish(c, want, ref)


# ================================================================================================ sample_stratified
STRAT_S = (1, 2, 3, 4, 5, 64, 65)
STRAT_NAMES = tuple("S%d_%s_%s_p%s_%s" % (S, form, "disp" if ld else "lin", p, nz)
                    for S in STRAT_S for (form, ld, p, nz) in (("rays", 0, "0", "rand"), ("rays", 1, "1", "rand"), ("scalar", 0, "0.5", "rand"),
                                                               ("rays", 0, "1", "zero"), ("rays", 1, "0.5", "top"), ("scalar", 1, "1", "rand"))) + \
    tuple("lattice_S%d_p%s" % (S, p) for S in (1, 2, 3, 5, 65) for p in ("0", "1"))


@functools.lru_cache(maxsize=None)
def stratified_case(name):
    """form rays: per-ray near / far from the [n,8] array (and points); scalar: one near / far.  noise: rand, zero (exactly 0) or top (1 - 2^-24).
    Lattice: S - 1 a power of two (t is dyadic), dyadic near / far / noise, integer rays: float32 is exact."""
    rng = np.random.default_rng(sum(map(ord, name)))
    lattice = name.startswith("lattice")
    if lattice:
        S, form, ld, p, nz = int(name.split("_")[1][1:]), "rays", 0, name.split("_p")[1], "dyadic"
    else:
        t = name.split("_")
        S, form, ld, p, nz = int(t[0][1:]), t[1], int(t[2] == "disp"), t[3][1:], t[4]
    n = 5 if S >= 64 else 37                                     # 5 * 64 = 320, 5 * 65 = 325: a ray's samples span the block edge at 256
    c = dict(kind="sample_stratified", name=name, lattice=lattice, n=n, S=S, lindisp=ld, perturb=float(p), form=form)
    rays = np.zeros((n, 8))
    if lattice:
        rays[:, :6] = rng.integers(-4, 5, (n, 6))
        rays[:, 6] = rng.integers(1, 5, n) / 2.0
        rays[:, 7] = rays[:, 6] + rng.choice([1, 2, 4], n)
        noise = rng.integers(0, 16, (n, S)) / 16.0
    else:
        rays[:, :6] = rng.standard_normal((n, 6))
        rays[:, 6] = rng.uniform(0.25, 1.5, n)                  # near >= 0.25
        rays[:, 7] = rays[:, 6] + rng.uniform(0.5, 6, n)
        noise = {"rand": rng.random((n, S)), "zero": np.zeros((n, S)), "top": np.full((n, S), 1 - 2.0 ** -24)}[nz]
    if form == "scalar":
        rays[:, 6], rays[:, 7] = rays[0, 6], rays[0, 7]
    c["rays"], c["noise"] = f32(rays), f32(noise)
    r = c["rays"]
    z = stratified32(r[:, 6:7], r[:, 7:8], S, ld, c["perturb"], c["noise"])
    want = {"z": z}
    pts, _, _, z64 = O.ray_marcher(_t64(r), S, bool(ld), c["perturb"], _t64(c["noise"]))
    ref = {"z": z64.numpy()}
    if form == "rays":
        want["pts"] = np.stack([r[:, None, k] + r[:, None, 3 + k] * z for k in range(3)], -1)
        ref["pts"] = pts.numpy()
    return _finish(c, want, ref)


# ================================================================================================ sample_cascade
CASCADE_S = (3, 6, 9, 63, 192, 384, 387, 765, 768)
CASCADE_LAYOUTS = ("disjoint", "nested", "overlapping", "identical", "descending", "reversed_stage")
CASCADE_T = ("null", "zero", "top", "rand")
CASCADE_NAMES = tuple("S%d_%s" % (S, t) for S in CASCADE_S for t in CASCADE_T) + ("lattice_S6", "lattice_S15")


def cascade32(c):
    S, n3, nf = c["S"], c["S"] // 3, c["near_far"]
    i = np.arange(S)
    k, j = i // n3, i % n3
    t = linspace01(j, n3)[None, :]
    v = f32(nf[:, 2 * k] * (ONE - t) + nf[:, 2 * k + 1] * t)
    z = np.sort(v, axis=1)
    if c["t_rand"] is not None:
        lower, upper = z.copy(), z.copy()
        lower[:, 1:] = HALF * (z[:, 1:] + z[:, :-1])
        upper[:, :-1] = HALF * (z[:, 1:] + z[:, :-1])
        z = f32(lower + (upper - lower) * c["t_rand"])
    out = {"z": z}
    out["pts"] = np.stack([c["rays_o"][kk] + z * c["rays_d"][:, None, kk] for kk in range(3)], -1)
    return out, v


@functools.lru_cache(maxsize=None)
def cascade_case(name):
    """One ray per range layout (six rays): the three stages' [near, far] disjoint and ascending, nested, overlapping, all identical (every value
    three times: ties), in descending order, and one stage with near > far.  P, the padded sort length (no multiple of 3 is a power of two, so P > S
    always): 3 -> 4, 6 -> 8, 9 -> 16, 63 -> 64 (one padding slot), 192 -> 256, 384 and 387 -> 512, 765 -> 1024 (259 padding slots), 768 -> 1024 (256)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    lattice = name.startswith("lattice")
    S = int(name.split("_")[1][1:]) if lattice else int(name.split("_")[0][1:])
    tk = "rand" if lattice else name.split("_")[1]
    nf = f32([[1.0, 2.0, 2.5, 3.5, 4.0, 5.0], [1.0, 5.0, 2.0, 4.0, 2.5, 3.5], [1.0, 3.0, 2.0, 4.0, 3.5, 5.0], [1.5, 3.5, 1.5, 3.5, 1.5, 3.5],
              [4.0, 5.0, 2.5, 3.5, 1.0, 2.0], [1.0, 3.0, 4.5, 2.5, 3.0, 5.0]])
    if not lattice:
        nf = f32(nf + np.array([[0], [0.013], [0.021], [0], [0.037], [0.041]]) * np.array([1, 1.1, 1.2, 1.3, 1.4, 1.5]))
        nf[3] = [1.5125, 3.4875, 1.5125, 3.4875, 1.5125, 3.4875]                         # identical stays identical
    n = nf.shape[0]
    c = dict(kind="sample_cascade", name=name, lattice=lattice, n=n, S=S, near_far=nf, layouts=CASCADE_LAYOUTS)
    if lattice:                                                                             # n3 - 1 a power of two: S = 6 (n3 = 2), 15 (n3 = 5)
        c["t_rand"] = f32(rng.integers(0, 8, (n, S)) / 8.0)
        c["rays_o"], c["rays_d"] = f32([1, -2, 3]), f32(rng.integers(-4, 5, (n, 3)))
    else:
        c["t_rand"] = {"null": None, "zero": np.zeros((n, S), F32), "top": np.full((n, S), F32(1 - 2.0 ** -24)), "rand": f32(rng.random((n, S)))}[tk]
        c["rays_o"], c["rays_d"] = f32(rng.standard_normal(3)), f32(rng.standard_normal((n, 3)))
    want, v = cascade32(c)
    c["unsorted"] = v
    cols = [_t64(nf[:, k:k + 1]) for k in range(6)]
    if c["t_rand"] is None:
        z64 = torch.sort(torch.cat([O.sample_points_uniform(cols[2 * k], cols[2 * k + 1], S // 3) for k in range(3)], -1), dim=-1)[0]
    else:
        z64 = O.cascade_depth_candidates(*cols, S, _t64(c["t_rand"]))
    ref = {"z": z64.numpy(), "pts": (_t64(c["rays_o"]).view(1, 1, 3) + z64.unsqueeze(-1) * _t64(c["rays_d"]).unsqueeze(1)).numpy()}
    return _finish(c, want, ref)


# ================================================================================================ ndc_project
NDC_PROJECT_NAMES = ("m1_w2c", "m255_w2c", "m257_w2c", "m255_cam", "m257_stride0", "m255_2d", "m64_equal_range", "lattice", "lattice_cam", "clamp")
STAGE_SUBSETS = tuple(s for k in range(1, 5) for s in itertools.combinations(("stage1", "stage2", "stage3", "ndc"), k))


def ndc_project32(c):
    p = c["pts"]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        if c["has_w2c"]:
            M = c["w2c"].reshape(-1)
            cx = x * M[0] + y * M[1] + z * M[2] + M[3]
            cy = x * M[4] + y * M[5] + z * M[6] + M[7]
            cz = x * M[8] + y * M[9] + z * M[10] + M[11]
            cz = f32(np.where(np.abs(cz) < CLAMP, CLAMP, cz))
            x, y, z = cx, cy, cz
        K = c["K"].reshape(-1)
        qx, qy, qz = x * K[0] + y * K[1] + z * K[2], x * K[3] + y * K[4] + z * K[5], x * K[6] + y * K[7] + z * K[8]
        u, v = (qx / qz + F32(0.0)) / c["inv_scale"][0], (qy / qz + F32(0.0)) / c["inv_scale"][1]
        if c["sample_2d"]:
            return {"ndc": np.stack([u, v, qz], -1)}, f32(z)
        out = {}
        for s in (1, 2, 3):
            nr, fr = c["near_%d" % s], c["far_%d" % s]
            out["stage%d" % s] = np.stack([u, v, (qz - nr) / (fr - nr)], -1)
        out["ndc"] = np.stack([u, v, (qz - c["near"]) / (c["far"] - c["near"])], -1)
    return out, f32(z)


def ndc_project_ref(c, dtype=torch.float64):
    cast = (lambda a: torch.from_numpy(np.array(a, dtype=F64 if dtype == torch.float64 else F32)))
    nf = None
    if not c["sample_2d"]:
        nf = {k: cast(c[k]).reshape(-1, 1) for k in ("near_1", "far_1", "near_2", "far_2", "near_3", "far_3")}
        nf["near"], nf["far"] = float(c["near"]), float(c["far"])
    with np.errstate(all="ignore"):
        out = O.get_ndc_coordinate(cast(c["w2c"]) if c["has_w2c"] else None, cast(c["K"]), cast(c["pts"]), cast(c["inv_scale"]), nf, bool(c["sample_2d"]))
    return {"ndc": out.numpy()} if c["sample_2d"] else {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def ndc_project_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    lattice = name.startswith("lattice")
    c = dict(kind="ndc_project", name=name, lattice=lattice, has_w2c=int("cam" not in name), sample_2d=int(name.endswith("2d")),
             nf_stride=int("stride0" not in name), near=F32(0.5), far=F32(4.5))
    if name == "clamp":
        return _clamp_case(c)
    if lattice:
        m = 96
        c["w2c"] = f32([[0, -1, 0, 2], [2, 0, 0, -1], [0, 0, 1, 0]])
        c["K"] = f32([[4, 0, 2], [0, 8, 1], [0, 0, 1]])
        c["inv_scale"] = f32([8, 4])                                                    # W - 1, H - 1 powers of two
        pts = np.stack([rng.integers(-8, 9, m) / 4.0, rng.integers(-8, 9, m) / 4.0, rng.choice([0.5, 1, 2, 4], m)], -1)     # q_z a power of two
        near = rng.integers(1, 8, (3, m)) / 4.0
        far = near + rng.choice([0.5, 1, 2, 4], (3, m))
        c["far"] = F32(8.5)                                                             # far - near = 8
    else:
        m = int(name.split("_")[0][1:])
        c["w2c"] = _pose(rng)
        c["K"] = f32([[37.5, 0.0, 9.3], [0.0, 41.25, 7.1], [0.0, 0.0, 1.0]])
        c["inv_scale"] = f32([19, 15])
        cam = np.stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.uniform(0.25, 4, m) * rng.choice([-1, 1], m)], -1)     # |c_z| >= 0.25
        if name == "m64_equal_range":
            cam[5, 2] = 2.0                                                              # q_z - near well away from zero: +inf on both sides
        M = c["w2c"].astype(F64)
        pts =(cam - M[:, 3]) @ M[:, :3] if c["has_w2c"] else cam
        near = rng.uniform(0.3, 1.0, (3, m))
        far = near + rng.uniform(0.5, 2.0, (3, m))
        if name == "m64_equal_range":
            far[1, 5] = near[1, 5]                                                       # one stage of one point: a division by zero
    if not c["nf_stride"]:
        near, far = near[:, :1], far[:, :1]
    c["m"], c["pts"] = m, f32(pts)
    for s in range(3):
        c["near_%d" % (s + 1)], c["far_%d" % (s + 1)] = f32(near[s]), f32(far[s])
    want, cz = ndc_project32(c)
    c["cz"] = cz
    if not lattice:
        assert float(np.abs(cz).min()) >= 0.24, name
    return _finish(c, want, ndc_project_ref(c))


def _clamp_case(c):
    """The camera-plane clamp, pinned on a lattice: w2c = a signed permutation with c_z = the point's z, so the depth of every point is the float
    given.  Depths: +-1e-4f exactly (NOT clamped: the comparison is strict), the floats on either side, 0, -0, +-2^-14 (inside), +-2^-13
    (outside), +-1.  The witness here is the oracle run in FLOAT32 (torch compares a float32 tensor with 1e-4 as 1e-4f, and its products are
    rounded one by one as the kernel's): bit for bit.  The float64 oracle is held to `bar` on every point but the two at exactly +-1e-4f, which
    the double threshold 1e-4 > 1e-4f clamps -- the one place where float64 is not what the reference computes."""
    t, up, dn = CLAMP, np.nextafter(CLAMP, F32(1)), np.nextafter(CLAMP, F32(0))
    depths = f32([t, -t, up, -up, dn, -dn, 0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -13, -2.0 ** -13, 1.0, -1.0])
    m = len(depths) * 3
    z = np.tile(depths, 3)
    xy = f32(np.stack([np.repeat([0.5, -1.25, 2.0], len(depths)), np.repeat([1.0, 0.75, -0.5], len(depths))], -1))
    c.update(m=m, pts=f32(np.concatenate([xy, z[:, None]], -1)), w2c=f32([[0, -1, 0, 2], [2, 0, 0, -1], [0, 0, 1, 0]]),
             K=f32([[4, 0, 2], [0, 8, 1], [0, 0, 1]]), inv_scale=f32([8, 4]), lattice=False)
    for s in range(3):
        c["near_%d" % (s + 1)], c["far_%d" % (s + 1)] = f32(np.full(m, 0.25 * (s + 1))), f32(np.full(m, 0.25 * (s + 1) + 2.0))
    want, cz = ndc_project32(c)
    c["cz"], c["depths"] = cz, z
    f32_oracle = ndc_project_ref(c, torch.float32)
    for k, w in want.items():
        assert same_bits(w, f32_oracle[k]), ("clamp", k)
    c["at_threshold"] = np.abs(z) == CLAMP
    ref = ndc_project_ref(c)
    for k in ref:                                                                       # the two points the double threshold decides otherwise: taken from float32
        ref[k] = np.where(c["at_threshold"][:, None], f32_oracle[k].astype(F64), ref[k])
    return _finish(c, want, ref)


# ================================================================================================ embed
EMBED_FREQS = (0, 1, 4, 10, 17, 30)
EMBED_MS = (1, 64, 65, 257)
EMBED_NAMES = tuple("L%d_lay%d_m%d" % (L, lay, EMBED_MS[(i + lay) % 4]) for i, L in enumerate(EMBED_FREQS) for lay in (0, 1)) + \
    ("L10_lay0_m65", "L4_lay1_m1", "L10_lay0_3d", "edges_lay0", "edges_lay1", "fixture_range_lay0")
QUADRANT_KS = tuple(list(range(0, 9)) + [100, 101, 102, 103, 1000, 4097, 16386, 30003] + list(range(32769, 32777)) + [36001, 40002, 41718, 41719, 41720, 41721])


def edge_arguments():
    """0, -0, every float within 4 ulp of k pi/2 and of (k + 1/2) pi/2 (both signs) for QUADRANT_KS, 64 (x 2^10 = 65536 exactly), the next
    float above 65536, the same two negative, +-inf, NaN, 600."""
    vals = [0.0, -0.0]
    for k in QUADRANT_KS:
        for centre in (k * math.pi / 2, (k + 0.5) * math.pi / 2):
            base = F32(centre)
            if abs(float(base)) > 65536.0:
                continue
            ring, lo, hi = [base], base, base
            for _ in range(4):
                lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
                ring += [lo, hi]
            vals += [float(v) for v in ring if abs(float(v)) <= 65536.0]
            vals += [-float(v) for v in ring if abs(float(v)) <= 65536.0]
    above = float(np.nextafter(SINCOS_FAST_MAX, F32(np.inf)))
    vals += [64.0, 65536.0, above, -64.0, -65536.0, -above, np.inf, -np.inf, np.nan, 600.0, -600.0]
    return f32(vals)


def embed32(x, L, layout):
    """-> out [m, 3 + 6 L] float32, slow [m, 3 + 6 L] bool (the slots whose argument took OCML's sincosf: filled from float64 here)."""
    x = f32(x).reshape(-1, 3)
    m = x.shape[0]
    out, slow = np.zeros((m, 3 + 6 * L), F32), np.zeros((m, 3 + 6 * L), bool)
    out[:, :3] = x
    for k in range(L):
        with np.errstate(all="ignore"):
            r = x * F32(1 << k)
            s, co = sincos_fast32(r)
            sl = is_slow(r)
            s, co = np.where(sl, np.sin(r.astype(F64)), s), np.where(sl, np.cos(r.astype(F64)), co)
        a, b = (3 + 3 * k, 3 + 3 * L + 3 * k) if layout == 0 else (3 + 6 * k, 3 + 6 * k + 3)
        out[:, a:a + 3], out[:, b:b + 3] = s, co
        slow[:, a:a + 3] = slow[:, b:b + 3] = sl
    return out, slow


@functools.lru_cache(maxsize=None)
def embed_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    shape = None
    if name.startswith("edges"):
        L, layout = 17, int(name[-1])
        v = edge_arguments()
        pad = (-len(v)) % 3
        x = np.concatenate([v, f32(rng.uniform(-1.3, 1.3, pad))]).reshape(-1, 3)
    elif name.startswith("fixture_range"):
        L, layout, x = 10, 0, f32(rng.uniform(-600, 600, (64, 3)))
    else:
        t = name.split("_")
        L, layout = int(t[0][1:]), int(t[1][3:])
        if t[2] == "3d":
            shape, x = (4, 5, 3), f32(rng.uniform(-1.3, 1.3, (20, 3)))
        else:
            x = f32(rng.uniform(-1.3, 1.3, (int(t[2][1:]), 3)))
    c = dict(kind="embed", name=name, lattice=False, n_freqs=L, layout=layout, x=x, m=x.shape[0], shape=shape or x.shape)
    out, slow = embed32(x, L, layout)
    c["slow"] = {"out": slow}
    with np.errstate(all="ignore"):
        ref = (O.embed_live if layout == 0 else O.embed_interleaved)(_t64(x), L).numpy()
    return _finish(c, {"out": out}, {"out": ref})


def embed_arguments(c):
    """[m, L, 3] float32: the sincos arguments x * 2^k of a case."""
    with np.errstate(all="ignore"):
        return f32(np.stack([c["x"] * F32(1 << k) for k in range(c["n_freqs"])], 1)) if c["n_freqs"] else np.zeros((c["m"], 0, 3), F32)


# ================================================================================================ all
KINDS = {"ray_gen": (RAY_GEN_NAMES, ray_gen_case), "ray_gen_sample": (RAY_GEN_SAMPLE_NAMES, ray_gen_sample_case),
         "ndc_rays": (NDC_RAYS_NAMES, ndc_rays_case), "dir_feature": (DIR_FEATURE_NAMES, dir_feature_case),
         "sample_stratified": (STRAT_NAMES, stratified_case), "sample_cascade": (CASCADE_NAMES, cascade_case),
         "ndc_project": (NDC_PROJECT_NAMES, ndc_project_case), "embed": (EMBED_NAMES, embed_case)}
ALL = tuple((kind, name) for kind, (names, _) in KINDS.items() for name in names)


def case(kind, name):
    return KINDS[kind][1](name)


def clear_caches():
    for _, fn in KINDS.values():
        fn.cache_clear()
