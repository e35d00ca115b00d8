"""Cases for the launch modes of the MLP entry points (ucnerf_mlp_fwd, ucnerf_mlp_fwd_train, ucnerf_mlp_bwd): one set of inputs per case,
re-expressed in every addressing mode the params structs offer, with a poison value written wherever the kernels have no business reading a
meaning from.  Shared by tests/test_mlp_modes_host.py (CPU) and tests/test_hip_mlp_modes.py (GPU); seeded, cached, numpy / torch only, nothing
here touches a device.

A case holds n_src, m, S, dense float32 `pts` [m,3], `dirs` [m/S,3] (one per ray: dirs_per_sample = 0), `feats` [m,F] (confidence column in
[0,1]), `g_raw` [m,4] and a state dict (uc_nerf_amd.synthetic.init_ucnerf_state_dict, sigma_scale 0.1, sigma_bias 0.02).  Every sample of every
case keeps every relu pre-activation of the float32 oracle at least RELU_MARGIN * max|pre| away from zero (max over the unit's layer in
its sample, see margin_ratio): the builder draws candidate samples from its seeded stream and keeps the first that do (a relu then cannot fall the other way between two routes of the backward, whose data
gradients are compared bit for bit; tests/test_mlp_modes_host.py re-checks the condition on the finished case against the oracle's own output).

A mode helper returns a View: flat float32 buffers, each `Buf.data` exactly as long as the header (include/ucnerf_hip.h) prescribes for that
mode -- its rows, their stride gaps, the tile padding, plus the TAIL readable floats the weight-gradient launch's 16-byte pieces may reach
behind the last row -- and `Buf.mask`, true where the helper wrote the poison.  The device test appends GUARD floats of -7.0 to every
allocation; no pointer is ever handed over whose documented extent is not allocated."""
import functools

import numpy as np
import torch

from oracle import ucnerf_oracle as O
import rays_cases as RC

F32, F64 = np.float32, np.float64
GUARD, GUARD_VALUE = 64, F32(-7.0)
TAIL = 4                                   # readable floats behind the last row of an input (include/ucnerf_hip.h, "readable extent")
RELU_MARGIN = 1e-4                         # of max|pre| (margin_ratio); the builder selects with SELECT_MARGIN, stricter: the oracle's bits
SELECT_MARGIN = 2e-4                       # may depend on the batch shape it is evaluated in
PTS_STRIDE, DIRS_STRIDE, FEAT_PAD = 7, 5, 3

# name -> (n_src, m, S).  m: a single row, a tile less one, a full tile, a ragged tail of one (per-ray directions, S = 3), two tiles + 1,
# three full tiles (per-ray directions), three tiles + 1.  F = 24 + 12 n_src + 1 = 37 / 97 / 121: always odd, no row-major row is 16-byte aligned.
CASES = {"m1_v6": (6, 1, 1), "m31_v1": (1, 31, 1), "m32_v8": (8, 32, 1), "m33_S3_v6": (6, 33, 3), "m65_v1": (1, 65, 1),
         "m96_S3_v8": (8, 96, 3), "m97_v6": (6, 97, 1)}
NAMES = tuple(CASES)
POISONS = {"nan": np.array([0x7fc00000], np.uint32).view(F32)[0], "inf": F32(np.inf), "3e38": F32(3e38)}
UNUSED_PARAMS = ("nerf.pts_bias_confidence_1", "nerf.feature_linear_1", "nerf.confi_linear")      # the reference never uses these


def n_feat(n_src):
    return 24 + 12 * n_src + 1


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def same_bits(a, b):
    """int32 views equal: a NaN equals a NaN only if the bits are equal; -0.0 is not +0.0."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


class Buf:
    def __init__(self, data, mask):
        self.data, self.mask = np.ascontiguousarray(data, F32).reshape(-1), np.ascontiguousarray(mask, bool).reshape(-1)
        assert self.data.shape == self.mask.shape
        self.data.setflags(write=False); self.mask.setflags(write=False)


class View:
    """One addressing mode of a case.  `bufs`: name -> Buf; pts / dirs / feats: (buffer name, offset in floats); the struct fields of
    ucnerf_mlp_params that select the mode; `expect`: floats the helper meant to poison (gaps, padding, tails)."""

    def __init__(self, bufs, pts, dirs, feats, expect, S, dirs_per_sample=0, feats_tiled=0, encoded=0, pts_stride=0, dirs_stride=0, feat_stride=0):
        self.bufs, self.pts, self.dirs, self.feats, self.expect = bufs, pts, dirs, feats, expect
        self.fields = dict(S=S, dirs_per_sample=dirs_per_sample, feats_tiled=feats_tiled, encoded=encoded, pts_stride=pts_stride,
                           dirs_stride=dirs_stride, feat_stride=feat_stride)

    def poisoned(self):
        return sum(int(b.mask.sum()) for b in self.bufs.values())


def _fill(poison):
    return F32(0.0) if poison is None else F32(poison)


def _rows(x, stride, poison, tail=TAIL):
    """[n, w] rows `stride` floats apart, then `tail` floats: gaps and tail poisoned."""
    n, w = x.shape
    data = np.full(n * stride + tail, _fill(poison), F32)
    mask = np.ones(n * stride + tail, bool)
    body = data[:n * stride].reshape(n, stride)
    body[:, :w] = x
    mask[:n * stride].reshape(n, stride)[:, :w] = False
    return Buf(data, mask)


# ------------------------------------------------------------------------------------------------ the network, with its relu arguments
def forward_with_pre(sd, pts, dirs_ps, feats, n_src, layout="live"):
    """O.run_network_mvs (same operations in the same order, so the same bits) that also returns every relu argument: the six trunk layers,
    views / view_confi, and the sigma blend.  pts [m,3], dirs_ps [m,3] (per sample), feats [m,F] torch tensors of one dtype."""
    emb = O.embed_live if layout == "live" else O.embed_interleaved
    e_pts, e_dir = emb(pts[:, None], 10), emb(dirs_ps[:, None], 4)
    n_mvs = 24 + 4 * n_src
    f = feats[:, None]
    mvs, img = f[..., :n_mvs], f[..., n_mvs:n_mvs + 8 * n_src]
    u = 1 - f[..., -1:]
    b_depth, b_conf = O._lin(sd, "nerf.pts_bias_depth_fine", mvs), O._lin(sd, "nerf.pts_bias_confidence", img)
    pre, h = [], e_pts
    for i in range(6):
        a = O._lin(sd, "nerf.pts_linears.%d" % i, h) * b_depth
        pre.append(a)
        h = torch.relu(a)
        if i == 4:
            h = torch.cat([e_pts, h], -1)
    base_rgb, base_sigma = O._lin(sd, "nerf.confi_rgb_linear", h), O._lin(sd, "nerf.alpha_linear_1", h)
    h1 = torch.cat([O._lin(sd, "nerf.feature_linear", h * b_conf), e_dir], -1)
    a_v, a_c = O._lin(sd, "nerf.views_linears.0", h1), O._lin(sd, "nerf.view_confi_linears.0", h1)
    pre += [a_v, a_c]
    adapt_rgb, adapt_sigma = O._lin(sd, "nerf.rgb_linear", torch.relu(a_v)), O._lin(sd, "nerf.alpha_linear", torch.relu(a_c))
    rgb = torch.sigmoid(base_rgb * (1 - u) + adapt_rgb * u)
    a_s = adapt_sigma * (1 - u) + base_sigma * u
    pre.append(a_s)
    raw = torch.cat([rgb, torch.relu(a_s)], -1)[:, 0]
    return raw, torch.cat([p[:, 0] for p in pre], -1)


RELU_LAYERS = (128,) * 6 + (64, 64, 1)                # widths of the relu arguments forward_with_pre returns, in its order


def margin_ratio(pre):
    """|pre| / scale per sample, smallest over the sample's units -> [n].  The scale of a unit is max|pre| over ITS LAYER IN ITS SAMPLE: the
    rounding error of a pre-activation is relative to the row it is summed from (that sample's inputs to that layer), so this is the scale on
    which two evaluations of the same row can disagree.  (A case-wide max|pre| cannot be met by any sample: the modulated trunk is heavy-tailed
    -- max|pre| 445 against a median of 1.7 over 3000 random samples -- and 0 of 3000 candidates keep 897 units 0.045 away from zero.)  The one-unit
    sigma blend has no row to take a maximum over: its scale is the largest |blend| of the batch."""
    a, out, o = pre.abs(), None, 0
    for w in RELU_LAYERS:
        p = a[:, o:o + w]
        o += w
        r = (p / (p.max(-1, keepdim=True)[0] if w > 1 else p.max())).min(-1)[0]
        out = r if out is None else torch.minimum(out, r)
    return out


def relu_margin(c):
    """The smallest margin_ratio of the float32 oracle over every sample of the case (to be >= RELU_MARGIN)."""
    t = lambda a: torch.from_numpy(np.array(a))
    _, pre = forward_with_pre(c["sd"], t(c["pts"]), t(c["dirs_ps"]), t(c["feats"]), c["n_src"])
    return float(margin_ratio(pre).min())


@functools.lru_cache(maxsize=None)
def case(name):
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    n_src, m, S = CASES[name]
    F, n_rays = n_feat(n_src), m // S
    assert n_rays * S == m
    seed = 1000 + sum(map(ord, name))
    sd = init_ucnerf_state_dict(seed=seed, n_src=n_src, sigma_scale=0.1, sigma_bias=0.02)
    sd = {k: v.float() for k, v in sd.items()}
    gen = torch.Generator().manual_seed(seed)
    # candidates: per ray (one direction) K samples, of which the first S that keep the margin are taken -- about one sample in ten does;
    # a ray with fewer than S is passed over
    pool, K = 2 * n_rays + 6, 32 * S
    pts = torch.rand(pool, K, 3, generator=gen) * 1.2 - 0.1
    feats = torch.randn(pool, K, F, generator=gen)
    feats[..., -1] = torch.rand(pool, K, generator=gen)
    dirs = torch.nn.functional.normalize(torch.randn(pool, 3, generator=gen), dim=-1)
    g_raw = torch.randn(pool, K, 4, generator=gen)
    _, pre = forward_with_pre(sd, pts.reshape(-1, 3), dirs[:, None].expand(-1, K, -1).reshape(-1, 3), feats.reshape(-1, F), n_src)
    good = (margin_ratio(pre) >= SELECT_MARGIN).view(pool, K)
    rays = (good.sum(-1) >= S).nonzero()[:, 0]
    assert rays.numel() >= n_rays, "case %s: only %d of %d candidate rays hold %d samples that keep the relu margin; re-seed" % (name, rays.numel(), pool, S)
    keep = rays[:n_rays]
    col = torch.stack([good[r].nonzero()[:S, 0] for r in keep])                     # [n_rays, S] the samples taken of each ray
    take = lambda x: torch.gather(x[keep], 1, col[..., None].expand(-1, -1, x.shape[-1]))
    pts, feats, g_raw = take(pts), take(feats), take(g_raw)
    dirs = dirs[keep]
    c = dict(name=name, n_src=n_src, m=m, S=S, F=F, sd=sd, flat=torch.cat([v.reshape(-1) for v in sd.values()]).numpy().copy(),
             pts=pts.reshape(m, 3).numpy().copy(), dirs=dirs.numpy().copy(), feats=feats.reshape(m, F).numpy().copy(),
             g_raw=g_raw.reshape(m, 4).numpy().copy())
    c["dirs_ps"] = np.repeat(c["dirs"], S, 0)                # the same directions, one row per sample
    c["perm"] = np.random.default_rng(seed).permutation(m)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------ float64 / float32 oracle of a case
@functools.lru_cache(maxsize=None)
def oracle(name, layout="live"):
    """raw and the gradients of sum(raw * g_raw) from the oracle in float64 (`raw`, `g_feats`, `g_params` by name; None where the reference
    gives no gradient) and the float32 oracle's own distance from them (`raw32_dist`)."""
    c = case(name)
    m, S, F, n_src = c["m"], c["S"], c["F"], c["n_src"]
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(dt)
    out = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.to(dt).clone().requires_grad_(True) for k, v in c["sd"].items()}
        fo = t(c["feats"], dt).requires_grad_(True)
        raw = O.run_network_mvs(p, t(c["pts"], dt).view(m // S, S, 3), t(c["dirs"], dt), fo.view(m // S, S, F), n_src=n_src, layout=layout).reshape(m, 4)
        if dt == torch.float32:
            out["raw32_dist"] = float((raw.detach().double() - out["raw"]).abs().max())
            break
        (raw * t(c["g_raw"], dt)).sum().backward()
        out["raw"], out["g_feats"] = raw.detach(), fo.grad
        out["g_params"] = {k: (None if v.grad is None else v.grad) for k, v in p.items()}
    return out


def param_slices(c):
    """name -> slice of the flat parameter vector (state_dict order)."""
    out, off = {}, 0
    for k, v in c["sd"].items():
        out[k] = slice(off, off + v.numel())
        off += v.numel()
    return out


# ------------------------------------------------------------------------------------------------ the modes
def dense(c, poison=None, per_sample=False):
    d = c["dirs_ps"] if per_sample else c["dirs"]
    bufs = {"pts": _rows(c["pts"], 3, poison), "dirs": _rows(d, 3, poison), "feats": _rows(c["feats"], c["F"], poison)}
    return View(bufs, ("pts", 0), ("dirs", 0), ("feats", 0), 3 * TAIL, c["S"], dirs_per_sample=int(per_sample))


def strided(c, poison=None, feats_only=False):
    """pts rows 7 floats apart, dirs rows 5 apart, feats rows F + 3 apart (feats_only: pts / dirs stay dense -- the precisions and the
    backward that refuse strided raw coordinates)."""
    m, F, nd = c["m"], c["F"], c["dirs"].shape[0]
    ps, ds = (3, 3) if feats_only else (PTS_STRIDE, DIRS_STRIDE)
    bufs = {"pts": _rows(c["pts"], ps, poison), "dirs": _rows(c["dirs"], ds, poison), "feats": _rows(c["feats"], F + FEAT_PAD, poison)}
    expect = m * (ps - 3) + nd * (ds - 3) + m * FEAT_PAD + 3 * TAIL
    return View(bufs, ("pts", 0), ("dirs", 0), ("feats", 0), expect, c["S"], pts_stride=0 if feats_only else ps, dirs_stride=0 if feats_only else ds,
                feat_stride=F + FEAT_PAD)


def one_matrix(c, poison=None):
    """pts | feats | dirs as the columns of one [m, 3 + F + 3] matrix (directions per sample)."""
    F = c["F"]
    x = np.concatenate([c["pts"], c["feats"], c["dirs_ps"]], 1)
    W = 3 + F + 3
    return View({"x": _rows(x, W, poison)}, ("x", 0), ("x", 3 + F), ("x", 3), TAIL, c["S"], dirs_per_sample=1, pts_stride=W, dirs_stride=W, feat_stride=W)


@functools.lru_cache(maxsize=None)
def encodings(name, pe_layout):
    """The float32 restatement of ucnerf_embed (tests/rays_cases.py: bit for bit the device's) of the case's points and per-sample directions."""
    c = case(name)
    e_pts, slow_p = RC.embed32(c["pts"], 10, pe_layout)
    e_dir, slow_d = RC.embed32(c["dirs_ps"], 4, pe_layout)
    assert not slow_p.any() and not slow_d.any()
    return e_pts, e_dir


def encoded(c, pe_layout, poison=None):
    """[m, 63 + F + 27] rows (the reference's UCNeRF.forward(x) input), the three strides equal to the row width."""
    F = c["F"]
    e_pts, e_dir = encodings(c["name"], pe_layout)
    X = 63 + F + 27
    x = np.concatenate([e_pts, c["feats"], e_dir], 1)
    return View({"x": _rows(x, X, poison)}, ("x", 0), ("x", 63 + F), ("x", 63), TAIL, 1, dirs_per_sample=1, encoded=1, pts_stride=X, dirs_stride=X, feat_stride=X)


def tiled(c, poison=None, per_sample=False):
    """feats as [ceil(m / 32)][F][32]; the rows of the last tile behind sample m - 1 are padding."""
    m, F = c["m"], c["F"]
    mt = (m + 31) // 32 * 32
    ft = np.full((mt, F), _fill(poison), F32)
    ft[:m] = c["feats"]
    fm = np.ones((mt, F), bool)
    fm[:m] = False
    lay = lambda a: a.reshape(mt // 32, 32, F).transpose(0, 2, 1).reshape(-1)
    data = np.concatenate([lay(ft), np.full(TAIL, _fill(poison), F32)])
    mask = np.concatenate([lay(fm), np.ones(TAIL, bool)])
    d = c["dirs_ps"] if per_sample else c["dirs"]
    bufs = {"pts": _rows(c["pts"], 3, poison), "dirs": _rows(d, 3, poison), "feats": Buf(data, mask)}
    return View(bufs, ("pts", 0), ("dirs", 0), ("feats", 0), (mt - m) * F + 3 * TAIL, c["S"], dirs_per_sample=int(per_sample), feats_tiled=1)


def untile(data, m, F):
    mt = (m + 31) // 32 * 32
    return np.asarray(data)[:mt * F].reshape(mt // 32, F, 32).transpose(0, 2, 1).reshape(mt, F)[:m]


def subset(c, idx):
    """The case restricted to the samples `idx` (in that order), directions per sample: a permutation, a single sample, a prefix."""
    idx = np.asarray(idx)
    d = dict(c)
    d.update(m=len(idx), S=1, pts=c["pts"][idx], dirs=c["dirs_ps"][idx], dirs_ps=c["dirs_ps"][idx], feats=c["feats"][idx], g_raw=c["g_raw"][idx])
    return d


def inverse(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def read_rows(view, which, n, w):
    """The [n, w] rows a View addresses as pts / dirs / feats (row-major modes), read back out of its buffers."""
    name, off = getattr(view, which)
    stride = view.fields[which + "_stride" if which != "feats" else "feat_stride"] or w
    data = view.bufs[name].data
    return np.stack([data[off + i * stride: off + i * stride + w] for i in range(n)])


def g_feats_buffer(m, F, stride, col0, sentinel):
    """A g_feats destination of m rows `stride` floats apart whose F columns start at column col0: NaN where the call must write, `sentinel`
    (which must survive) everywhere else.  -> (data, mask of the sentinel floats)."""
    data = np.full(m * stride, _fill(sentinel), F32)
    mask = np.ones(m * stride, bool)
    data.reshape(m, stride)[:, col0:col0 + F] = POISONS["nan"]
    mask.reshape(m, stride)[:, col0:col0 + F] = False
    return data, mask
