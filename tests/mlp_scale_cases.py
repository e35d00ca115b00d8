"""Cases that carry the MLP kernels past one round of their persistent loops: batch sizes chosen from the device's CU count so that the
weight-gradient launch (csrc/mlp_wgrad.hip) and the gradient chain (csrc/mlp_bwd_chain.hip) reach every regime of their schedulers, with the
samples at which a scheduler can go wrong marked as HOT positions and 64-sample stage WINDOWS.  Shared by tests/test_mlp_scale_host.py (CPU) and
tests/test_hip_mlp_scale.py (GPU); seeded, cached, numpy / torch only, nothing here touches a device.  profiles/mlp_scale.md has the reasons.

The two launch formulas are restated here as plain functions of (m, cus) -- wgrad_launch (mlp_wgrad.hip:509-516) and launch_mlp_bwd_chain
(mlp_bwd_chain.hip:290, 564) -- together with the split of the weight-gradient grid into home blocks (mlp_wgrad.hip:120-130), which needs the
fifteen pairs' cost weights (mlp_bwd.hip:752-765, mlp_wgrad.hip:491).

Every batch size is 64 (stages - 1) + r with 33 <= r <= 63, r not a multiple of 8, and m a multiple of 10: the last stage is ragged inside an
octet and inside its second 32-sample tile, per-ray directions with S = 10 divide m, and m16 = m - m % 16 (the S = 16 calls' batch) has the same
number of stages.

A case holds per-ray directions `dirs10` [m / 10, 3] and `dirs16` [m16 / 16, 3]; `dirs_ps` [m, 3] is dirs16 one row per sample (rows from m16 on:
dirs10's), so that a call with per-sample directions and a call with S = 16 are the same function of the same numbers.  A one-hot call at sample
s uses dirs10[s // 10].  SPECIAL rows (the hot positions and the rows of the anchor window) keep every relu argument of the float32 oracle
SELECT_MARGIN away from zero under both of their directions (tests/mlp_modes_cases.py, margin_ratio): they are held to the float64 oracle.  Hot
rows also have a gradient that reaches every parameter tensor and a quarter of every trunk layer's columns (grad_reaches), which the float32
oracle itself gives within a quarter of the parity bar (float32_oracle_headroom)."""
import functools

import numpy as np
import torch

from oracle import ucnerf_oracle as O
import mlp_modes_cases as M

F32 = np.float32
WG_STAGE, WG_CHUNK_MAX, WG_LEAD, N_PAIRS = 64, 16, 4, 15
CHAIN_WAVES = 4
S_RAY, S_WIN = 10, 16
REGIMES = ("R1", "R2", "R3", "R4", "R5")
CASES = tuple((r, 6) for r in REGIMES) + (("R2", 1), ("R2", 8))          # (regime, n_src)
CASE_IDS = tuple("%s_v%d" % c for c in CASES)
TRIES = 400                                   # candidates looked at per special row before the builder gives up
TRUNK = ["nerf.pts_linears.%d" % i for i in range(6)]


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch formulas, restated
def stages_of(m):
    return cdiv(m, WG_STAGE)


def chunk_of(m, cus):
    c = N_PAIRS * stages_of(m) // (5 * cus)
    return min(max(c, 2), WG_CHUNK_MAX)


def chunks_of(m, cus):
    return cdiv(stages_of(m), chunk_of(m, cus))


def wgrad_blocks(m, cus):
    return min(cus, N_PAIRS * chunks_of(m, cus))


def chain_blocks(m, cus):
    return min(cus, cdiv(cdiv(m, 32), CHAIN_WAVES))


def chain_rounds(m, cus):
    return cdiv(cdiv(m, 32), CHAIN_WAVES * chain_blocks(m, cus))


def pair_costs(n_src):
    """(nout, width, 24-bit X) of the fifteen pairs in the order ucnerf_mlp_bwd adds them -> their cost weights."""
    n_mvs, n_img = 24 + 4 * n_src, 8 * n_src
    pairs = [(128, 128, 1), (128, 27, 0), (128, 128, 1), (128, n_img, 0), (128, 63, 0), (128, 128, 1)] + [(128, 128, 1)] * 4 + \
            [(128, 63, 0), (128, n_mvs, 0), (4, 128, 1), (3, 64, 1), (1, 64, 1)]
    r32 = lambda x: (x + 31) & ~31
    return [r32(n) * 3 // 4 + r32(w) * (3 if x24 else 4) // 4 + 224 for n, w, x24 in pairs]


def home_blocks(m, cus, n_src):
    """Per pair: (home blocks nb, chunks owned without asking ns * nb, chunks behind the counter)."""
    st, grid, chunks = stages_of(m), wgrad_blocks(m, cus), chunks_of(m, cus)
    prefix = np.concatenate([[0], np.cumsum([st * c for c in pair_costs(n_src)])])
    total = int(prefix[-1])
    fb = [cdiv(int(p) * grid, total) for p in prefix[:-1]] + [grid]
    out = []
    for p in range(N_PAIRS):
        nb = fb[p + 1] - fb[p]
        ns = min(chunks // nb, WG_LEAD) if nb > 0 else 0
        out.append((nb, ns * nb, chunks - ns * nb))
    return out


def m_of_stages(st):
    """64 (st - 1) + r, 33 <= r <= 63, m a multiple of 10, r no multiple of 8: the smallest such r."""
    for r in range(33, 64):
        m = WG_STAGE * (st - 1) + r
        if m % S_RAY == 0 and r % 8:
            return m
    raise AssertionError(st)


def regime_holds(regime, m, cus, n_src=6):
    """The defining inequalities of a regime."""
    st, ch, chunks = stages_of(m), chunk_of(m, cus), chunks_of(m, cus)
    ragged = m % WG_STAGE != 0 and m % 8 != 0
    tiles = cdiv(m, 32)
    partial = tiles % (CHAIN_WAVES * chain_blocks(m, cus)) != 0
    hb = home_blocks(m, cus, n_src)
    if regime == "R1":        # fewer blocks than CUs; some pair has more home blocks than chunks: a home block without a chunk
        return N_PAIRS * chunks < cus and ragged and chunks >= 2 and any(nb > chunks for nb, _, _ in hb)
    if regime == "R2":        # chunk 2; every pair owns WG_LEAD rows of chunks and keeps a remainder behind its counter; odd stage count
        return ch == 2 and st % 2 == 1 and ragged and all(chunks > WG_LEAD * nb and dyn > 0 for nb, _, dyn in hb)
    if regime == "R3":        # a chunk length strictly inside 2 .. 16, a short last chunk of at least two stages
        return 2 < ch < WG_CHUNK_MAX and st % ch >= 2 and ragged
    if regime == "R4":        # the chain walks two rounds, the second partial, with waves past the end in a block that has valid ones
        return chain_rounds(m, cus) == 2 and partial and tiles % CHAIN_WAVES != 0 and ragged
    if regime == "R5":        # the chunk length at its cap, a short last chunk, three chain rounds or more
        return ch == WG_CHUNK_MAX and st % WG_CHUNK_MAX >= 2 and chain_rounds(m, cus) >= 3 and partial and ragged
    raise KeyError(regime)


def regime_m(regime, cus, n_src=6):
    """The batch size of a regime on a device with `cus` compute units: R1 at half the chunks that would fill the grid, every other regime at
    the smallest stage count whose m (m_of_stages) satisfies regime_holds."""
    if regime == "R1":
        chunks = max(2, ((cus - 1) // N_PAIRS) // 2)
        m = m_of_stages(2 * chunks)
        assert regime_holds(regime, m, cus, n_src), (regime, m, cus)
        return m
    lo = {"R2": 3, "R3": cus // 2, "R4": 2 * cus, "R5": 2 * cus}[regime]
    for st in range(max(lo, 3), 40 * cus):
        m = m_of_stages(st)
        if regime_holds(regime, m, cus, n_src):
            return m
    raise AssertionError("no batch size lands in %s with %d CUs" % (regime, cus))


def describe(regime, m, cus, n_src=6):
    hb = home_blocks(m, cus, n_src)
    return ("%s v%d: m %d, %d stages (last %d samples), chunk %d, %d chunks (last %d stages), wgrad grid %d, home blocks %d..%d, chunks behind "
            "counters %d..%d, chain grid %d x %d rounds (last round %d tiles)"
            % (regime, n_src, m, stages_of(m), m - 64 * (stages_of(m) - 1), chunk_of(m, cus), chunks_of(m, cus),
               stages_of(m) - (chunks_of(m, cus) - 1) * chunk_of(m, cus), wgrad_blocks(m, cus), min(h[0] for h in hb), max(h[0] for h in hb),
               min(h[2] for h in hb), max(h[2] for h in hb), chain_blocks(m, cus), chain_rounds(m, cus),
               cdiv(m, 32) - (chain_rounds(m, cus) - 1) * CHAIN_WAVES * chain_blocks(m, cus)))


# ------------------------------------------------------------------------------------------------ positions
def chunk_marks(m, cus):
    """The chunks k = 1, middle, last - 1, last."""
    chunks = chunks_of(m, cus)
    return sorted({min(1, chunks - 1), chunks // 2, max(chunks - 2, 0), chunks - 1})


def hot_positions(regime, m, cus, seed):
    """name -> sample, the structural positions of a size (later names of the same sample are dropped)."""
    ch, st = chunk_of(m, cus), stages_of(m)
    out = {"s0": 0, "s31": 31, "s32": 32, "s63": 63, "s64": 64, "last stage first": (st - 1) * 64, "m-1": m - 1}
    for k in chunk_marks(m, cus):
        out["chunk%d first" % k] = k * ch * 64
        out["chunk%d last" % k] = min((k + 1) * ch * 64, m) - 1
    if regime in ("R4", "R5"):
        out["last chain round first"] = (chain_rounds(m, cus) - 1) * CHAIN_WAVES * chain_blocks(m, cus) * 32
        out["last chain round first - 1"] = out["last chain round first"] - 1
    rng = np.random.default_rng(seed)
    for i in range(3):
        out["random %d" % i] = int(rng.integers(0, m))
    seen, keep = set(), {}
    for k, s in out.items():
        assert 0 <= s < m, (k, s, m)
        if s not in seen:
            keep[k] = s
            seen.add(s)
    return keep


ANCHOR_WINDOW = "last whole stage"


def windows(m, cus):
    """name -> first sample of a whole 64-aligned stage: the stage holding each chunk boundary (the last stage of chunk k - 1 and the first of
    chunk k) and the last whole stage.  m is ragged, so the last whole stage is stages - 2."""
    ch, st = chunk_of(m, cus), stages_of(m)
    out = {}
    for k in chunk_marks(m, cus):
        if k * ch - 1 >= 0:
            out["before chunk%d" % k] = (k * ch - 1) * 64
        out["chunk%d first stage" % k] = k * ch * 64
    seen, keep = set(), {}
    for k, s in [(ANCHOR_WINDOW, (st - 2) * 64)] + list(out.items()):
        if s + 64 <= m - m % S_WIN and s not in seen:
            keep[k] = s
            seen.add(s)
    return keep


def probe_rows(m, cus, seed, n_random=120):
    """Rows of the forward probe: first and last row of the tiles around every boundary of a round of tiles, for the round lengths the forward
    launches can have (4, 8 or 16 waves' worth of tiles per CU on the whole device, and on 1 or 3 blocks), the first two and last two tiles,
    m - 1, and seeded random rows."""
    n_tiles = cdiv(m, 32)
    tiles = {0, 1, n_tiles - 2, n_tiles - 1}
    for per_round in sorted({w * b for w in (4, 8, 16) for b in (1, 3, cus)}):
        bounds = list(range(per_round, n_tiles, per_round))
        for b in (bounds[:2] + bounds[-2:]) if per_round < 4 * cus else bounds:
            tiles.update(t for t in (b - 2, b - 1, b, b + 1) if 0 <= t < n_tiles)
    rows = {m - 1}
    for t in tiles:
        rows.update((32 * t, min(32 * t + 31, m - 1)))
    rows.update(int(x) for x in np.random.default_rng(seed).integers(0, m, n_random))
    return np.array(sorted(rows))


# ------------------------------------------------------------------------------------------------ data
def t32(a):
    return torch.from_numpy(np.array(a, F32))


def sample_grads(sd, n_src, pts, d, feats, g_raw, dtype=torch.float32):
    """Autograd of sum(raw * g_raw) through the oracle for samples with per-sample directions -> (g_params by name, g_feats)."""
    n, F = pts.shape[0], feats.shape[1]
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    fo = t32(feats).to(dtype).requires_grad_(True)
    raw = O.run_network_mvs(p, t32(pts).to(dtype).view(n, 1, 3), t32(d).to(dtype), fo.view(n, 1, F), n_src=n_src).reshape(n, 4)
    (raw * t32(g_raw).to(dtype)).sum().backward()
    return {k: v.grad for k, v in p.items()}, fo.grad


def grad_reaches(g_params):
    """The condition on a hot sample: its gradient alone has a non-zero entry in every parameter tensor that receives a gradient at all, and at
    least a quarter of the 128 columns (output units: the rows of the weight gradient) of every trunk layer's are non-zero."""
    for k, g in g_params.items():
        if k.rsplit(".", 1)[0] in M.UNUSED_PARAMS:
            continue
        if g is None or not bool((g != 0).any()):
            return False
    return all(int((g_params[k + ".weight"] != 0).any(1).sum()) >= 32 for k in TRUNK)


HEADROOM = 4.0


def bar_ratios(got_params, got_feats, g64):
    """name -> (largest |got - want| / (atol + rtol |want|) of the tensor, its flat index) under the parity bar of
    test_hip_parity.py::test_mlp_backward_vs_oracle_autograd; `got_params`: name -> tensor / array (None entries are passed over)."""
    out = {}
    pairs = [("g_feats", got_feats, g64[1], 0.0)] + [(k, got_params[k], g64[0][k], 1e-7) for k in g64[0] if g64[0][k] is not None]
    for k, a, b, floor in pairs:
        a = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.array(a))
        r = ((a.double().reshape(-1) - b.reshape(-1)).abs() / (2e-4 * float(b.abs().max()) + floor + 2e-3 * b.reshape(-1).abs()))
        out[k] = (float(r.max()), int(r.argmax()))
    return out


def float32_oracle_headroom(sd, n_src, pts, d, feats, g_raw, g32=None):
    """A single sample's gradient is one product G[n] X[k] per weight, with nothing to average over.  Where a factor is ill-conditioned in
    float32 -- the recorded cases: raw (1 - raw) of a sigmoid output within 2e-5 of 1, whose float32 1 - raw has 12 to 300 ulp left
    (profiles/mlp_scale.md) -- every float32 evaluation, the oracle's own included, leaves the whole row of the gradient a relative error the
    parity bar (2e-4 max|g| + 2e-3 |g|, made for sums over a batch) does not take.  A hot sample is one whose FLOAT32 ORACLE gradient stays
    within 1 / HEADROOM of that bar of the float64 oracle's.  HEADROOM = 4 is the factor the suite already grants a kernel over the float32
    oracle's own distance (test_hip_parity.py::test_mlp_forward_vs_reference_golden, tests/test_hip_mlp_modes.py: 4 x raw32_dist): a kernel
    four times as far from float64 as the float32 oracle then still meets the bar."""
    g32 = g32 or sample_grads(sd, n_src, pts, d, feats, g_raw)
    g64 = sample_grads(sd, n_src, pts, d, feats, g_raw, torch.float64)
    return max(r for r, _ in bar_ratios({k: v.detach() for k, v in g32[0].items() if v is not None}, g32[1].detach(), g64).values()) <= 1.0 / HEADROOM


def trunk_margin(pre):
    a = pre[:, :768].abs().view(-1, 6, 128)
    return (a / a.max(-1, keepdim=True)[0]).min(-1)[0].min(-1)[0]


@functools.lru_cache(maxsize=None)
def case(regime, n_src, cus, filtered=True):
    """filtered = False: hot rows are taken without float32_oracle_headroom (the rows the parity bar was first missed on: see error_ratios)."""
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    m = regime_m(regime, cus, n_src)
    F, m16 = M.n_feat(n_src), m - m % S_WIN
    seed = 7000 + 10 * REGIMES.index(regime) + n_src
    sd = {k: v.float() for k, v in init_ucnerf_state_dict(seed=seed, n_src=n_src, sigma_scale=0.1, sigma_bias=0.02).items()}
    gen = torch.Generator().manual_seed(seed)
    draw_pts = lambda n: torch.rand(n, 3, generator=gen) * 1.2 - 0.1

    def draw_feats(n):
        f = torch.randn(n, F, generator=gen)
        f[:, -1] = torch.rand(n, generator=gen)
        return f
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    pts, feats = draw_pts(m).numpy(), draw_feats(m).numpy()
    dirs10, dirs16 = unit(m // S_RAY).numpy(), unit(m16 // S_WIN).numpy()
    dirs_ps = np.concatenate([np.repeat(dirs16, S_WIN, 0), np.repeat(dirs10, S_RAY, 0)[m16:]])
    g_raw = torch.randn(m, 4, generator=gen).numpy()
    hot, win = hot_positions(regime, m, cus, seed), windows(m, cus)

    # candidates whose trunk keeps the margin (six of the nine relu layers, none of which sees the direction)
    n_pool = 4096
    cp, cf = draw_pts(n_pool), draw_feats(n_pool)
    _, pre = M.forward_with_pre(sd, cp, unit(1).expand(n_pool, 3), cf, n_src)
    pool = iter((trunk_margin(pre) >= M.SELECT_MARGIN).nonzero()[:, 0].tolist())

    def place(s, need_grad):
        ds = [dirs10[s // S_RAY]] + ([dirs16[s // S_WIN]] if s < m16 else [])
        for _ in range(TRIES):
            i = next(pool, None)
            assert i is not None, "%s v%d: the candidate pool ran out at sample %d; enlarge n_pool" % (regime, n_src, s)
            good = True
            for d in ds:
                _, pre = M.forward_with_pre(sd, cp[i:i + 1], t32(d)[None], cf[i:i + 1], n_src)
                good = good and float(M.margin_ratio(pre)) >= M.SELECT_MARGIN
            if good and need_grad:
                one = (cp[i:i + 1].numpy(), ds[0][None], cf[i:i + 1].numpy(), g_raw[s:s + 1])
                g32 = sample_grads(sd, n_src, *one)
                good = grad_reaches(g32[0]) and (not filtered or float32_oracle_headroom(sd, n_src, *one, g32=g32))
            if good:
                pts[s], feats[s] = cp[i].numpy(), cf[i].numpy()
                return
        raise AssertionError("%s v%d: no candidate in %d tries for sample %d" % (regime, n_src, TRIES, s))

    a0 = win[ANCHOR_WINDOW]
    special = set(hot.values())
    for s in range(a0, a0 + 64):
        if s not in special:
            place(s, False)
    for s in hot.values():
        place(s, True)
    c = dict(key=(regime, n_src, filtered), regime=regime, n_src=n_src, cus=cus, m=m, m16=m16, F=F, sd=sd, flat=torch.cat([v.reshape(-1) for v in sd.values()]).numpy().copy(),
             pts=pts, feats=feats, dirs10=dirs10, dirs16=dirs16, dirs_ps=dirs_ps, g_raw=g_raw, hot=hot, windows=win,
             probe=probe_rows(m, cus, seed), prefill=np.random.default_rng(seed + 1).standard_normal(sum(v.numel() for v in sd.values())).astype(F32))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def hot_sample(c, s):
    """The single-sample call of hot position s: (pts [1,3], direction [1,3] of its ray, feats [1,F], g_raw [1,4])."""
    return c["pts"][s:s + 1], c["dirs10"][s // S_RAY][None], c["feats"][s:s + 1], c["g_raw"][s:s + 1]


def window_samples(c, s0):
    """The 64-sample call of the window at s0, directions per sample."""
    w = slice(s0, s0 + 64)
    return c["pts"][w], c["dirs_ps"][w], c["feats"][w], c["g_raw"][w]


def bias_sum_bounds(c, s0):
    """name of every bias -> an upper bound of sum over the window's samples of |the DEVICE's gradient of it from that sample alone|, i.e. of
    sum_s |G_dev[s][n]|.  The float64 oracle gives G64[s][n] (the bias of every layer is given one copy per sample, whose gradient is the
    sample's row of G); a single-sample device call is held to the parity bar (2e-4 max_n |G64[s]| + 1e-7 + 2e-3 |G64[s][n]|, the anchor test),
    so |G_dev[s][n]| <= 1.002 |G64[s][n]| + 2e-4 max_n |G64[s]| + 1e-7, summed over the 64 samples."""
    pts, d, feats, g_raw = window_samples(c, s0)
    n, F, dt = 64, c["F"], torch.float64
    p = {k: v.to(dt) for k, v in c["sd"].items()}
    per = {}
    for k in list(p):
        if k.endswith(".bias"):
            per[k] = p[k].expand(n, 1, -1).clone().requires_grad_(True)
            p[k] = per[k]
    raw = O.run_network_mvs(p, t32(pts).to(dt).view(n, 1, 3), t32(d).to(dt), t32(feats).to(dt).view(n, 1, F), n_src=c["n_src"]).reshape(n, 4)
    (raw * t32(g_raw).to(dt)).sum().backward()
    out = {}
    for k, v in per.items():
        if v.grad is None:
            out[k] = None
            continue
        g = v.grad.abs()[:, 0]                                   # [64, width]
        out[k] = (1.002 * g.sum(0) + (2e-4 * g.max(1)[0] + 1e-7).sum()).numpy()
    return out
