"""The builder of tests/mlp_scale_cases.py, checked without a device: it is deterministic, its positions and windows lie where it says, the
batch size it picks for a CU count satisfies the inequalities that define each regime, every hot sample's gradient reaches every parameter
tensor, and the relation the device tests rest on -- the gradient of a batch whose g_raw is zero outside one sample is that sample's own -- holds
for the oracle in float64."""
import numpy as np
import pytest
import torch

import mlp_modes_cases as M
import mlp_scale_cases as SC

CUS = (256, 304, 64)
HOST_CUS = 256                                 # the data of the cases is checked for one CU count (the sizes for all three)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("regime,n_src", SC.CASES)
def test_regime_inequalities_hold(regime, n_src, cus):
    m = SC.regime_m(regime, cus, n_src)
    print(SC.describe(regime, m, cus, n_src))
    assert SC.regime_holds(regime, m, cus, n_src)
    st, ch = SC.stages_of(m), SC.chunk_of(m, cus)
    assert m % SC.S_RAY == 0 and 33 <= m - 64 * (st - 1) <= 63 and (m % 8) != 0 and SC.stages_of(m - m % SC.S_WIN) == st
    assert ch == min(max(15 * st // (5 * cus), 2), 16)
    tiles = SC.cdiv(m, 32)
    assert SC.chain_rounds(m, cus) == SC.cdiv(tiles, 4 * min(cus, SC.cdiv(tiles, 4)))
    if regime != "R1":                         # the smallest: no smaller stage count of the same shape lands in the regime
        lo = {"R2": 3, "R3": cus // 2, "R4": 2 * cus, "R5": 2 * cus}[regime]
        assert not any(SC.regime_holds(regime, SC.m_of_stages(s), cus, n_src) for s in range(max(lo, 3), st))
    assert sum(nb for nb, _, _ in SC.home_blocks(m, cus, n_src)) == SC.wgrad_blocks(m, cus)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("regime", SC.REGIMES)
def test_positions_and_windows_are_in_range_and_aligned(regime, cus):
    m = SC.regime_m(regime, cus)
    st, ch, chunks = SC.stages_of(m), SC.chunk_of(m, cus), SC.chunks_of(m, cus)
    hot, win = SC.hot_positions(regime, m, cus, 1), SC.windows(m, cus)
    assert hot == SC.hot_positions(regime, m, cus, 1) and list(hot) == list(SC.hot_positions(regime, m, cus, 1))
    assert all(0 <= s < m for s in hot.values()) and len(set(hot.values())) == len(hot)
    for s in (0, 31, 32, 63, 64, m - 1, (st - 1) * 64, (chunks - 1) * ch * 64, (chunks - 1) * ch * 64 - 1, ch * 64, min(2 * ch * 64, m) - 1):
        assert s in hot.values(), s
    if regime in ("R4", "R5"):
        first = (SC.chain_rounds(m, cus) - 1) * 4 * SC.chain_blocks(m, cus) * 32
        assert first in hot.values() and first - 1 in hot.values() and first < m
    assert all(s % 64 == 0 and s + 64 <= m - m % 16 for s in win.values()) and len(set(win.values())) == len(win)
    assert win[SC.ANCHOR_WINDOW] == (st - 2) * 64
    for s in ((chunks - 1) * ch * 64, (chunks - 1) * ch * 64 - 64, ch * 64, ch * 64 - 64):
        assert s in win.values() or s + 64 > m - m % 16, s              # (a one-stage last chunk is the ragged stage: no whole window)
    rows = SC.probe_rows(m, cus, 1)
    assert (np.diff(rows) > 0).all() and rows[0] == 0 and rows[-1] == m - 1 and (regime not in ("R4", "R5") or 200 <= len(rows) <= 400)
    assert (rows == SC.probe_rows(m, cus, 1)).all()


@pytest.mark.parametrize("regime,n_src", SC.CASES)
def test_builder_is_deterministic_and_hot_samples_reach_every_parameter(regime, n_src):
    c = SC.case(regime, n_src, HOST_CUS)
    SC.case.cache_clear()
    d = SC.case(regime, n_src, HOST_CUS)
    for k in ("pts", "feats", "dirs10", "dirs16", "dirs_ps", "g_raw", "flat", "probe", "prefill"):
        assert M.same_bits(c[k], d[k]) if c[k].dtype == np.float32 else (c[k] == d[k]).all(), k
    assert c["hot"] == d["hot"] and c["windows"] == d["windows"]
    m, m16 = c["m"], c["m16"]
    assert (c["dirs_ps"][:m16] == np.repeat(c["dirs16"], 16, 0)).all() and (c["dirs_ps"][m16:] == np.repeat(c["dirs10"], 10, 0)[m16:]).all()
    assert np.isfinite(c["pts"]).all() and np.isfinite(c["feats"]).all() and (c["feats"][:, -1] >= 0).all() and (c["feats"][:, -1] <= 1).all()
    t = SC.t32
    for name, s in c["hot"].items():
        pts, dr, feats, g_raw = SC.hot_sample(c, s)
        assert SC.grad_reaches(SC.sample_grads(c["sd"], n_src, pts, dr, feats, g_raw)[0]), name
        assert SC.float32_oracle_headroom(c["sd"], n_src, pts, dr, feats, g_raw), name
        for d_ in [dr] + ([c["dirs16"][s // 16][None]] if s < m16 else []):
            _, pre = M.forward_with_pre(c["sd"], t(pts), t(d_), t(feats), n_src)
            assert float(M.margin_ratio(pre)) >= M.RELU_MARGIN, name
    a0 = c["windows"][SC.ANCHOR_WINDOW]
    pts, dr, feats, _ = SC.window_samples(c, a0)
    _, pre = M.forward_with_pre(c["sd"], t(pts), t(dr), t(feats), n_src)
    assert float(M.margin_ratio(pre).min()) >= M.RELU_MARGIN


def test_a_dead_unit_is_noticed():
    """grad_reaches refuses a gradient with an empty tensor or with fewer than 32 live units in a trunk layer."""
    c = SC.case("R1", 6, HOST_CUS)
    g, _ = SC.sample_grads(c["sd"], 6, *SC.hot_sample(c, 0))
    assert SC.grad_reaches(g)
    h = dict(g)
    h["nerf.alpha_linear.weight"] = torch.zeros_like(g["nerf.alpha_linear.weight"])
    assert not SC.grad_reaches(h)
    h = dict(g)
    w = g["nerf.pts_linears.3.weight"].clone()
    w[31:] = 0
    h["nerf.pts_linears.3.weight"] = w
    assert not SC.grad_reaches(h)


@pytest.mark.parametrize("n_src", (1, 6, 8))
def test_one_hot_batch_gradient_is_the_samples_own_in_float64(n_src):
    """The relation itself, independent of any device: 97 samples, g_raw zero outside sample 70, per-ray directions (S = 10 would not divide
    97: per sample here) -- every parameter gradient and row 70 of the feature gradient equal the single-sample call's to 1e-13 of their
    scale (float64 sums 96 exact zeros; BLAS may block the products differently in the two shapes), every other feature row is exactly zero."""
    c = SC.case("R2", n_src, HOST_CUS)
    idx, s = np.arange(97), 70
    g_raw = np.zeros((97, 4), np.float32)
    g_raw[s] = c["g_raw"][s]
    gp_b, gf_b = SC.sample_grads(c["sd"], n_src, c["pts"][idx], c["dirs_ps"][idx], c["feats"][idx], g_raw, torch.float64)
    gp_1, gf_1 = SC.sample_grads(c["sd"], n_src, c["pts"][s:s + 1], c["dirs_ps"][s:s + 1], c["feats"][s:s + 1], g_raw[s:s + 1], torch.float64)
    assert torch.count_nonzero(gf_b[:s]) == 0 and torch.count_nonzero(gf_b[s + 1:]) == 0
    torch.testing.assert_close(gf_b[s], gf_1[0], rtol=0, atol=1e-13 * float(gf_1.abs().max()))
    for k in gp_1:
        if gp_1[k] is None:
            assert gp_b[k] is None
        else:
            torch.testing.assert_close(gp_b[k], gp_1[k], rtol=0, atol=1e-13 * float(gp_1[k].abs().max()) + 1e-300)
