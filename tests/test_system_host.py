"""Host-side checks of `uc_nerf_amd.system.UCNeRFSystem` and of the restatement the step-target tests compare against.  No GPU: the modules are
built on the CPU, the scenes only hold their constants there, and the step functions are stubbed where a step would need the device."""
import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR

import system_cases as YC

CPU = torch.device("cpu")


def make_system(tmp_path=None, **over):
    from uc_nerf_amd.system import UCNeRFSystem
    if tmp_path is not None:
        over = dict(over, basedir=str(tmp_path))
    scene = YC.tiny_scene(CPU)
    return UCNeRFSystem(YC.tiny_args(CPU, **over), [scene], network_mvs=YC.tiny_mvs())


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", YC.GATHER_CASES, ids=YC.GATHER_IDS)
def test_step_targets_ref_is_torch_advanced_indexing(case):
    H, W, n_rays, patch_num, ps, n_total = case
    sd, sw, dpt = YC.gather_maps(H, W, seed=7)
    pix = YC.gather_coords(H, W, n_total, seed=8)
    assert pix[0].min() >= -H and pix[0].max() < H and pix[1].min() >= -W and pix[1].max() < W
    assert (pix < 0).any() and (pix[:, 0] == 0).all()                           # a wrap is among them, and the corner
    got = YC.step_targets_ref(sd, sw, dpt, pix, n_rays, patch_num, ps)
    tsd, tsw, tdpt, tpix = (torch.from_numpy(a) for a in (sd, sw, dpt, pix))
    patch_pts = patch_num * ps * ps
    want = (tsd[:, tpix[0, n_rays:], tpix[1, n_rays:]], tsw[:, tpix[0, n_rays:], tpix[1, n_rays:]],
            tdpt[:, tpix[0, :patch_pts], tpix[1, :patch_pts]].reshape(-1, ps, ps, 1))
    for g, w, shape in zip(got, want, ((1, n_total - n_rays), (1, n_total - n_rays), (patch_num, ps, ps, 1))):
        assert g.shape == tuple(w.shape) == shape
        assert np.array_equal(g.view(np.int32), w.numpy().view(np.int32))        # bit for bit: NaN, the infinities and -0.0 included
    # float32 coordinates holding the same whole numbers give the same picks
    again = YC.step_targets_ref(sd, sw, dpt, pix.astype(np.float32), n_rays, patch_num, ps)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))


def test_entry_point_checks_sizes_before_anything_is_launched():
    """ucnerf_step_targets without a device.  With both parts empty it returns success on a struct whose pointers are all NULL: the return
    sits in front of the pointer checks, and those in front of the launch, so nothing was launched.  With one element to write the same
    struct is refused (the launch is behind that check); negative and inconsistent counts are refused whatever the pointers."""
    import ctypes as C
    from uc_nerf_amd import _lib as L
    lib = L.lib()

    def call(**fields):
        p = L.StepTargetsParams()
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.ucnerf_step_targets(C.addressof(p), None), lib.ucnerf_last_error().decode()

    assert lib.ucnerf_step_targets(None, None) == -1
    assert call(H=5, W=7, n_total=6, n_rays=6, patch_num=0, patch_size=2)[0] == 0                  # n_total == n_rays and patch_num == 0
    assert call()[0] == 0
    rc, msg = call(H=5, W=7, n_total=7, n_rays=6, patch_num=0, patch_size=2)
    assert rc == -1 and "null pixel_coordinates" in msg
    rc, msg = call(H=5, W=7, n_total=6, n_rays=6, patch_num=1, patch_size=2)
    assert rc == -1 and "null pixel_coordinates" in msg
    for bad, word in ((dict(n_rays=-1), "negative"), (dict(patch_num=-1), "negative"), (dict(n_rays=16), "above n_total"),
                      (dict(patch_num=4), "more than the n_total"), (dict(patch_size=1 << 30), "more than the n_total"), (dict(coord_is_float=2), "coord_is_float"),
                      (dict(H=0), "no pixel")):
        f = dict(H=5, W=7, n_total=15, n_rays=6, patch_num=2, patch_size=2, sparse_depths=64, sparse_weights=64, dpt=64, pixel_coordinates=64,
                 target_depths=64, target_weights=64, patch_dpt=64)                                  # non-null dummies, never dereferenced
        f.update(bad)
        rc, msg = call(**f)
        assert rc == -1 and word in msg, (bad, rc, msg)


# ------------------------------------------------------------------------------------------------ optimiser and scheduler
@pytest.mark.parametrize("num_epochs", [1, 4])
def test_learning_rates_follow_a_fresh_cosine_annealing(num_epochs):
    system = make_system(num_epochs=num_epochs)
    (opt,), (sched,) = system.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    assert opt.param_groups[0]["params"] == system.grad_vars
    p = torch.nn.Parameter(torch.zeros(1))
    twin_opt = torch.optim.Adam([{"params": [p], "lr": system.args.lrate}], betas=(0.9, 0.999))
    twin = CosineAnnealingLR(twin_opt, T_max=num_epochs, eta_min=1e-7)
    for _ in range(num_epochs + 2):
        assert opt.param_groups[0]["lr"] == twin_opt.param_groups[0]["lr"]
        opt.step(), twin_opt.step()
        sched.step(), twin.step()
    assert opt.param_groups[0]["lr"] == twin_opt.param_groups[0]["lr"]


def test_finetune_keeps_the_mvs_network_out_of_the_optimiser():
    both, nerf_only = make_system(), make_system(finetune=True)
    n_mvs = len(list(both.Consist_Learner.parameters()))
    assert n_mvs > 0 and len(both.grad_vars) == len(nerf_only.grad_vars) + n_mvs
    mvs_ids = {id(p) for p in nerf_only.Consist_Learner.parameters()}
    assert not any(id(p) in mvs_ids for p in nerf_only.grad_vars)
    assert both.args.feat_dim == 24 + (YC.V - 1) * 12 + 1
    assert "network_mvs" not in both.render_kwargs_train and "N_samples" not in both.render_kwargs_train and both.render_kwargs_train["NDC_local"] is False


# ------------------------------------------------------------------------------------------------ the epoch order
def test_epoch_order_is_a_seeded_permutation_of_all_metas():
    system = make_system(num_train_samples=7)
    metas = system.train_metas(np.random.default_rng(0))
    assert len(metas) == 7 and all(s == 0 and t in (1, 3, 5) and len(src) == YC.V - 1 for s, t, src in metas)
    tagged = [(k,) + m for k, m in enumerate(metas)]                             # (equal metas may repeat: the tag tells them apart)
    a = system.epoch_order(tagged, np.random.default_rng(5))
    b = system.epoch_order(tagged, np.random.default_rng(5))
    c = system.epoch_order(tagged, np.random.default_rng(6))
    assert sorted(a) == sorted(tagged) and a == b and a != c and sorted(c) == sorted(tagged)
    assert system.train_metas(np.random.default_rng(0)) == metas
    assert [m[1] for m in system.val_metas()] == [0, 2, 4]


# ------------------------------------------------------------------------------------------------ fit's schedule
def test_fit_runs_the_sanity_step_then_trains_and_validates_every_second_epoch():
    system = make_system(num_epochs=4, num_train_samples=2)
    system.configure_optimizers()
    calls = []
    system._train_visit = lambda meta, k: calls.append("train")
    system._val_visit = lambda meta, k: calls.append("val")
    system.on_validation_epoch_end = lambda: calls.append("val_end") or {"epoch": system.current_epoch}
    real = system.scheduler.step
    system.scheduler.step = lambda: calls.append("sched") or real()
    results = system.fit(seed=3)
    epoch, val = ["train", "train", "sched"], ["val", "val", "val", "val_end"]
    assert calls == ["val", "val_end"] + epoch + epoch + val + epoch + epoch + val          # one sanity step, its epoch end discarded
    assert results == [{"epoch": 1}, {"epoch": 3}]
    del calls[:]
    assert system.fit(max_epochs=1, check_val_every_n_epoch=1, num_sanity_val_steps=0, seed=3) == [{"epoch": 0}]
    assert calls == epoch + val
    del calls[:]
    assert system.validate() == {"epoch": 0} and calls == val


# ------------------------------------------------------------------------------------------------ the checkpoint
def test_save_ckpt_writes_the_two_reference_keys_and_create_ucnerf_reloads_them(tmp_path):
    from uc_nerf_amd.network.models import create_ucnerf
    system = make_system(tmp_path)
    path = system.save_ckpt()
    assert path.endswith("tiny/ckpts//latest.tar")
    ckpt = torch.load(path, map_location="cpu")
    assert sorted(ckpt) == ["network_fn_state_dict", "network_mvs_state_dict"]
    args = YC.tiny_args(CPU, ckpt=path)
    args.feat_dim, args.network_mvs = system.args.feat_dim, YC.tiny_mvs()
    before = {k: v.clone() for k, v in args.network_mvs.state_dict().items()}
    kw, _, _, _ = create_ucnerf(args, dir_embedder=True, pts_embedder=True)          # load_state_dict's default is strict=True
    for (k, a), (_, b) in zip(kw["network_fn"].state_dict().items(), system.render_kwargs_train["network_fn"].state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(args.network_mvs.state_dict().items(), system.Consist_Learner.state_dict().items()):
        assert torch.equal(a, b), k
    assert any(not torch.equal(before[k], v) for k, v in args.network_mvs.state_dict().items())      # (the load changed the fresh net)
