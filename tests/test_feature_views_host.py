"""Host-side checks of FeatureNet over all views in one pass (no GPU): the four grouped batch-norm symbols and their structs, every argument
check of the new entry points through ctypes (they come before anything is launched), the `groups` keyword of the ops, FeatureNet.forward_views
and CascadeMVSNet's `feature_views` keyword, forward_views against the per-view loop on the CPU, the per-view restatement of
tests/feature_views_cases.py against torch's own layers in float64, and the ReLU-side condition of the seeds the GPU module tests use."""
import ctypes as C
import inspect
import os

import pytest
import torch

import bn_cases as BC
import feature_views_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("ucnerf_bn_stats_groups", "ucnerf_bn_stats"), ("ucnerf_bn_apply_groups", "ucnerf_bn_apply"), ("ucnerf_bn_bwd_reduce_groups", "ucnerf_bn_bwd_reduce"),
         ("ucnerf_bn_bwd_apply_groups", "ucnerf_bn_bwd_apply"))
LIMIT = (1 << 31) - (1 << 20)                                              # the documented limit on N


def M():
    from uc_nerf_amd.network import mvs_models
    return mvs_models


@pytest.fixture(scope="module")
def L():
    from uc_nerf_amd.build import build
    build()
    from uc_nerf_amd import _lib
    _lib.lib()
    return _lib


def test_the_four_symbols_and_structs_are_registered_and_the_abi_stays_at_6(L):
    from uc_nerf_amd.build import CSRC, HEADERS, SOURCES
    hdr = open(os.path.join(ROOT, "include", "ucnerf_hip.h")).read()
    assert L.lib().ucnerf_abi_version() == 6 == L.ABI_VERSION and "#define UCNERF_ABI_VERSION 6" in hdr
    raw = C.CDLL(L.LIB_PATH)
    for name, plain in PAIRS:
        assert hasattr(raw, name) and name in L.SYMBOLS and "int %s(const %s_params* p, void* stream);" % (name, name) in hdr, name
        struct, base = L.ADDED_STRUCTS[name + "_params"], L.ADDED_STRUCTS[plain + "_params"]
        assert name + "_params" not in L.STRUCTS and "struct %s_params {" % name in hdr
        # the ungrouped counterpart's fields with an int64 G in front
        assert struct._fields_ == [("G", C.c_int64)] + base._fields_
        assert L.lib().ucnerf_sizeof((name + "_params").encode()) == C.sizeof(struct) == C.sizeof(base) + 8, name
    assert hdr.index("ucnerf_conv2d_bias_grad(") < hdr.index("struct ucnerf_bn_stats_groups_params {")       # appended: nothing above moved
    # one code path: a single batch-norm source with four kernels behind all eight entry points
    assert [f for f in sorted(os.listdir(CSRC)) if f.startswith("bn")] == ["bn.hip"] and "bn.hip" in SOURCES
    assert not any(os.path.basename(h).startswith("bn") for h in HEADERS)
    assert open(os.path.join(CSRC, "bn.hip")).read().count("__global__") == 4
    for name in sum(PAIRS, ()):
        assert C.cast(getattr(raw, name), C.c_void_p).value, name
    from uc_nerf_amd import ops
    from uc_nerf_amd.ops import cnn
    assert ops.BN_MAX_GROUPS is cnn.BN_MAX_GROUPS == VC.MAX_GROUPS
    for f in (ops.batch_norm_train, ops.batch_norm_train_bwd, ops.conv2d_bn_train):
        assert inspect.signature(f).parameters["groups"].default == 1, f


# ------------------------------------------------------------------------------------------------ argument checks before any device call
def _calls(L):
    one = (C.c_double * 2)(0, 0)
    addr = C.addressof(one)                                                # a non-null, 16-byte aligned host address: never dereferenced by a check
    lib = L.lib()

    def make(name, **kw):
        p = L.ADDED_STRUCTS[name + "_params"]()
        p.G, p.n, p.C, p.S = 2, 1, 3, 8
        for field, kind in p._fields_:
            if kind is C.c_void_p:
                setattr(p, field, addr)
        if hasattr(p, "workspace_triples"):
            p.workspace_triples = 1 << 40
        else:
            p.workspace_pairs = 1 << 40
        if hasattr(p, "eps"):
            p.eps = 1e-5
        if hasattr(p, "momentum"):
            p.momentum = 0.1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(name, **kw):
        p = make(name, **kw)
        return getattr(lib, name)(C.addressof(p), None), lib.ucnerf_last_error().decode()

    return call


@pytest.mark.parametrize("name", [p[0] for p in PAIRS])
def test_grouped_entries_refuse_bad_arguments_before_any_device_call(L, name):
    call = _calls(L)
    lib = L.lib()
    assert getattr(lib, name)(None, None) == -1 and "null params" in lib.ucnerf_last_error().decode()
    P = lambda n, S: lib.ucnerf_bn_partials(n, S)                          # noqa: E731
    space = "workspace_triples" if "bwd" not in name else "workspace_pairs"
    cases = [
        (dict(G=0), "G=0"), (dict(G=-1), "G=-1"), (dict(G=VC.MAX_GROUPS + 1), "G=65"),                        # the groups
        (dict(n=0), "at least 1"), (dict(C=0), "at least 1"), (dict(S=-1), "at least 1"),                     # everything the ungrouped entries refuse
        (dict(n=1, S=1), "at least 2"), (dict(n=1, S=LIMIT + 1), "values per channel"), (dict(n=1 << 16, S=1 << 16), "values per channel"),
        (dict(C=65536), "C=65536"), (dict(n=1 << 40), "values per channel"),
        (dict(G=2, n=1, S=LIMIT // 2 + 1), "over all groups"),                                                # G n S past the limit on N
        (dict(G=64, n=1 << 10, S=1 << 15, C=65535), "over all groups"),
        ({space: 2 * 3 * P(1, 8) - 1}, "workspace holds"),                                                    # a workspace below G C P
        (dict(G=3, n=1, C=4, S=4352, **{space: 3 * 4 * 2 - 1}), "workspace holds"),
        (dict(workspace=None), "null"), (dict(y=None), "null"),
        (dict(workspace=C.addressof((C.c_double * 2)(0, 0)) + 4), "8-byte aligned"),
    ]
    if "apply_groups" in name and "bwd" not in name:
        cases += [(dict(eps=0.0), "eps="), (dict(eps=float("nan")), "eps="), (dict(momentum=0.0), "momentum="), (dict(momentum=1.5), "momentum="),
                  (dict(out=None), "null"), (dict(weight=None), "null"), (dict(saved_mean=None), "null"), (dict(running_var=None), "null"),
                  (dict(num_batches_tracked=None), "null")]
    if "bwd" in name:
        cases += [(dict(eps=0.0), "eps="), (dict(g=None), "null"), (dict(saved_var=None), "null"), (dict(bias=None), "null")]
    if name == "ucnerf_bn_bwd_apply_groups":
        cases += [(dict(grad_y=None), "null"), (dict(grad_weight=None), "null"), (dict(grad_bias=None), "null")]
    for kw, word in cases:
        rc, msg = call(name, **kw)
        assert rc == -1 and word in msg, (name, kw, msg)
    assert P(1, 4352) == 2 and 64 * LIMIT < 1 << 62                      # (G n C S cannot overflow below the other limits: C <= 65535, G n S <= 2^31)


# ------------------------------------------------------------------------------------------------ the keywords
def test_groups_keyword_of_the_ops_is_checked_before_anything_else():
    from uc_nerf_amd import ops
    z = torch.zeros
    c8 = (z(8), z(8), z(8), z(8), z(1, dtype=torch.int64))
    for bad in (0, -1, 65, 2.0, "2", None, True):
        with pytest.raises(RuntimeError, match="groups="):
            ops.batch_norm_train(z(4, 8, 2, 2), *c8, groups=bad)
        with pytest.raises(RuntimeError, match="groups="):
            ops.batch_norm_train_bwd(z(4, 8, 2, 2), z(4, 8, 2, 2), z(8), z(8), z(8), z(8), groups=bad)
        with pytest.raises(RuntimeError, match="groups="):
            ops.conv2d_bn_train(z(4, 8, 4, 4), z(8, 8, 3, 3), *c8, groups=bad)
    for f in (lambda: ops.batch_norm_train(z(4, 8, 2, 2), *c8, groups=3), lambda: ops.conv2d_bn_train(z(4, 8, 4, 4), z(8, 8, 3, 3), *c8, groups=3),
              lambda: ops.batch_norm_train_bwd(z(4, 8, 2, 2), z(4, 8, 2, 2), z(3, 8), z(3, 8), z(8), z(8), groups=3)):
        with pytest.raises(RuntimeError, match="groups=3 does not divide"):
            f()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):         # one value per channel and group: torch's refusal of each call
        ops.batch_norm_train(z(4, 8, 1, 1), *c8, groups=4)
    for f in (lambda: ops.batch_norm_train(z(4, 8, 2, 2), *c8, groups=2), lambda: ops.conv2d_bn_train(z(4, 8, 4, 4), z(8, 8, 3, 3), *c8, groups=2),
              lambda: ops.batch_norm_train_bwd(z(4, 8, 2, 2), z(4, 8, 2, 2), z(2, 8), z(2, 8), z(8), z(8), groups=2)):
        with pytest.raises(RuntimeError, match="ROCm device"):             # a good keyword: the next check, no fall-back
            f()


def test_feature_views_keyword_is_checked_and_handed_down():
    m = M()
    for bad in ("bogus", None, True, "Batched", 1):
        with pytest.raises(ValueError, match="feature_views="):
            m.CascadeMVSNet.with_cnns(feature_views=bad)
        with pytest.raises(ValueError, match="feature_views="):
            m.CascadeMVSNet(feature=m.FeatureNet(8), cost_regularization=[m.CostRegNet(c, 8) for c in (32, 16, 8)], feature_views=bad)
    assert inspect.signature(m.CascadeMVSNet.with_cnns).parameters["feature_views"].default == "loop"
    sig = inspect.signature(m.CascadeMVSNet.__init__).parameters["feature_views"]
    assert sig.default == "loop" and sig.kind is inspect.Parameter.KEYWORD_ONLY
    assert m.CascadeMVSNet.with_cnns().feature_views == "loop" and m.CascadeMVSNet.with_cnns(feature_views="batched").feature_views == "batched"

    class Plain(torch.nn.Module):                                          # a caller's feature net without forward_views
        def forward(self, x):
            return {}

    regs = [m.CostRegNet(c, 8) for c in (32, 16, 8)]
    assert m.CascadeMVSNet(feature=Plain(), cost_regularization=regs).feature_views == "loop"
    with pytest.raises(ValueError, match="forward_views"):
        m.CascadeMVSNet(feature=Plain(), cost_regularization=regs, feature_views="batched")
    net = m.FeatureNet(8)
    for bad in (torch.zeros(2, 3, 3, 8, 8), torch.zeros(3, 8, 8), torch.zeros(0, 3, 8, 8), None):
        with pytest.raises(RuntimeError, match="forward_views"):
            net.forward_views(bad)


# ------------------------------------------------------------------------------------------------ the method on the CPU: the loop itself
@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("index", range(len(VC.MODULE_CASES)))
def test_forward_views_on_the_cpu_is_the_loop(index, mode, monkeypatch):
    from uc_nerf_amd import ops
    calls = []
    for name in ("conv2d_bn_train", "conv2d_train", "batch_norm_train", "conv2d_bias_relu"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    case = VC.MODULE_CASES[index]
    imgs, R = VC.module_inputs(case)
    a, b = (BC.randomise_train(M().FeatureNet(8, batch_stats="device", training="device"), case[1]) for _ in range(2))
    if mode == "eval":
        a.eval(), b.eval()
    X, Y = imgs.clone().requires_grad_(True), imgs.clone().requires_grad_(True)
    got = a.forward_views(X)
    loop = [b(Y[:, i]) for i in range(imgs.shape[1])]
    want = {k: torch.cat([o[k] for o in loop]) for k in VC.STAGES}
    assert not calls
    for k in VC.STAGES:
        assert got[k].shape == R[k].shape and torch.equal(got[k], want[k]), k
    for outs in (got, want):
        sum((outs[k] * R[k]).sum() for k in VC.STAGES).backward()
    assert torch.equal(X.grad, Y.grad)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), k

    def same_state(passes):
        state = b.state_dict()
        for k, v in a.state_dict().items():
            assert torch.equal(v, state[k]), k
        assert int(a.conv0[0].bn.num_batches_tracked) == (passes * imgs.shape[1] if mode == "train" else 0)

    same_state(1)
    with torch.no_grad():                                                  # the [V,3,H,W] form means the same
        again = a.forward_views(imgs[0])
        loop = [b(imgs[:, i]) for i in range(imgs.shape[1])]
    assert all(torch.equal(again[k], torch.cat([o[k] for o in loop])) for k in VC.STAGES)
    same_state(2)


# ------------------------------------------------------------------------------------------------ the restatement
def test_per_view_restatement_agrees_with_torch_layers_in_float64():
    case = VC.MODULE_CASES[0]
    imgs, R = VC.module_inputs(case)
    m = BC.randomise_train(M().FeatureNet(8), case[1])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.double()
    X = imgs.double().requires_grad_(True)
    outs = [m(X[:, i]) for i in range(imgs.shape[1])]
    sum((o[k] * R[k][i:i + 1].double()).sum() for i, o in enumerate(outs) for k in VC.STAGES).backward()
    r = VC.feature_views(imgs, sd, torch.float64, R)
    pairs = [(k, r["out"][k], torch.cat([o[k] for o in outs]).detach()) for k in VC.STAGES] + [("grad_x", r["grad_x"], X.grad)]
    grads = dict(m.named_parameters())
    assert len(grads) == 31 and set(grads) == set(r["grads"])
    pairs += [(k, r["grads"][k], p.grad) for k, p in grads.items()]
    for k, got, want in pairs:
        assert got.shape == want.shape and float((got - want).abs().max() / want.abs().max()) <= 1e-10, k
    after = m.state_dict()
    for k, v in r["sd"].items():                                           # the buffers after V forwards in ascending order
        if "running_" in k:
            assert float((v - after[k]).abs().max()) <= 1e-12 * max(1.0, float(after[k].abs().max())), k
        elif "num_batches" in k:
            assert int(v) == int(after[k]) == int(sd[k]) + imgs.shape[1], k


@pytest.mark.parametrize("index", range(len(VC.MODULE_CASES) + 1))
def test_no_relu_of_the_module_cases_sits_within_the_chain_bar_of_zero_in_any_view(index):
    case = (VC.MODULE_CASES + (VC.CASCADE_CASE,))[index]
    imgs, R = VC.module_inputs(case)
    m = BC.randomise_train(M().FeatureNet(8), case[1])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    r64, r32 = VC.feature_views(imgs, sd, torch.float64), VC.feature_views(imgs, sd, torch.float32)
    assert len(r64["views"]) == imgs.shape[1]
    bad = VC.relu_offenders(r64, r32)
    assert not bad, bad[:5]


def test_exact_backward_case_is_what_it_claims():
    for shape in VC.OP_SHAPES[:3]:
        G, n, C, spatial = shape
        y, go, mu, var, eps = VC.exact_backward_case(G, n, C, spatial, 41)
        assert y.dtype == var.dtype == torch.float32 and mu.shape == var.shape == (G, C)
        r = 1.0 / torch.sqrt(var.double() + float(torch.tensor(eps, dtype=torch.float32)))
        assert bool(((var + torch.tensor(eps)) == (var.double() + eps).float()).all())
        assert set(r.flatten().tolist()) <= {0.5, 1.0, 2.0} and bool((r.float() == 1.0 / torch.sqrt(var + eps)).all())
        d = y.double() - mu.double().repeat_interleave(n, 0).view((G * n, C) + (1,) * len(spatial))
        assert bool((d == d.round()).all()) and float(d.abs().max()) <= 4 and bool((go == go.round()).all())
        per_group = (go.double() * d).view((G, n, C, -1)).sum((1, 3)) * r
        assert float(per_group.abs().sum(0).max()) < 2 ** 24 and bool((per_group * 2 == (per_group * 2).round()).all())
