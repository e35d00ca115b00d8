"""The masked source repack (ucnerf_gather_repack_masked) and the renderer's "bring the copies up to date" mode built on it.

  * the native call: for every one of the 32 masks the selected sources get the very bytes of the full repack, everything else in the buffer is
    not written;
  * CoarseFineRenderer.render(repack=True): a source written in place is copied again, the others are not, and the render equals a freshly built
    renderer's bit for bit; re-allocation, `.data` writes + repack="force", graph capture, and a short random sequence of state changes.

Shapes: 32 x 40 images, cascade volumes of 480 / 1280 / 2560 voxels (the first is no multiple of the 256-thread block), 2 or 6 source views,
33 rays x 8 + 16 samples.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, N_RAYS, NC, NF = 32, 40, 33, 8, 16
POISON = 0x3F000000                      # (0.5f in every word: no source region looks like that, and a render that reads it is an ordinary render)
NAN_PATTERN = 0x7FC0DEAD
SOURCES = ("vols0", "vols1", "vols2", "img_feat", "imgs")


def _scene(V, seed=0):
    from uc_nerf_amd.synthetic import make_scene, scene_to
    return scene_to(make_scene(seed=seed, H=H, W=W, V=V, small_volumes=True), torch.device(DEV))


def _clone(scene):
    return {k: ([t.clone() for t in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in scene.items()}


def _flat(V, seed=0):
    from uc_nerf_amd.pipeline import flat_params_of
    from uc_nerf_amd.synthetic import init_ucnerf_state_dict
    return flat_params_of(init_ucnerf_state_dict(seed=seed, n_src=V - 1, sigma_scale=0.05, sigma_bias=0.05)).to(DEV)


def _renderer(scene, flat, precision="bf16x3_fused", **kw):
    from uc_nerf_amd.pipeline import CoarseFineRenderer
    return CoarseFineRenderer(scene, flat, NC, NF, precision=precision, **kw)


def _rays(seed=1):
    from uc_nerf_amd.synthetic import random_pixels
    xs, ys = random_pixels(N_RAYS, H, W, seed=seed)
    noise = torch.rand(N_RAYS, NC, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return dict(xs=xs.to(DEV), ys=ys.to(DEV), perturb=1.0, noise=noise)


def _source(scene, k):
    return scene["vols"][k] if k < 3 else scene["img_feat"] if k == 3 else scene["imgs"]


def _assert_same(got, want, where=""):
    """Every tensor of a render's dict (the nested coarse dict included), bit for bit: float32 tensors as their 32-bit words (a ray that hits
    nothing has disp = NaN in both renders, which torch.equal on the values would call different)."""
    assert set(got) == set(want), (where, sorted(got), sorted(want))
    for k, v in want.items():
        if isinstance(v, dict):
            _assert_same(got[k], v, where + k + ".")
        elif torch.is_tensor(v):
            g = got[k]
            assert g.dtype == v.dtype and g.shape == v.shape, where + k
            assert torch.equal(_bits(g), _bits(v)) if v.dtype == torch.float32 else torch.equal(g, v), where + k


def _regions(src):
    """[(start, stop)] per source, in floats of src._cl: the layout of ucnerf_gather_repack (volumes, image features, colours; a source read in
    place takes no room), computed here from the shapes."""
    half = 2 if src.cl_bf16 else 1
    px = src.V * src.H * src.W
    counts = [8 * v.shape[1] * v.shape[2] * v.shape[3] for v in src.vols] + [8 * px, 4 * px]
    out, at = [], 0
    for k, c in enumerate(counts):
        n = 0 if src.inplace[k] else (c // half + 3) // 4 * 4
        out.append((at, at + n))
        at += n
    return out, at


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1: the native call
@pytest.mark.parametrize("V, bf16, inplace", [(3, False, ()), (7, False, ()), (3, True, ()), (3, False, (1, 4))],
                         ids=["V3", "V7", "V3-bf16", "V3-two-in-place"])
def test_masked_repack_writes_the_full_repacks_bytes_and_nothing_else(V, bf16, inplace):
    """All 32 masks.  Buffer A: the full repack of the NEW source values over a NaN pattern; buffer A0: of the OLD ones.  Buffer B: the pattern,
    a full repack of the old values, then the masked repack of the new ones.  Per source region B must equal A where the bit is set and A0 where
    it is clear -- as raw 32-bit words -- and the whole buffer, region by region, is covered: a row table or a grid sized wrongly would leave a
    selected source short (480 voxels are less than one block, 2560 pixels are ten) or write into a neighbour.  Mask 0 writes nothing at all.
    In-place sources (the last case) take no room and a mask that names them is not an error."""
    from uc_nerf_amd import _lib as L
    scene = _clone(_scene(V))
    if 1 in inplace:
        scene["vols"][1] = scene["vols"][1].contiguous(memory_format=torch.channels_last_3d)
    if 4 in inplace:
        scene["imgs"] = scene["imgs"][0].contiguous(memory_format=torch.channels_last).unsqueeze(0)
    r = _renderer(scene, _flat(V), precision="f32", sources_bf16=bf16)
    src, p = r.src, r.pass_.p
    assert [k for k in range(5) if src.inplace[k]] == list(inplace)
    p.cl = src.cl_inplace
    regions, n = _regions(src)
    assert n == L.lib().ucnerf_gather_repack_floats(C.addressof(p))
    assert (regions[0][1] - regions[0][0]) * (2 if bf16 else 1) // 8 % 256 != 0          # a source that is no whole number of blocks
    tensors = [_source(scene, k) for k in range(5)]
    old = [t.clone() for t in tensors]
    new = [t * 1.5 + 0.25 for t in tensors]

    def put(values):
        with torch.no_grad():
            for t, v in zip(tensors, values):
                t.copy_(v)

    def repack(buf, mask=None):
        out = L.ClSources()
        stream = torch.cuda.current_stream().cuda_stream
        if mask is None:
            L.check(L.lib().ucnerf_gather_repack(C.addressof(p), buf.data_ptr(), C.addressof(out), stream), "ucnerf_gather_repack")
        else:
            L.check(L.lib().ucnerf_gather_repack_masked(C.addressof(p), buf.data_ptr(), C.addressof(out), mask, stream), "ucnerf_gather_repack_masked")
        return out

    def pattern():
        return torch.full((n,), NAN_PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)

    put(old)
    a0 = pattern()
    repack(a0)
    put(new)
    a = pattern()
    lay = repack(a)
    assert not (_bits(a) == NAN_PATTERN).any() and not (_bits(a0) == NAN_PATTERN).any()      # (sizes are whole float4s: the regions tile the buffer)
    for k, (lo, hi) in enumerate(regions):                                                   # the layout is the one this test computed
        ptr = lay.vol[k] if k < 3 else lay.img_feat if k == 3 else lay.imgs
        if not src.inplace[k]:
            assert ptr == a.data_ptr() + 4 * lo, k
            assert not torch.equal(_bits(a[lo:hi]), _bits(a0[lo:hi])), k
    for mask in range(32):
        put(old)
        b = pattern()
        repack(b)
        assert torch.equal(_bits(b), _bits(a0))
        put(new)
        before = b.clone()
        got = repack(b, mask)
        assert (got.rgb_stride, got.bf16) == (lay.rgb_stride, lay.bf16)                      # the entries are those of the full repack, whatever the mask
        for k in range(5):
            mine, full = (x.vol[k] if k < 3 else x.img_feat if k == 3 else x.imgs for x in (got, lay))
            assert (mine == full) if src.inplace[k] else (mine - b.data_ptr() == full - a.data_ptr()), (mask, k)
        if mask == 0:
            assert torch.equal(_bits(b), _bits(before))
        for k, (lo, hi) in enumerate(regions):
            want = a if mask >> k & 1 else a0
            assert torch.equal(_bits(b[lo:hi]), _bits(want[lo:hi])), "mask %#x source %d" % (mask, k)


# ------------------------------------------------------------------------------------------------ 2: up to date
def _write(scene, what):
    with torch.no_grad():
        if what == "copy_":
            scene["vols"][2].copy_(scene["vols"][2] * 0.5 + 1.0)
            return [2]
        for k in what:
            _source(scene, k).mul_(2)
    return list(what)


@pytest.mark.parametrize("V", [3, 7])
@pytest.mark.parametrize("what", [(0,), (1,), (2,), (3,), (4,), (1, 4), "copy_"], ids=lambda w: w if isinstance(w, str) else "+".join(SOURCES[k] for k in w))
def test_render_refreshes_what_changed_and_only_that(V, what):
    """render -> write sources in place -> render: the second render equals a FRESH renderer's on the changed scene in every returned tensor.
    That only the written sources were copied again is read off the buffer: the copies of the others are overwritten with a recognisable value
    before a render and must still hold it afterwards, while the written sources' regions hold the full repack's bytes."""
    scene, flat, rays = _clone(_scene(V)), _flat(V), _rays()
    r = _renderer(scene, flat)
    r.render(**rays)
    gen = r.src._cl_gen
    assert r.src.stale_mask() == 0
    changed = _write(scene, what)
    assert r.src.stale_mask() == sum(1 << k for k in changed)
    fresh = _renderer(_clone(scene), flat)
    want = fresh.render(**rays)
    regions, n = _regions(r.src)
    cl = r.src._cl
    keep = cl.clone()
    for k, (lo, hi) in enumerate(regions):
        if k not in changed:
            _bits(cl)[lo:hi] = POISON
    r.render(**rays)                                             # (its result read the poison: not looked at)
    for k, (lo, hi) in enumerate(regions):
        if k in changed:
            assert torch.equal(_bits(cl[lo:hi]), _bits(fresh.src._cl[lo:hi])), "source %d was not refreshed" % k
        else:
            assert bool((_bits(cl[lo:hi]) == POISON).all()), "source %d was copied again" % k
            cl[lo:hi] = keep[lo:hi]
    assert r.src._cl is cl and r.src._cl_gen == gen and r.src.stale_mask() == 0
    assert torch.equal(_bits(cl), _bits(fresh.src._cl))
    _assert_same(r.render(**rays), want)
    assert torch.equal(_bits(cl), _bits(fresh.src._cl))


def test_unchanged_sources_and_confidence_launch_no_repack():
    """Nothing written: the whole buffer can be poisoned and is not touched.  The confidence map is read where it is: a write to it is seen by
    the next render with no copy to refresh."""
    scene, flat, rays = _clone(_scene(3)), _flat(3), _rays()
    r = _renderer(scene, flat)
    r.render(**rays)
    with torch.no_grad():
        scene["confidence"].mul_(0.5)
    keep = r.src._cl.clone()
    _bits(r.src._cl)[:] = POISON
    r.render(**rays)
    assert bool((_bits(r.src._cl) == POISON).all())
    r.src._cl.copy_(keep)
    _assert_same(r.render(**rays), _renderer(_clone(scene), flat).render(**rays))


def test_small_pass_follows_the_shared_copies():
    """fused_min_rounds puts small passes on a second RenderPass bound to the same sources: it reads the copies the first one keeps current."""
    scene, flat, rays = _clone(_scene(3)), _flat(3), _rays()
    r = _renderer(scene, flat, fused_min_rounds=4)
    assert r.pass_small is not None
    r.render(**rays)
    _write(scene, (0, 3))
    _assert_same(r.render(**rays), _renderer(_clone(scene), flat, fused_min_rounds=4).render(**rays))


# ------------------------------------------------------------------------------------------------ 3: reallocation
def test_no_stale_copy_across_reallocation():
    """Copies taken over from sources of another size (GatherSources.adopt_copies, what the drop-in's session does for unchanged tensors): the
    buffer does not fit, is allocated again, and EVERY source is rebuilt -- although every tensor here has the version count the old copies
    were recorded with (0: freshly made tensors), which a cache keyed on versions alone would take for "unchanged"."""
    flat, rays = _flat(3), _rays()
    a = _renderer(_clone(_scene(3)), flat)
    a.render(**rays)
    from uc_nerf_amd.synthetic import make_scene, scene_to
    big = scene_to(make_scene(seed=5, H=H, W=48, V=3, small_volumes=True), torch.device(DEV))
    b = _renderer(_clone(big), flat)
    assert [t._version for t in b.src._cl_tensors()] == a.src._cl_versions
    b.src.adopt_copies(a.src)
    old_cl, gen = a.src._cl, a.src._cl_gen
    assert b.src.stale_mask() == 0                                # (what the versions alone say)
    got = b.render(**rays)
    assert b.src._cl is not old_cl and b.src._cl.numel() != old_cl.numel() and b.src._cl_gen == gen + 1
    fresh = _renderer(_clone(big), flat)
    _assert_same(got, fresh.render(**rays))
    assert torch.equal(_bits(b.src._cl), _bits(fresh.src._cl))
    # and a second RenderPass that took its pointers from the old buffer takes them again
    c = _renderer(_clone(big), flat, fused_min_rounds=4)
    c.render(**rays)
    c.src._cl, c.src.cl_all = None, None                          # (the buffer is dropped under both passes)
    _assert_same(c.render(**rays), _renderer(_clone(big), flat, fused_min_rounds=4).render(**rays))
    lo = c.src._cl.data_ptr()
    for rp in (c.pass_, c.pass_small):                            # both passes are bound to the new buffer: every repacked source, inside it
        for k in range(5):
            bound, want = ((x.vol[k] if k < 3 else x.img_feat if k == 3 else x.imgs) for x in (rp.p.cl, c.src.cl_all))
            assert c.src.inplace[k] or (lo <= bound < lo + 4 * c.src._cl.numel() and bound == want), k


def _ops_pass(scene, flat):
    """(GatherSources of the scene's tensors, a way to bind an f32 ops.RenderPass to sources)"""
    from uc_nerf_amd import ops

    def sources(sc):
        return ops.GatherSources(sc["vols"], sc["confidence"], sc["imgs"], sc["img_feat"], sc["w2cs"][1:], sc["intrinsics"][1:])

    def bind(src):
        pw = ops.PackedWeights.get(src.V, 0, torch.device(DEV), "f32")
        return ops.RenderPass(src, pw, pw.pack(flat), scene["c2w"][:3, 3], scene["w2cs"][0], scene["intrinsics"][0], scene["w2cs"][0],
                              scene["near"], scene["far"])
    return sources, bind


def test_second_pass_follows_a_reallocation_without_being_told():
    """Two ops.RenderPass objects on one GatherSources, no renderer around them.  The buffer of copies is dropped and pass `a` builds it again
    (from sources written in the meantime); pass `b`, called with no repack call of any kind, reads the new buffer: its outputs are those of a
    pass on fresh sources of the changed tensors, bit for bit.  (A pass that kept the pointers it was given once would render the old values.)
    Ends the process, with every thread's stack, should it take longer than 120 s."""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        scene, flat, rays = _clone(_scene(3)), _flat(3), _rays()
        sources, bind = _ops_pass(scene, flat)
        rays_d, _, z = _renderer(scene, flat, precision="f32").sampler(rays["xs"], rays["ys"], rays["perturb"], rays["noise"])
        src = sources(scene)
        a, b = bind(src), bind(src)
        a.repack_sources()
        b.repack_sources(force=False)
        before = a(rays_d, z)
        _assert_same(b(rays_d, z), before)
        _write(scene, (0, 3))
        dropped = src._cl                                         # (kept alive here: the new buffer is another allocation, the old one stays valid memory)
        src._cl, src.cl_all = None, None
        a.repack_sources("changed")
        assert src._cl.data_ptr() != dropped.data_ptr()
        got = b(rays_d, z)
        fresh = bind(sources(_clone(scene)))
        fresh.repack_sources()
        _assert_same(got, fresh(rays_d, z))
        assert not torch.equal(got["rgb"], before["rgb"])         # (the write shows in the render: the old copies would not have passed)
    finally:
        faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ 4: .data
def test_force_rebuilds_after_a_data_write():
    """A write through `.data` does not bump the version counter (documented as unseen by the up-to-date mode): repack="force" rebuilds."""
    scene, flat, rays = _clone(_scene(3)), _flat(3), _rays()
    r = _renderer(scene, flat)
    r.render(**rays)
    scene["vols"][1].data.mul_(2)
    scene["imgs"].data.mul_(0.5)
    assert r.src.stale_mask() == 0
    _assert_same(r.render(repack="force", **rays), _renderer(_clone(scene), flat).render(**rays))


# ------------------------------------------------------------------------------------------------ 5: capture
def test_captured_step_records_the_full_repack():
    """capture() -> sources written in place -> replay: the graph holds the repack of every source (a replay cannot consult the host's
    versions), so the replay equals an eager render on the changed sources."""
    scene, flat, rays = _clone(_scene(3)), _flat(3), _rays()
    r = _renderer(scene, flat)
    g = r.capture(N_RAYS, perturb=1.0)
    _write(scene, (0, 2, 3, 4))
    out = g(rays["xs"], rays["ys"], rays["noise"])
    torch.cuda.synchronize()
    want = _renderer(_clone(scene), flat).render(**rays)
    for k in ("rgb", "depth", "acc", "weights", "z_fine", "z_samples"):
        assert torch.equal(out[k], want[k]), k
    _write(scene, (1,))
    _assert_same(r.render(**rays), _renderer(_clone(scene), flat).render(**rays))      # the eager route afterwards, same renderer


# ------------------------------------------------------------------------------------------------ 6: a short stateful sequence
def test_stateful_sequence_matches_fresh_renderers():
    """40 random steps of {render, source written in place, set_params, sources switched between channel-major and channel-last per source} on one
    renderer (the shape of tests/fuzz_pipeline.py); every render compared bit for bit with a renderer built for it."""
    from uc_nerf_amd.synthetic import random_pixels
    V = 3
    rng = np.random.RandomState(20)
    base = _scene(V, seed=7)
    flat = _flat(V, seed=7)
    cl = [False] * 5

    def laid_out(scene, cl_):
        v = [t.contiguous(memory_format=torch.channels_last_3d) if k else t.contiguous() for t, k in zip(scene["vols"], cl_[:3])]
        f = scene["img_feat"][:, 0].contiguous(memory_format=torch.channels_last).unsqueeze(1) if cl_[3] else scene["img_feat"].contiguous()
        i = scene["imgs"][0].contiguous(memory_format=torch.channels_last).unsqueeze(0) if cl_[4] else scene["imgs"].contiguous()
        return dict(scene, vols=v, img_feat=f, imgs=i)

    scene = laid_out(_clone(base), cl)
    r = _renderer(scene, flat)
    renders, log = 0, []
    for step in range(40):
        op = rng.choice(["render", "render", "render", "sources", "sources", "params", "layout"])
        if op == "render":
            xs, ys = random_pixels(N_RAYS, H, W, seed=step)
            g = torch.Generator().manual_seed(step)
            perturb = float(rng.choice([0.0, 1.0]))
            kw = dict(xs=xs.to(DEV), ys=ys.to(DEV), perturb=perturb, noise=torch.rand(N_RAYS, NC, generator=g).to(DEV) if perturb else None,
                      reuse_coarse=[None, True, False][int(rng.randint(0, 3))])
            got = r.render(**kw)
            want = _renderer(laid_out(_clone(scene), cl), flat.clone()).render(**kw)
            renders += 1
            log.append("render")
            _assert_same(got, want, "step %d after %s: " % (step, log[-8:]))
        elif op == "sources":
            k = int(rng.randint(0, 6))
            with torch.no_grad():
                (_source(scene, k) if k < 5 else scene["confidence"]).mul_(0.9)
            log.append("write %d" % k)
        elif op == "params":
            flat = flat * (1.0 + 0.02 * float(rng.randn()))
            r.set_params(flat)
            log.append("params")
        else:
            cl = [bool(rng.rand() < 0.5) for _ in range(5)]
            scene = laid_out(_clone(scene), cl)
            r = _renderer(scene, flat)                        # (new source tensors: a new renderer, as a script would build)
            log.append("layout %s" % "".join(str(int(x)) for x in cl))
    assert renders >= 10
