"""The 64 coarse + 128 fine hierarchical renderer composed from the library's entry points
(ray_marcher -> render -> sample_pdf on mid-points with w[1:-1] -> sorted merge -> render).

Library calls per batch (+ the source repack for the sources that changed since their channel-last copies were made), all on the caller's stream:
  ray_gen_sample (rays + coarse depths) -> render_fused_fwd (coarse; its compositing launch also runs sample_pdf + merge) -> render_fused_fwd (the
  network on the n_fine NEW depths, evaluation only) -> composite_merged_fwd (compositing over the new rows and the coarse pass's kept rows, read
  in merged order: no merged array).
  Five kernel launches per step on the gather-fused route (rays, MLP, composite + re-sample, MLP, composite); `fold_rays` moves the first into the
  coarse MLP launch (four launches; measured slower, off by default).  With reuse_coarse=False the fine pass is one render_fused_fwd over all
  n_coarse + n_fine depths instead (what the reference computes; the renders are bit-identical): five launches as well.

Training: render_train() is the same composition from the differentiable ops (feat_gather, mlp, composite, composite_merged), exact f32.
"""
import torch

from . import _lib as L
from . import ops


def flat_params_of(state_dict):
    """Concatenates a reference-style UCNeRF state_dict (state_dict order) into the flat vector the packer reads."""
    return torch.cat([v.reshape(-1) for v in state_dict.values()]).float()


class CoarseFineRenderer:
    """scene: dict with K[3,3], c2w[4,4] (target camera), w2cs[V,4,4] + intrinsics[V,3,3] (index 0 = reference
    view, 1.. = source views), near, far, vols (3 x [1,8,D,h,w]), imgs [1,V-1,3,H,W], img_feat [V-1,1,8,H,W],
    confidence [H,W]; tensors already on the device.  flat_params: the MLP's flat parameter vector (device)."""

    def __init__(self, scene, flat_params, n_coarse=64, n_fine=128, white_bkgd=False, pe_layout=0, max_blocks=0,
                 precision="f32", fused_min_rounds=0, sources_bf16=False):
        dev = scene["confidence"].device
        self.scene, self.dev = scene, dev
        self.n_coarse, self.n_fine, self.white_bkgd, self.max_blocks = n_coarse, n_fine, white_bkgd, max_blocks
        self.src = ops.GatherSources(scene["vols"], scene["confidence"], scene["imgs"], scene["img_feat"],
                                     scene["w2cs"][1:], scene["intrinsics"][1:], cl_bf16=sources_bf16)
        self.precision = precision          # "f32": exact fp32 MFMA; "bf16x3": split-bf16 matrix cores (inference, within the
                                            # parity bar); "bf16": plain bf16 operands (inference, ~3e-3 render error);
                                            # "bf16x3_fused": bf16x3 with the feature gather inside the MLP kernel (one launch per pass)
        self.pw = ops.PackedWeights.get(self.src.V, pe_layout, dev, precision)
        self.wstream = self.pw.pack(flat_params)
        w2c_ref = scene["w2cs"][0]
        self.pass_ = ops.RenderPass(self.src, self.pw, self.wstream, scene["c2w"][:3, 3].to(dev), w2c_ref,
                                    scene["intrinsics"][0], w2c_ref, scene["near"], scene["far"], white_bkgd, max_blocks)
        # fused_min_rounds > 0: passes with fewer tiles per wave than that take the two-kernel route (a second stream of the same
        # parameters).  Measured (scripts/ab_rounds.sh, 512 .. 2048 rays x 64 + 128): the fused kernel wins or ties at every size,
        # so the default is 0 -- always fused; the option stays for devices / shapes where a launch-bound shard might prefer otherwise.
        self.pass_small, self.fused_min_samples = None, 0
        if precision == "bf16x3_fused" and fused_min_rounds > 0:
            cus = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else 256
            self.fused_min_samples = int(fused_min_rounds) * cus * 8 * 32
            self.pw_small = ops.PackedWeights.get(self.src.V, pe_layout, dev, "bf16x3")
            self.wstream_small = self.pw_small.pack(flat_params)
            self.pass_small = ops.RenderPass(self.src, self.pw_small, self.wstream_small, scene["c2w"][:3, 3].to(dev), w2c_ref,
                                             scene["intrinsics"][0], w2c_ref, scene["near"], scene["far"], white_bkgd, max_blocks)
        self.u_det = torch.linspace(0., 1., n_fine, device=dev)
        # camera matrices and depth range travel BY VALUE in the ABI structs: keep host copies so that a render call
        # never reads device memory back (a read-back would drain the stream once per batch)
        self.K_host, self.c2w_host = scene["K"].detach().cpu(), scene["c2w"].detach().cpu()
        self.w2c_dir_host = w2c_ref.detach().cpu()
        self.near_host, self.far_host = float(scene["near"]), float(scene["far"])
        self.sampler = ops.RaySampler(self.K_host, self.c2w_host, n_coarse, self.near_host, self.far_host, self.w2c_dir_host)
        # round 4: the small launches around the coarse pass are folded into it -- ray_gen_sample into the gather-fused kernel's prologue, the coarse
        # compositing + sample_pdf + merge into one launch (a 512-ray shard's step is five launches instead of seven); False restores the old structure
        self.fold_launches = True     # coarse compositing + sample_pdf + merge: one launch (-2.5 us per step at 512 and at 4096 rays, same box)
        # ray_gen_sample inside the gather-fused coarse launch (ABI v4 gen_rays / gen_depths).  Per tile (the RAYGEN instantiation) it is bit-identical
        # and measured SLOWER than the 4.8-us launch it removes -- +1.2 us per step at 512 rays, +8 us at 4096 (profiles/r04_experiments.md: five
        # correctly rounded divisions and a square root per lane and tile, twice, are ~200 vector instructions in a kernel where none is free).  On the
        # tail route of small passes a block owns whole rays and makes them once, in its prologue: free.  None = that case only.
        self.fold_rays = None
        # what the last render() did in the fine pass: "new_depths" (network on the n_fine new depths, coarse rows reused) or "all_depths", and why
        self.fine_route, self.fine_route_reason = None, None

    def set_params(self, flat_params):
        self.wstream.copy_(self.pw.pack(flat_params))
        if self.pass_small is not None:
            self.wstream_small.copy_(self.pw_small.pack(flat_params))

    def _pass_for(self, n_samples):
        """The render pass serving a pass of `n_samples` samples (see fused_min_samples)."""
        if self.pass_small is not None and n_samples < self.fused_min_samples:
            if self.pass_.use_cl and not self.pass_small.use_cl:
                self.pass_small.repack_sources(force=False)      # (the channel-last copies belong to the shared sources object)
            return self.pass_small
        return self.pass_

    def _reuse_by_default(self, n):
        """(reuse?, reason) for reuse_coarse=None: the fine pass takes the coarse depths' rows from the coarse pass unless they would not be the
        bits a full evaluation gives, or the library says the reuse does not pay at this size (ucnerf_reuse_coarse_pays)."""
        nc, nf = self.n_coarse, self.n_fine
        if self.pw.guarded or (self.pass_small is not None and self.pw_small.guarded):
            # "fp16_guarded": a fine launch that saturates replays itself on bf16 terms while the kept coarse rows came from fp16 terms -- the
            # merged rows would mix the two and not equal the all-depths replay
            return False, "fp16_guarded operand mode"
        if len({id(self._pass_for(n * k)) for k in (nc, nf, nc + nf)}) != 1:
            # fused_min_rounds puts the passes on different kernels: their rows are not bit-identical to each other
            return False, "fused_min_rounds: the passes run on different kernels"
        fpass = self._pass_for(n * (nc + nf))
        if (fpass.pw.cfg.precision == 3 and fpass.use_cl and not self.src.cl_bf16 and not self.max_blocks
                and not L.lib().ucnerf_reuse_coarse_pays(n, nc, nf)):
            # the pass over all depths composites inside its MLP launch: one launch; the reuse would put a compositing launch back
            return False, "tail route: the all-depths pass is one launch"
        return True, "default"

    def render(self, xs, ys, perturb=0.0, noise=None, u=None, events=None, repack=True, reuse_coarse=None):
        """xs, ys: pixel coordinates [n] (device, float32).  events: optional [(start, stop), (start, stop)]
        Event pairs recorded around the coarse and the fine MLP launches.
        repack: what happens to the channel-last copies of the sources before the step.  True (default): they are brought up to date -- a source
        (each volume, the image features, the images: on its own) whose tensor was written since its copy was made is copied again, in one launch
        for all of them; a step on unchanged sources launches nothing (RenderPass.repack_sources(force="changed")).  "Written" is what the tensor's
        version counter says: in-place ops, copy_, optimizer steps are seen; a write through `.data`, or by another library through the raw
        pointer, is NOT -- pass repack="force" (all copies rebuilt, unconditionally) after those.  False: the copies are used as they are.
        While a graph is being captured (capture()) True records the full repack: a replay cannot ask the host what changed.
        reuse_coarse: the fine pass evaluates the network on the n_fine NEW depths only and takes the n_coarse coarse
        depths' outputs from the coarse pass (a sample's output depends on nothing but that sample, so the merged
        rows -- and everything composited from them -- are bit-identical to re-evaluating all n_coarse + n_fine, which is
        what the reference does): one third less network and gather work in the fine pass.  None (default): the renderer
        decides -- reuse, except where the rows would not be the full evaluation's bits or the all-depths pass is small enough to
        composite inside its own MLP launch (_reuse_by_default); the returned
        dict is that of reuse_coarse=False, name for name.  True / False force the choice; True also returns the working
        buffers (coarse["raw"], the merge rank, "disp").  self.fine_route names what was done."""
        sc = self.scene
        if repack:
            self.pass_.repack_sources(force=True if repack == "force" else "changed")
        # rays and their view-direction feature from one launch; both passes take the feature as an input
        n = int(xs.shape[0])
        explicit = reuse_coarse is not None
        if explicit:
            reuse_coarse, why = bool(reuse_coarse), "forced"
        else:
            reuse_coarse, why = self._reuse_by_default(n)
        self.fine_route, self.fine_route_reason = ("new_depths" if reuse_coarse else "all_depths"), why
        cpass = self._pass_for(n * self.n_coarse)
        # fold_rays (gather-fused kernel, up to six source views): the coarse launch generates rays, coarse depths and direction features itself
        # (ABI v4 gen_rays / gen_depths) -- no ray_gen_sample launch
        fold_rays = self.fold_rays
        if fold_rays is None:
            fold_rays = (cpass.pw.cfg.precision == 3 and cpass.use_cl and not self.src.cl_bf16 and not self.max_blocks
                         and bool(L.lib().ucnerf_fused_tail_fits_resample(n, self.n_coarse, self.n_fine) if self.fold_launches
                                  else L.lib().ucnerf_fused_tail_fits(n, self.n_coarse)))
        gen = self.sampler if (fold_rays and cpass.pw.cfg.precision == 3 and cpass.use_cl and self.src.V <= 6) else None
        rays_d, angle, z_c = self.sampler.prepare(xs, ys, perturb, noise) if gen is not None else self.sampler(xs, ys, perturb, noise)
        ev = [(a.h, b.h) for a, b in events] if events else (None, None)
        # the coarse pass's compositing launch draws the fine depths as well (composite + sample_pdf + sorted merge: one launch, ABI v4)
        if self.fold_launches:
            coarse = cpass(rays_d, z_c, want=("weights",), events=ev[0], keep=("raw",) if reuse_coarse else (), dir_feat=angle, gen=gen,
                           resample={"u": self.u_det if u is None else u, "want_rank": reuse_coarse})
            hs = coarse
        else:                                                   # (the launch structure of rounds 1-3, kept for A/B and the bit-identity tests)
            coarse = cpass(rays_d, z_c, want=("weights",), events=ev[0], keep=("raw",) if reuse_coarse else (), dir_feat=angle, gen=gen)
            hs = ops.sample_pdf(None, coarse["weights"], self.u_det if u is None else u, z_merge=z_c, want_inds=False,
                                from_coarse=True, want_rank=reuse_coarse)
        if reuse_coarse:
            new = self._pass_for(n * self.n_fine)(rays_d, hs["samples"], want=None, events=ev[1], dir_feat=angle)      # (evaluation only: no compositing of its own)
            out = ops.composite_merged_fwd(new["raw"], coarse["raw"], hs["merge_rank"], hs["z_sorted"], self.white_bkgd)      # cat(samples, z_coarse) order
            if not explicit:                                    # the working buffers stay inside: the names of the all-depths route
                del out["disp"], coarse["raw"], hs["merge_rank"]
        else:
            out = self._pass_for(n * (self.n_coarse + self.n_fine))(rays_d, hs["z_sorted"], want=("acc", "weights", "var"), events=ev[1], dir_feat=angle)
        out.update(z_coarse=z_c, z_fine=hs["z_sorted"], z_samples=hs["samples"], coarse=coarse, rays_d=rays_d)
        return out

    # ------------------------------------------------------------------------------------------------ training
    def _train_coords(self, rays_d, z):
        """(pts [n,S,3], dict stage1, stage2, stage3, ndc) at the depths z: world points o + z d in the order of the render pass's own kernel, and
        their stage coordinates as RenderPass derives them (scene near / far for every stage).  No gradient: positions are not differentiable here."""
        if not hasattr(self, "_K_ref_host"):
            self._K_ref_host = self.scene["intrinsics"][0].detach().cpu()
        pts = (self.pass_.rays_o.view(1, 1, 3) + z.unsqueeze(-1) * rays_d.unsqueeze(1)).contiguous()
        nf = dict.fromkeys(("near_1", "near_2", "near_3"), self.near_host)
        nf.update(dict.fromkeys(("far_1", "far_2", "far_3"), self.far_host), near=self.near_host, far=self.far_host)
        return pts, ops.ndc_project(pts, self.w2c_dir_host, self._K_ref_host, [self.src.W - 1, self.src.H - 1], nf)

    def _eval_train(self, flat_params, wstream, rays_d, angle, z):
        """raw [n,S,4] at the depths z with autograd history: ops.feat_gather on the scene's own tensors, ops.mlp on `flat_params`."""
        sc = self.scene
        n, S = z.shape
        if not hasattr(self, "_w2cs_src"):
            self._w2cs_src, self._intr_src = sc["w2cs"][1:].detach().contiguous(), sc["intrinsics"][1:].detach().contiguous()
        pts, ndc = self._train_coords(rays_d, z)
        feats = ops.feat_gather(sc["vols"], sc["confidence"], sc["img_feat"], sc["imgs"], self._w2cs_src, self._intr_src, pts,
                                ndc["stage1"], ndc["stage2"], ndc["stage3"])
        return ops.mlp(flat_params, feats, ndc["ndc"], angle, self.pw, S, wstream).view(n, S, 4)

    def render_train(self, xs, ys, flat_params, perturb=0.0, noise=None, u=None, maps=False):
        """render(reuse_coarse=True) with autograd history: the same dict, name for name (rgb, depth, acc, disp, weights, var, coarse{rgb, depth,
        weights, raw, samples, z_sorted, merge_rank}, z_coarse, z_fine, z_samples, rays_d; disp and var carry no gradient), differentiable back to `flat_params` and to whichever of the scene's volumes, image features and confidence
        have requires_grad.  xs, ys, perturb, noise, u: as in render().
        Route: sampler -> gather + MLP at the coarse depths (ops.feat_gather, ops.mlp) -> ops.composite; its weights, detached, draw the new
        depths (ops.sample_pdf: no gradient, as in the reference) -> gather + MLP at the NEW depths only -> ops.composite_merged over the new rows
        and the coarse rows.  The coarse rows receive gradient twice -- from the coarse compositing and, as raw_b, from the fine one -- and
        autograd sums the two.  The network runs on a stream packed from `flat_params` here (the renderer's own stream is not touched).
        maps=True: both compositing steps go through ops.composite_maps / ops.composite_merged_maps instead -- the same forward launches, the
        same values -- so that `disp` and `var` (and coarse["disp"], coarse["var"], returned in addition) carry gradient: a loss on the
        weights' variance or on disparity trains the network (one extra launch per compositing step in the backward, and only when such a
        gradient arrives).  The composited uncertainty wu is not among them: the training forward gathers features, not the per-sample u,
        as a tensor; ops.composite_maps(raw, z, u=...) takes a loss on it at the ops level.
        Exact-f32 precision only."""
        if self.pw.guarded:
            raise RuntimeError("uc_nerf_amd.CoarseFineRenderer.render_train: the 'fp16_guarded' operand mode is an inference mode -- a launch that "
                               "saturates replays itself on other terms, which no backward follows; train with precision='f32'")
        if self.precision != "f32":
            raise RuntimeError("uc_nerf_amd.CoarseFineRenderer.render_train: precision %r has no training forward in the ops layer (ops.mlp's "
                               "backward re-runs the network in exact f32); train with precision='f32'" % self.precision)
        rays_d, angle, z_c = self.sampler(xs, ys, perturb, noise)
        wstream = self.pw.pack(flat_params.detach())
        raw_c = self._eval_train(flat_params, wstream, rays_d, angle, z_c)
        if maps:
            rgb_c, depth_c, acc_c, w_c, disp_c, var_c = ops.composite_maps(raw_c, z_c, self.white_bkgd)
        else:
            rgb_c, depth_c, acc_c, w_c, _, _ = ops.composite(raw_c, z_c, self.white_bkgd)
        hs = ops.sample_pdf(None, w_c.detach(), self.u_det if u is None else u, z_merge=z_c, want_inds=False, from_coarse=True, want_rank=True)
        raw_f = self._eval_train(flat_params, wstream, rays_d, angle, hs["samples"])
        fine = ops.composite_merged_maps if maps else ops.composite_merged
        rgb, depth, acc, weights, disp, var = fine(raw_f, raw_c, hs["merge_rank"], hs["z_sorted"], self.white_bkgd)      # cat(samples, z_coarse) order
        coarse = dict(rgb=rgb_c, depth=depth_c, weights=w_c, raw=raw_c, samples=hs["samples"], z_sorted=hs["z_sorted"], merge_rank=hs["merge_rank"])
        if maps:
            coarse.update(disp=disp_c, var=var_c)
        return dict(rgb=rgb, depth=depth, acc=acc, disp=disp, weights=weights, var=var, z_coarse=z_c, z_fine=hs["z_sorted"], z_samples=hs["samples"],
                    coarse=coarse, rays_d=rays_d)

    # ------------------------------------------------------------------------------------------------ HIP graph
    def capture(self, n_rays, perturb=0.0, repack=True, reuse_coarse=None):
        """Captures one render of `n_rays` rays into a HIP graph (the launch-bound regime of small
        per-GPU batches).  Returns a callable g(xs, ys, noise=None) -> the same dict as render(); its tensors are owned
        by the graph and overwritten by the next replay.  repack=True (or "force") records the repack of all the sources: every replay
        re-reads them.  Every launch of the step goes to the capturing stream and
        the step allocates only through torch's caching allocator, so the capture is a plain stream capture."""
        dev = self.dev
        xs_s, ys_s = torch.zeros(n_rays, device=dev), torch.zeros(n_rays, device=dev)
        noise_s = torch.rand(n_rays, self.n_coarse, device=dev) if perturb > 0 else None
        kw = dict(perturb=perturb, noise=noise_s, repack=repack, reuse_coarse=reuse_coarse)
        from .train_step import _CAPTURE_STREAMS          # one stream of the graph's own for warm-up and capture, never destroyed (train_step.GraphedStep)
        cap = torch.cuda.Stream(device=dev)
        _CAPTURE_STREAMS.append(cap)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap):                        # warm-up: one-time attribute calls, workspace allocation
            for _ in range(2):
                self.render(xs_s, ys_s, **kw)
        torch.cuda.current_stream(dev).wait_stream(cap)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            out = self.render(xs_s, ys_s, **kw)

        def replay(xs=None, ys=None, noise=None):
            """One hipGraphLaunch.  Arguments given are first copied into the graph's static inputs (one small launch each); a caller
            that wants none of those writes into `replay.inputs` itself and calls replay()."""
            if xs is not None:
                xs_s.copy_(xs, non_blocking=True)
            if ys is not None:
                ys_s.copy_(ys, non_blocking=True)
            if noise_s is not None and noise is not None:
                noise_s.copy_(noise, non_blocking=True)
            graph.replay()
            return out

        replay.graph = graph
        replay.inputs = {"xs": xs_s, "ys": ys_s, "noise": noise_s}
        return replay
