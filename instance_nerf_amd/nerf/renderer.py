"""``NeRFRenderer`` - the drop-in render API.

Keeps torch-ngp's public surface (``render``, ``run_cuda``, ``update_extra_state``,
``mark_untrained_grid``, ``reset_extra_state`` and the module buffers
``density_grid``/``density_bitfield``/``step_counter``/``mean_count``/...) so the
reference's instance-field trainer and grid extractor call it unchanged
(upstream ``nerf/renderer.py`` of the un-vendored submodule,
/root/reference/.gitmodules:4-6, README.md:27,59).  ``cuda_ray=True`` is the
hot path (``run_cuda``, all HIP); upstream's default sampler without an occupancy
grid (``run``: uniform + importance samples) is kept as tensor-op glue around the
HIP ray/box test and field kernels.

MI355X-first differences (results identical up to fp32 rounding):
* inference renders a whole ray batch in four launches - count/scan, write,
  fused field, composite - with no host round trip per marching step
  (``infer_mode='fused'``); upstream's alive-ray loop is kept as
  ``infer_mode='wavefront'`` for API-level parity tests;
* sample slots are deterministic (scan in ray order).
"""
import math
import os

import torch
import torch.nn as nn

from .. import _lib, raymarching
from .._lib import check, ptr, stream_ptr


def sample_pdf(bins, weights, n_samples, det=False):
    """Inverse-CDF sampling of ``n_samples`` depths per ray from the piecewise-constant density ``weights`` over
    ``bins`` (NeRF's hierarchical sampling, as upstream ``nerf/renderer.py::sample_pdf``).  bins [N, T+1],
    weights [N, T] -> [N, n_samples]."""
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    if det:
        u = torch.linspace(0.5 / n_samples, 1 - 0.5 / n_samples, steps=n_samples, device=weights.device)
        u = u.expand(list(cdf.shape[:-1]) + [n_samples])
    else:
        u = torch.rand(list(cdf.shape[:-1]) + [n_samples], device=weights.device)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    cdf_g = torch.stack([torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)], -1)
    bins_g = torch.stack([torch.gather(bins, 1, below), torch.gather(bins, 1, above)], -1)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


class MarchedHead:
    """The prefetched head of a training render (``NeRFRenderer.march_ahead``): the ray/box test and the march of one
    batch - and, with ``shade``, its frozen field and compositing forward - queued ahead of the render that consumes
    them.  Every rule about whether it is still that render's head lives here."""
    __slots__ = ("rays_o", "rays_d", "skip_labels", "n_rays", "grid_state", "nears", "fars", "xyzs", "dirs", "deltas",
                 "rays", "counter", "shaded", "T_thresh", "density_scale", "slot_taken", "slot_index", "done", "side")

    def __init__(self, rays_o, rays_d, skip_labels, n_rays, grid_state, nears=None, fars=None, xyzs=None, dirs=None,
                 deltas=None, rays=None, counter=None, shaded=None, T_thresh=1e-4, density_scale=1.0, slot_taken=False,
                 slot_index=-1, done=None, side=None):
        self.rays_o, self.rays_d = rays_o, rays_d        # the caller's tensors, as handed to march_ahead
        self.skip_labels = skip_labels                   # the label tensor the march was pruned with, or None
        self.n_rays, self.grid_state = n_rays, grid_state        # ray count; iter_density of the grid marched through
        self.nears, self.fars = nears, fars
        self.xyzs, self.dirs, self.deltas, self.rays, self.counter = xyzs, dirs, deltas, rays, counter
        # (weights_sum, depth, image, weights, sample_ray) of march_ahead(shade=True), for this T_thresh / density_scale
        self.shaded, self.T_thresh, self.density_scale = shaded, float(T_thresh), float(density_scale)
        self.slot_taken, self.slot_index = slot_taken, slot_index        # the renderer's step_counter slot (drop_ahead)
        self.done, self.side = done, side                # event recorded behind the head on the stream it was queued on

    def marched_for(self, rays_o, rays_d, skip_labels):
        """Marched for THESE tensors (identity, not addresses: a freshly allocated batch may reuse the address of a freed
        one - round-3 advisor) and, in the instance stage, pruned with THESE labels (round-5 advisor: a march that left
        out the rays another mask tensor ignores would silently drop labelled rays of this batch)."""
        return self.rays_o is rays_o and self.rays_d is rays_d and self.skip_labels is skip_labels

    def fits(self, training, n_rays, grid_state):
        """A training render of as many rays, through the occupancy grid the head was marched through."""
        return bool(training) and self.n_rays == n_rays and self.grid_state == grid_state

    def shaded_for(self, T_thresh, density_scale):
        """The pre-shaded outputs, if they were computed with this threshold and density scale; None otherwise."""
        if self.T_thresh == float(T_thresh) and self.density_scale == float(density_scale):
            return self.shaded
        return None

    def wait(self):
        """The current stream waits for the head (nothing to do on the stream it was queued on)."""
        if self.done is None:
            return
        cur = torch.cuda.current_stream()
        if self.side is not cur:
            cur.wait_event(self.done)

    def ordered_here(self, grid_state):
        """The same buffers, already ordered on the consuming stream (nothing to wait for) and valid for the grid
        generation given.  The slot flags stay with the original, which is the one a caller may drop."""
        return MarchedHead(self.rays_o, self.rays_d, self.skip_labels, self.n_rays, grid_state, self.nears, self.fars,
                           self.xyzs, self.dirs, self.deltas, self.rays, self.counter, self.shaded, self.T_thresh,
                           self.density_scale)


class _NoGate:
    """``field_gate`` of a render that shares the device with no other view: nothing to order."""

    def acquire(self):
        pass

    def release(self):
        pass


_NO_GATE = _NoGate()


class NeRFRenderer(nn.Module):
    min_staged_batch = 1 << 20

    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01,
                 bg_radius=-1, grid_size=128):
        super().__init__()
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.grid_size = grid_size
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        # > 0: the subclass's background sphere model (``background_rays`` / ``blend_background``) REPLACES whatever
        # ``bg_color`` a render call is given, in training and in inference - upstream's behaviour, also for the random
        # background of an RGBA batch.
        self.bg_radius = bg_radius
        aabb = torch.tensor([-bound, -bound, -bound, bound, bound, bound], dtype=torch.float32)
        self.register_buffer("aabb_train", aabb)
        self.register_buffer("aabb_infer", aabb.clone())
        self.cuda_ray = cuda_ray
        if cuda_ray:
            self.register_buffer("density_grid", torch.zeros(self.cascade, grid_size ** 3))
            self.register_buffer("density_bitfield", torch.zeros(self.cascade * grid_size ** 3 // 8, dtype=torch.uint8))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0
            self.last_counter = None     # (total samples, N) int32 view of the march the last training render consumed

    # ``mean_density`` (upstream: a float set by every occupancy update) is a host float that the update leaves on the
    # device until somebody asks: the bit field's threshold min(mean, density_thresh) is formed on the device, so the
    # training loop never needs the number and the update ends without waiting for its own kernels.
    @property
    def mean_density(self):
        pending = self.__dict__.get("_mean_density_dev")
        if pending is not None:
            self.__dict__["_mean_density"] = float(pending[0].item())
            self.__dict__["_mean_density_dev"] = None
        return self.__dict__.get("_mean_density", 0)

    @mean_density.setter
    def mean_density(self, value):
        self.__dict__["_mean_density_dev"] = None
        self.__dict__["_mean_density"] = value

    # subclass API ---------------------------------------------------------------------------
    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def density_sigma(self, x):
        """sigma only (the occupancy update needs nothing else); subclasses may skip the geo features."""
        return self.density(x)["sigma"]

    def instance(self, x):
        return None

    # bg_radius > 0: the subclass's background model
    def background_rays(self, rays_o, rays_d):
        """rays [N,3] -> rgb [N,3] (an autograd tensor while the model trains)."""
        raise NotImplementedError()

    def blend_background(self, rays_o, rays_d, weights_sum, image):
        """No-grad: ``image += (1 - weights_sum) * background`` in place; -> the background [N,3]."""
        bg = self.background_rays(rays_o, rays_d).detach()
        image.add_((1 - weights_sum).unsqueeze(-1) * bg)
        return bg

    def _bg_params(self):
        return []

    # optional: what the render paths ask a subclass before they take its fused kernels (``NeRFNetwork`` sets them)
    num_instances = 0          # channels of the instance head; 0: none
    _fusable = False           # the NeRF field has the fused kernels (forward_table, sh_table, nerf_render, _fused_nerf,
    #                            _nerf_params, last_frame_path)
    _fusable_inst = False      # ... and so has the instance field (instance_render, instance_head_train)

    def instance_head_available(self, x):
        """Field + K-channel compositing of the samples ``x`` as one autograd node (``instance_head_train``)."""
        return False

    def reset_extra_state(self):
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    # ----------------------------------------------------------------------------------------
    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """The sampler upstream uses when the network is built WITHOUT ``cuda_ray`` (its default): ``num_steps``
        uniform depths between the ray's entry and exit of the box, ``upsample_steps`` more drawn from the coarse
        weights (inverse-CDF sampling, as in NeRF), every sample evaluated by ``density`` / ``color`` (the HIP field
        kernels), colours only where the weight exceeds 1e-4.  No occupancy grid is involved.  Tensor-op glue around
        the HIP ray/box test and field kernels - this is upstream's slow path, kept for callers that never enabled
        ``cuda_ray``; the hot path is ``run_cuda``.  rays_o, rays_d [B,N,3] -> dict(image, depth, weights_sum
        (, instance))."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N, device = rays_o.shape[0], rays_o.device
        aabb = self.aabb_train if self.training else self.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        hit = (fars > nears) & (fars < 3.0e38)            # rays that miss the box keep near = far = FLT_MAX
        nears = torch.where(hit, nears, torch.zeros_like(nears)).unsqueeze(-1)
        fars = torch.where(hit, fars, torch.ones_like(fars)).unsqueeze(-1)

        z_vals = torch.linspace(0.0, 1.0, num_steps, device=device).unsqueeze(0)
        z_vals = nears + (fars - nears) * z_vals                                      # [N, T]
        sample_dist = (fars - nears) / num_steps
        if perturb:
            z_vals = z_vals + (torch.rand(z_vals.shape, device=device) - 0.5) * sample_dist

        def positions(z):
            x = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z.unsqueeze(-1)
            return torch.min(torch.max(x, aabb[:3]), aabb[3:])

        def weights_of(z, sigma):
            deltas = torch.cat([z[..., 1:] - z[..., :-1], sample_dist * torch.ones_like(z[..., :1])], dim=-1)
            alphas = 1 - torch.exp(-deltas * self.density_scale * sigma)
            shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], dim=-1)
            return alphas * torch.cumprod(shifted, dim=-1)[..., :-1], deltas

        xyzs = positions(z_vals)
        den = {k: v.view(N, num_steps, -1) for k, v in self.density(xyzs.reshape(-1, 3)).items()}
        if upsample_steps > 0:
            with torch.no_grad():
                weights, deltas = weights_of(z_vals, den["sigma"].squeeze(-1))
                z_mid = z_vals[..., :-1] + 0.5 * deltas[..., :-1]
                new_z = sample_pdf(z_mid, weights[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_xyzs = positions(new_z)
            new_den = {k: v.view(N, upsample_steps, -1) for k, v in self.density(new_xyzs.reshape(-1, 3)).items()}
            z_vals, order = torch.sort(torch.cat([z_vals, new_z], dim=1), dim=1)
            xyzs = torch.gather(torch.cat([xyzs, new_xyzs], dim=1), 1, order.unsqueeze(-1).expand(-1, -1, 3))
            den = {k: torch.gather(torch.cat([den[k], new_den[k]], dim=1), 1,
                                   order.unsqueeze(-1).expand(-1, -1, den[k].shape[-1])) for k in den}
        weights, _ = weights_of(z_vals, den["sigma"].squeeze(-1))
        weights = weights * hit.unsqueeze(-1)
        T = z_vals.shape[1]
        dirs = rays_d.unsqueeze(-2).expand(-1, T, -1)
        mask = (weights > 1e-4).reshape(-1)
        rgbs = self.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=mask,
                          geo_feat=den["geo_feat"].reshape(-1, den["geo_feat"].shape[-1])).view(N, T, 3)
        weights_sum = weights.sum(dim=-1)
        depth = torch.sum(weights * ((z_vals - nears) / (fars - nears)).clamp(0, 1), dim=-1)
        image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2)
        if self.bg_radius > 0:
            bg_color = self.background_rays(rays_o, rays_d)
        elif bg_color is None:
            bg_color = 1
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        results = {"image": image.view(*prefix, 3), "depth": depth.view(*prefix), "weights_sum": weights_sum.view(*prefix)}
        if self.num_instances > 0:
            logits = self.instance(xyzs.reshape(-1, 3)).view(N, T, -1)
            results["instance"] = torch.sum(weights.detach().unsqueeze(-1) * logits, dim=-2).view(*prefix, -1)
        return results

    def _instance_for_compositing(self, x):
        """Logits handed to the K-channel compositing kernels; a network may return more channels than
        ``num_instances`` (zero-padded MFMA tiles) - the renderer keeps the first ``num_instances`` rendered ones."""
        return self.instance(x)

    def run_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False,
                 max_steps=1024, T_thresh=1e-4, infer_mode="auto", noises=None, field_gate=None, ce_labels=None,
                 ce_ignore_index=-1, mse_target=None, marched=None, ce_prune=False, **kwargs):
        """rays_o, rays_d [B,N,3] -> dict(image [B,N,3], depth [B,N], weights_sum [B,N] (, instance [B,N,K])).

        infer_mode (eval only; all modes render the same image):
          "fused"            march -> fused field kernel -> compositing kernel (fastest when rays stay transparent)
          "fused_terminate"  march -> ONE kernel for field + compositing that stops a 16-ray group once all its rays
                             are opaque (measured 4x faster than "fused" on an opaque scene, 1.4x slower on a
                             transparent one)
          "auto" (default)   picks between the two from the fraction of samples the early-terminating kernel skips /
                             would skip, as counted by the previous inference calls (> terminate_above = 0.50)
          "fused_raymajor" / "wavefront"   reference paths kept for parity tests (ray-major layout / upstream's loop)

        ce_labels (training, networks with an instance head; int64, one per ray): the cross entropy of the rendered
        instance logits against them (``ce_ignore_index`` rows skipped) is returned as ``results["instance_ce"]`` when
        the one-node instance head applies (``instance_head_available``); otherwise the key is absent and the caller
        computes the loss from ``results["instance"]`` as usual.
        ce_prune (training, with ce_labels): rays labelled ``ce_ignore_index`` are not marched at all - they carry no
        loss and no gradient, so loss and gradients are unchanged; their image / depth / instance rows come back as
        those of a ray that misses the volume (background, zeros).  Trainer(stage="instance") asks for it; a caller
        that wants the rendered rows of ignored rays leaves it off.

        marched (training): the result of ``march_ahead`` for exactly these rays - the ray/box test and the march were
        queued earlier (on a side stream, under the previous step's backward) and are not repeated here.

        mse_target (training, [.., 3] per ray): the mean squared error of the shaded image against it is returned as
        ``results["image_mse"]`` when the fused tail applies (gradient flows through the image, uniform or per-ray
        background, <= 65536 rays): blend, depth normalisation, loss and its gradients are then one launch each way
        instead of ~18 element-wise launches; otherwise the key is absent and the caller forms the loss itself.

        field_gate (eval, one-pass modes): an object with ``acquire()`` / ``release()`` called on the current stream
        right before and after the field evaluation.  FramePipeline uses it to keep the field kernels of views that
        are rendered on different streams one after the other while everything else overlaps.
        """
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N = rays_o.shape[0]
        aabb = self.aabb_train if self.training else self.aabb_infer
        if marched is not None and not marched.fits(self.training, N, self.iter_density):
            self.drop_ahead(marched)         # other rays, or marched through an occupancy grid that has been updated since
            marched = None
        if marched is not None:
            marched.wait()
            nears, fars = marched.nears, marched.fars
        elif self.training and ce_prune and ce_labels is not None:
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near, skip_labels=ce_labels,
                                                         ignore_index=ce_ignore_index)
        else:
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        if not self.training and infer_mode == "auto":
            infer_mode = "fused_terminate" if self._recent_skippable() > self.terminate_above else "fused"
        gate = _NO_GATE if field_gate is None else field_gate
        jitter = noises if perturb else None
        # the samples are consumed by the fused kernels only (NeRF field, fused instance render)
        all_fused = self._fusable and (self._fusable_inst or self.num_instances == 0)
        results = {}
        if self.training or infer_mode == "fused_raymajor":
            weights_sum, depth, image = self._render_ray_major(
                results, prefix, rays_o, rays_d, nears, fars, marched, dt_gamma, max_steps, perturb, noises,
                force_all_rays, T_thresh, ce_labels, ce_ignore_index)
        elif infer_mode == "fused_terminate" and all_fused:
            weights_sum, depth, image = self._render_terminating(
                results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, jitter, T_thresh, gate)
        elif infer_mode in ("fused", "fused_terminate"):
            weights_sum, depth, image = self._render_two_kernel(
                results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, jitter, T_thresh, gate, all_fused)
        elif infer_mode == "wavefront":
            weights_sum, depth, image = self._render_wavefront(
                results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, perturb, T_thresh)
        else:
            raise ValueError(f"unknown infer_mode {infer_mode!r}")
        one_pass = not self.training and infer_mode != "wavefront"
        if self.bg_radius > 0:
            # The model's background replaces the caller's bg_color.  Where a gradient flows (to the background model,
            # or through the shaded image) it is a per-ray tensor and the blend is _finish_rays' tensor expression;
            # otherwise _finish_rays runs with a zero triplet and the background launch blends in place: two launches.
            bg_flows = torch.is_grad_enabled() and any(p.requires_grad for p in self._bg_params())
            if bg_flows or (torch.is_grad_enabled() and (image.requires_grad or weights_sum.requires_grad)):
                with torch.set_grad_enabled(bg_flows):
                    bg = self.background_rays(rays_o, rays_d)
                return self._finish_rays(results, prefix, weights_sum, depth, image, nears, fars, bg, mse_target,
                                         one_pass, jitter, dt_gamma, max_steps)
            results = self._finish_rays(results, prefix, weights_sum, depth, image, nears, fars, 0, mse_target, one_pass,
                                        jitter, dt_gamma, max_steps)
            self.blend_background(rays_o, rays_d, results["weights_sum"].detach().reshape(-1).contiguous().float(),
                                  results["image"].view(-1, 3))
            return results
        return self._finish_rays(results, prefix, weights_sum, depth, image, nears, fars,
                                 1 if bg_color is None else bg_color, mse_target, one_pass, jitter, dt_gamma, max_steps)

    def _take_counter_slot(self):
        """-> (index, row) of ``step_counter`` for the next training march - (total samples, N), written by its count
        pass; ``local_step`` advances."""
        index = self.local_step % 16
        self.local_step += 1
        return index, self.step_counter[index]

    def _composite_with_logits(self, composite, results, prefix, xyzs, *args, **kwargs):
        """K-channel compositing: ``composite(*args, extra=<logits of the samples>)`` -> weights_sum, depth, image; of the
        rendered channels (``_instance_for_compositing``) the first ``num_instances`` are kept."""
        with_instance = self.num_instances > 0
        extra = self._instance_for_compositing(xyzs) if with_instance else None
        out = composite(*args, extra=extra, **kwargs)
        if with_instance:
            results["instance"] = out[3][:, :self.num_instances].reshape(*prefix, -1)
        return out[0], out[1], out[2]

    def _render_terminating(self, results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, jitter, T_thresh, gate):
        """``fused_terminate``: ONE launch for field + compositing, with early termination per 16-ray group (opaque
        scenes)."""
        with_instance = self.num_instances > 0
        counter = torch.zeros(2, dtype=torch.int32, device=rays_o.device)
        # both consumers take the writer's normalised coordinates and look the direction up per ray: the table
        # feed (x01 + ray id, 24 instead of 32 bytes written per sample)
        xyzs, _, deltas, rays = raymarching.march_rays_patch(
            rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars,
            dt_gamma, max_steps, noises=jitter, counter=counter, table=True)
        gate.acquire()
        weights_sum, depth, image, wbuf, evaluated = self.nerf_render(xyzs, deltas, rays, rays_d, T_thresh,
                                                                      want_weights=with_instance, normalised=True)
        gate.release()
        if with_instance:
            gate.acquire()                   # a gather kernel too: never beside another view's field kernel
            results["instance"] = self.instance_render(xyzs, rays, wbuf, normalised=True).view(*prefix, -1)
            gate.release()
        results["num_samples"] = counter
        results["num_evaluated"] = evaluated
        self._note_skippable(evaluated, int(xyzs.shape[0]), True)        # raw counter, marched total (host), "evaluated"
        return weights_sum, depth, image

    def _render_two_kernel(self, results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, jitter, T_thresh, gate,
                           table):
        """``fused``: the full batch in four launches, patch-interleaved sample layout (csrc/raymarch.hip).  ``table``:
        the samples are consumed by the fused kernels only, so the writer emits normalised coordinates + ray ids and the
        field reads a per-ray direction table (forward_table).

        Feed of a ``table`` frame: (t, ray id) records - 8 bytes per sample between march, field and compositing, which
        rebuild position and (dt, t - t_prev) with the marcher's operations - when nothing else reads positions
        (``num_instances == 0``), 2*bound is a power of two and the field runs on the fused kernel, neither sliced nor
        probing (``plan_frame``, asked once the sample count is known, before the write pass); positions (x01 [M,3] +
        deltas [M,2]) otherwise and under ``frame_records = False``.  Same outputs bit for bit; ``results["frame_feed"]``."""
        device = rays_o.device
        fused_inst = self.num_instances > 0 and self._fusable_inst
        counter = torch.zeros(2, dtype=torch.int32, device=device)
        may_record = bool(table and self.num_instances == 0 and self.records_apply())
        # the direction table and the counter of the compositing kernel do not depend on the sample count: they
        # are queued behind the count pass and run while the host waits for the count and prepares the write pass
        early = {}

        def while_waiting():
            early["skippable"] = torch.zeros(1, dtype=torch.int64, device=device)
            if may_record:
                early["rows"] = self.ray_table(rays_o, rays_d)
            elif table:
                early["shq"] = self.sh_table(rays_d)

        def feed_of(M):
            early["plan"] = self.plan_frame(M, records=may_record)
            return raymarching.RECORDS if early["plan"]["feed"] == "records" else True
        xyzs, dirs, deltas, rays = raymarching.march_rays_patch(
            rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars,
            dt_gamma, max_steps, noises=jitter, counter=counter, table=feed_of if table else False,
            while_waiting=while_waiting)
        records = None
        gate.acquire()
        if not table:
            sigmas, rgbs = self(xyzs, dirs)
        elif early["plan"]["feed"] == "records":
            # xyzs is t [M]; the compositing rebuilds (dt, t - t_prev) from it and the rays' start
            records = raymarching.MarchRecords(nears, jitter, dt_gamma, max_steps, self.cascade, self.grid_size)
            sigmas, rgbs = self.forward_table(xyzs, dirs, rays_d, shq=early["rows"], rays_o=rays_o, plan=early["plan"])
            deltas = xyzs
        else:       # (a frame that could have recorded but is sliced or probing: the [N,16] table is built here)
            sigmas, rgbs = self.forward_table(xyzs, dirs, rays_d, shq=early.get("shq"), plan=early["plan"])
        gate.release()
        if self.density_scale != 1:
            sigmas = self.density_scale * sigmas
        skippable = early["skippable"]
        if fused_inst:
            # weights first, then the instance field accumulates w * logits on chip (no [M, K] round trip)
            weights_sum, depth, image, wbuf = raymarching.composite_rays_patch(sigmas, rgbs, deltas, rays, T_thresh,
                                                                              return_weights=True, skippable=skippable)
            gate.acquire()                   # a gather kernel too: never beside another view's field kernel
            results["instance"] = self.instance_render(xyzs, rays, wbuf, normalised=table).view(*prefix, -1)
            gate.release()
        else:
            weights_sum, depth, image = self._composite_with_logits(
                raymarching.composite_rays_patch, results, prefix, xyzs, sigmas, rgbs, deltas, rays, T_thresh,
                skippable=skippable, **({"records": records} if records is not None else {}))
        results["num_samples"] = counter
        if table:
            results["frame_path"] = self.last_frame_path     # "fused" | "sliced" [+ " (probing)"]
            results["frame_feed"] = early["plan"]["feed"]    # "records" | "positions"
        self._note_skippable(skippable, int(xyzs.shape[0]), False)       # raw counter, marched total (host), "skippable"
        return weights_sum, depth, image

    def _render_ray_major(self, results, prefix, rays_o, rays_d, nears, fars, marched, dt_gamma, max_steps, perturb, noises,
                          force_all_rays, T_thresh, ce_labels, ce_ignore_index):
        """Training, and ``fused_raymajor``: ray-major samples (taken from ``marched`` when there is one), field and
        compositing as autograd nodes."""
        with_instance = self.num_instances > 0
        if marched is not None:
            counter = marched.counter
            xyzs, dirs, deltas, rays = marched.xyzs, marched.dirs, marched.deltas, marched.rays
        else:
            if self.training:
                _, counter = self._take_counter_slot()
                mean_count = self.mean_count
            else:
                counter = torch.zeros(2, dtype=torch.int32, device=rays_o.device)
                mean_count = -1
                force_all_rays = True
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(
                rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars,
                counter, mean_count, perturb, 128, force_all_rays, dt_gamma, max_steps, noises=noises)
        if self.training:
            self.last_counter = counter          # (total samples, N) of the march this render consumed
        head = with_instance and self.instance_head_available(xyzs)
        shaded = marched.shaded_for(T_thresh, self.density_scale) if marched is not None else None
        if shaded is not None and not (head and self.shade_ahead_applies()):
            shaded = None
        if shaded is None:                       # else: frozen field + compositing forward were queued with the march
            sigmas, rgbs = self(xyzs, dirs)
            if self.density_scale != 1:
                sigmas = self.density_scale * sigmas
        if head:
            # the instance head as ONE autograd node (field + K-channel compositing; one backward launch)
            weights_sum, depth, image, wbuf, sample_ray = shaded if shaded is not None else raymarching.composite_rays_train(
                sigmas, rgbs, deltas, rays, T_thresh, return_weights=True, total_dev=counter)
            if ce_labels is not None:
                # the mask loss of the instance stage inside the compositing launch (Trainer.train_step passes the
                # batch's matched-mask ids): results["instance_ce"] = mean CE over the rows != ce_ignore_index
                inst, results["instance_ce"] = self.instance_head_train(
                    xyzs, wbuf, sample_ray, rays, n_dev=counter, ce_labels=ce_labels.reshape(-1),
                    ce_ignore_index=ce_ignore_index)
            else:
                inst = self.instance_head_train(xyzs, wbuf, sample_ray, rays, n_dev=counter)
            results["instance"] = inst[:, :self.num_instances].reshape(*prefix, -1)
        else:
            weights_sum, depth, image = self._composite_with_logits(
                raymarching.composite_rays_train, results, prefix, xyzs, sigmas, rgbs, deltas, rays, T_thresh,
                total_dev=counter)
        results["num_samples"] = counter
        return weights_sum, depth, image

    def _render_wavefront(self, results, prefix, rays_o, rays_d, nears, fars, dt_gamma, max_steps, perturb, T_thresh):
        """``wavefront``: upstream's loop over the rays still alive, a few steps per pass."""
        N, device = rays_o.shape[0], rays_o.device
        with_instance = self.num_instances > 0
        dtype = torch.float32
        weights_sum = torch.zeros(N, dtype=dtype, device=device)
        depth = torch.zeros(N, dtype=dtype, device=device)
        image = torch.zeros(N, 3, dtype=dtype, device=device)
        inst = torch.zeros(N, self.num_instances, dtype=dtype, device=device) if with_instance else None
        n_alive = N
        rays_alive = torch.arange(n_alive, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        step = 0
        while step < max_steps and n_alive > 0:
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d,
                                                        self.bound, self.density_bitfield, self.cascade,
                                                        self.grid_size, nears, fars, 128, perturb, dt_gamma,
                                                        max_steps)
            sigmas, rgbs = self(xyzs, dirs)
            sigmas = self.density_scale * sigmas
            extra = self.instance(xyzs) if with_instance else None
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum,
                                       depth, image, T_thresh, extra=extra, extra_acc=inst)
            rays_alive, n_alive = raymarching.compact_alive(rays_alive, n_alive)
            step += n_step
        if with_instance:
            results["instance"] = inst.view(*prefix, -1)
        return weights_sum, depth, image

    def _finish_rays(self, results, prefix, weights_sum, depth, image, nears, fars, bg_color, mse_target, one_pass, jitter,
                     dt_gamma, max_steps):
        """Depth convention, background blend and (``mse_target``) the image loss -> ``results`` with image, depth and
        weights_sum in the caller's shape.  ``one_pass``: the samples were composited by a one-pass inference mode;
        ``jitter``: the per-ray noise their march started with, or None."""
        N = weights_sum.shape[0]
        # Depth.  Upstream's training compositing counts t from the ray's first step, its inference compositing uses
        # the absolute ray parameter (SURVEY Appendix A.1 "Inference loop").  The one-pass inference modes composite
        # like the training kernel, so they add the start parameter back: sum w (t0 + t_rel) = depth + t0 * sum w.
        # (The wavefront mode runs upstream's loop and is absolute already.)
        t_start = None
        if one_pass:
            t_start = nears
            if jitter is not None:
                dt_min = 2 * math.sqrt(3) / max_steps
                dt_max = 2 * math.sqrt(3) * 2 ** (self.cascade - 1) / self.grid_size
                t_start = nears + torch.clamp(nears * dt_gamma, dt_min, dt_max) * jitter.to(nears)
        bg3 = self._bg_triplet(bg_color)
        flows = torch.is_grad_enabled() and (image.requires_grad or weights_sum.requires_grad)
        bg_per_ray = torch.is_tensor(bg_color) and bg_color.is_cuda and bg_color.numel() == 3 * N
        bg_trained = torch.is_tensor(bg_color) and bg_color.requires_grad      # the fused tail gives a background no gradient
        if (self.training and mse_target is not None and flows and t_start is None and image.is_cuda and not bg_trained
                and 0 < N <= raymarching.FINISH_MSE_MAX_RAYS and (bg3 is not None or bg_per_ray)):
            image, depth, results["image_mse"] = raymarching.finish_rays_mse(
                image, weights_sum, depth, nears, fars, bg3 if bg3 is not None else bg_color, mse_target)
        elif bg3 is not None and not flows:
            # no gradient flows through the shaded image (inference, or the instance stage on a frozen NeRF):
            # background blend + depth normalisation in one launch, in place on this call's own buffers
            lib = _lib.load()
            src_i, src_d = image.detach().contiguous(), depth.detach().contiguous()
            # the training path keeps the compositing outputs for its backward: write to fresh buffers there
            image = torch.empty_like(src_i) if self.training else src_i
            depth = torch.empty_like(src_d) if self.training else src_d
            check(lib.inr_finish_rays(ptr(src_i, torch.float32, "image"), ptr(src_d, torch.float32, "depth"),
                                      ptr(weights_sum.detach().contiguous(), torch.float32, "weights_sum"),
                                      ptr(nears, torch.float32, "nears"), ptr(fars, torch.float32, "fars"),
                                      ptr(t_start, torch.float32, "t0", allow_none=True),
                                      bg3[0], bg3[1], bg3[2], N, ptr(image), ptr(depth), stream_ptr()), "finish_rays")
        else:
            if isinstance(bg_color, (list, tuple)):
                bg_color = image.new_tensor(bg_color)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
            if t_start is not None:
                depth = depth + t_start * weights_sum.detach()
            depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        results["image"] = image.view(*prefix, 3)
        results["depth"] = depth.view(*prefix)
        results["weights_sum"] = weights_sum.view(*prefix)
        return results

    # infer_mode="auto": which kernel path pays?  The early-terminating kernel costs 1.20-1.26x per EVALUATED sample (a
    # wave owns a 16-ray group for all its steps, so the 256 waves of an XCD hold 256 patches at 256 different depths
    # where the two-kernel path holds a few patches' consecutive tiles: L2 miss rate 55 % against 37 %, measured -
    # profiles/r03_NOTES.txt section 13; 1.26-1.37x before the dynamic group schedule of round 3) and skips every step
    # at which the whole group is below T_thresh, so it wins when it skips more than 17-21 % of the marched samples -
    # against the statically dealt two-kernel path; with its hybrid schedule (late round 3: frames 3 % faster, the
    # trained scene 9 %) the ratio is 1.26-1.42x and the break-even 21-30 %: 35 % is used (margin against flapping).
    # The two-kernel path counts that fraction in its compositing kernel,
    # the terminating kernel reports what it really evaluated.  (Round 1 switched on mean opacity > 0.5: a half-trained
    # scene - opacity 0.88, only 8 % skippable - then rendered in 20.5 ms instead of 14.4, r02 notes section 11.)  The
    # value travels to the host through a pinned buffer + event and is only read once its copy has completed: no call
    # waits for a previous frame.
    # Round 4: 0.50.  The chunked variant the round-3 verdict proposed (two-kernel tile order, a per-group "dead" bit
    # between depth chunks) was not built: on every trained scene measured the skippable fraction is 5-8 % (trained room,
    # 1500 steps: 5.7 %), so even a termination that cost NOTHING would save at most that share of the field kernel
    # (10.5 -> 9.9 ms per frame), and every structure that tracks liveness per group has cost 18-42 % per evaluated
    # sample so far (profiles/r03k_terminate_vs_two_kernel_pmc.txt: L2 miss rate 55 % against 37 %).  `auto` therefore
    # takes the terminating kernel only where it wins by a wide margin - scenes that skip more than half of what they
    # march (the opaque test scene: 1.0 against 5.75 ms); profiles/r04_NOTES.txt 5.
    terminate_above = 0.50

    def _note_skippable(self, counter, total, counts_evaluated):
        """counter: the device counter of the frame (samples skippable / samples evaluated); total: marched samples, known
        on the host.  The raw 8-byte counter is copied to a pinned scalar and divided on the host once it has landed (the
        fraction used to be formed by four tiny device kernels per frame)."""
        if not counter.is_cuda:
            v = float(counter.reshape(-1)[0]) / max(total, 1)
            self._skippable_value = 1.0 - v if counts_evaluated else v
            return
        d = self.__dict__
        if "_skippable_free" not in d:             # four pinned scalars, allocated once
            d["_skippable_free"] = [torch.empty(1, dtype=torch.int64, pin_memory=True) for _ in range(4)]
            d["_skippable_pending"] = []
        self._recent_skippable()                   # recycles the slots whose copies have landed
        if not d["_skippable_free"]:
            return                                 # four samples still in flight: skip this one
        host = d["_skippable_free"].pop()
        host.copy_(counter.reshape(-1)[:1].view(torch.int64), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        d["_skippable_pending"].append((ev, host, total, counts_evaluated))

    def _recent_skippable(self):
        d = self.__dict__
        pending = d.get("_skippable_pending", [])
        while pending and pending[0][0].query():
            _, host, total, counts_evaluated = pending.pop(0)
            v = float(int(host[0])) / max(total, 1)
            d["_skippable_value"] = 1.0 - v if counts_evaluated else v
            d["_skippable_free"].append(host)
        return d.get("_skippable_value", 0.0)

    @staticmethod
    def _bg_triplet(bg_color):
        """(r, g, b) floats when the background is one colour for all rays (a number or a host-side triple)."""
        if isinstance(bg_color, (int, float)):
            return (float(bg_color),) * 3
        if isinstance(bg_color, (list, tuple)) and len(bg_color) == 3 and all(isinstance(c, (int, float)) for c in bg_color):
            return tuple(float(c) for c in bg_color)
        return None

    # ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """Marks cells no training camera sees with -1 (they never become occupied); upstream
        ``NeRFRenderer.mark_untrained_grid``.  One launch over all cascades and cells (inr_mark_untrained_grid);
        ``S`` (upstream's chunk size) is accepted and unused."""
        if not self.cuda_ray:
            return
        if not torch.is_tensor(poses):
            poses = torch.as_tensor(poses)
        dev = self.density_grid.device
        poses = poses.to(dev).float().contiguous().view(-1, 16)
        fx, fy, cx, cy = [float(v) for v in intrinsic]
        check(_lib.load().inr_mark_untrained_grid(ptr(poses, torch.float32, "poses", allow_none=poses.shape[0] == 0),
                                                  poses.shape[0], fx, fy, cx, cy, self.grid_size, self.cascade,
                                                  float(self.bound), ptr(self.density_grid, torch.float32, "density_grid"),
                                                  stream_ptr()), "mark_untrained_grid")

    def shade_ahead_applies(self):
        """``march_ahead(shade=True)`` may also run the field and the compositing forward: a FROZEN NeRF on the fused
        kernel (nothing of it is trained, so neither launch depends on what the step in flight updates) rendered
        together with the one-node instance head."""
        if not (self.num_instances > 0 and self._fusable and self._fusable_inst):
            return False
        if any(p.requires_grad for p in self._nerf_params()):
            return False
        inst = [self.instance_encoder.embeddings] + [l.weight for l in self.instance_net]
        return bool(self._fusable_inst and self.fused_instance_train and self.fused_instance_head
                    and all(p.requires_grad for p in inst))

    @torch.no_grad()
    def march_ahead(self, rays_o, rays_d, dt_gamma=0, perturb=False, max_steps=1024, stream=None, shade=False,
                    T_thresh=1e-4, bufs=None, counter=None, skip_labels=None, ignore_index=-1):
        """The parameter-independent head of a TRAINING render - ray/box test, jitter, march (count, scan, write) - queued
        now, on ``stream`` (a side stream: it then runs beside whatever the current stream is busy with - the previous
        step's backward, whose table-gradient scatter leaves the CUs idle; measured: ~47 of its ~60 us hide), for a
        ``render(..., marched=<result>)`` of the SAME rays later.  Needs the steady state (``mean_count > 0``: no host
        read-back) and an occupancy grid that will not change in between (the caller's business: ``Trainer`` skips the
        step before an occupancy update).  -> the ``MarchedHead`` ``run_cuda`` takes as ``marched``, or None
        (nothing queued, nothing counted: the caller marches in the step as usual).

        shade (round 4): with a frozen NeRF under the one-node instance head (``shade_ahead_applies``) the field
        evaluation and the compositing forward do not depend on the trained parameters either: both are queued behind
        the march, into the same persistent buffer set - ~165 us of the instance stage's ~0.83 ms step that can run
        beside the atomic-bound scatter.  ``bufs`` / ``counter``: a caller-owned buffer set
        (``raymarching.march_train_buffers(shade=...)``) and sample counter (int32 [2]) instead of the renderer's two
        alternating sets and its ``step_counter`` slot - the captured pipeline of ``Trainer`` owns both.
        ``skip_labels`` (int64, one per ray): rays labelled ``ignore_index`` are not marched (``render(ce_prune=True)``)."""
        if not (self.cuda_ray and self.training and self.mean_count > 0 and rays_o.is_cuda):
            return None
        rays_o_in, rays_d_in = rays_o, rays_d
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N = rays_o.shape[0]
        # the persistent buffers need the staged wave-per-ray marcher (its write pass clears the rows no ray owns):
        # larger batches, longer rays or set_march_mode(0) fall back to the in-step march - asked BEFORE a counter slot
        # is taken (round-3 advisor: the refusal used to surface as a RuntimeError inside the backward hook)
        if not _lib.load().inr_march_write_fills_unowned_rows(N, raymarching.SAMPLE_CAP_TRAIN, int(max_steps)):
            return None
        shade = bool(shade) and self.shade_ahead_applies()
        main = torch.cuda.current_stream()
        side = stream if stream is not None else main
        if side is not main:
            side.wait_stream(main)               # rays, bitfield and mean_count as the current stream leaves them
        # Two persistent buffer sets, used in turn and allocated HERE, on the current stream's pool: nothing is allocated
        # on the side stream (the caching allocator keeps a pool per stream; blocks that cross streams are freed late and
        # cost ~0.2 ms of host time per step - measured, profiles/r03_NOTES.txt 16).  Set A is read by step i (forward
        # and, through autograd's saved tensors, backward) while the side stream fills set B for step i + 1; set A is
        # written again for step i + 2 only after `side.wait_stream(main)` below, i.e. behind all of step i's launches.
        M_al = raymarching.sample_capacity(self.mean_count)
        if bufs is not None:
            b = bufs
            if b["n_rays"] != N or b["n_samples"] < M_al or (shade and "sigmas" not in b):
                raise RuntimeError("march_ahead(bufs=): buffer set of another batch size")
        else:
            own = getattr(self, "_ahead_bufs", None)
            if (own is None or own[0]["n_rays"] != N or own[0]["n_samples"] != M_al or own[0]["nears"].device != rays_o.device
                    or (shade and "sigmas" not in own[0])):
                own = self._ahead_bufs = [raymarching.march_train_buffers(N, M_al, rays_o.device, shade=shade) for _ in range(2)]
                self._ahead_turn = 0
            b = own[self._ahead_turn]
            self._ahead_turn ^= 1
        slot_taken = counter is None
        slot_index = -1
        if slot_taken:
            slot_index, counter = self._take_counter_slot()
        with torch.cuda.stream(side):
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, self.aabb_train, self.min_near,
                                                         out=(b["nears"], b["fars"]), skip_labels=skip_labels,
                                                         ignore_index=ignore_index)
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(
                rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars,
                counter, self.mean_count, perturb, 128, False, dt_gamma, max_steps, out=b)
            shaded = None
            if shade:
                M = xyzs.shape[0]
                sigmas, rgbs = b["sigmas"][:M], b["rgbs"][:M]
                self._fused_nerf(xyzs, dirs, True, False, out=(sigmas, rgbs))
                if self.density_scale != 1:
                    sigmas.mul_(self.density_scale)
                shaded = raymarching.composite_rays_train_into(sigmas, rgbs, deltas, rays, T_thresh, b)
            done = None
            if side is not main:
                done = torch.cuda.Event()
                done.record(side)
        return MarchedHead(rays_o_in, rays_d_in, skip_labels, N, self.iter_density, nears, fars, xyzs, dirs, deltas, rays,
                           counter, shaded, T_thresh, self.density_scale, slot_taken, slot_index, done, side)

    def drop_ahead(self, marched):
        """A prefetched march that no render will consume: give its ``step_counter`` slot back (it would otherwise count
        as a step of its own in the next ``mean_count``) - but only while it is still the MOST RECENT slot (round-4
        advisor: if another training render took a slot in between, stepping back would make the next render overwrite
        that real step's counter).  An orphaned slot further back is left alone: it holds the sample total of a real
        march of a real batch, a valid sample of what ``mean_count`` averages."""
        if marched is not None and marched.slot_taken and self.local_step > 0:
            if marched.slot_index == (self.local_step - 1) % 16:
                self.local_step -= 1
            marched.slot_taken = False

    @torch.no_grad()        # as upstream's: without it the NeRF stage's update ran the density query through the
    #                          composable autograd path (HIP encoder + BLAS layers, graph and all): 2.0 instead of 1.0 ms
    def update_extra_state(self, decay=0.95, S=128):
        """EMA-max occupancy update + bitfield rebuild (SURVEY a3, Appendix A.1 "Occupancy update"; upstream
        ``NeRFRenderer.update_extra_state``).  First 16 calls: every cell of every cascade; afterwards H^3/4 uniformly
        random cells plus H^3/4 random occupied cells per cascade.  All on the device: query positions
        (inr_occ_cell_positions, Morton order), sigma through the fused field kernel, EMA-max + mean
        (inr_occ_update) and the bitfield with its threshold min(mean, density_thresh) formed on the device
        (inr_packbits_mean).  The host needs ONE number back, the mean sample count that sizes the next 16 steps'
        buffers, and the counters it comes from are final before the update starts: their read-back is queued first
        and waited for last, so the call returns with its kernels still queued and the next step is enqueued under
        them (waiting for the update's own result left the device idle for ~0.3 ms while the host caught up;
        profiles/r03_NOTES.txt 20).  The mean density stays on the device until it is asked for (``mean_density``).
        ``S`` is accepted for upstream's signature; nothing is chunked here."""
        if not self.cuda_ray:
            return
        lib = _lib.load()
        dev = self.density_bitfield.device
        H, C = self.grid_size, self.cascade
        n_cells = H ** 3
        st = stream_ptr()
        total_step = min(16, self.local_step)
        counted = None
        if total_step > 0:
            host = self.__dict__.get("_count_host")
            if host is None:
                host = self.__dict__["_count_host"] = torch.empty(1, dtype=torch.int64).pin_memory()
            host.copy_(self.step_counter[:total_step, 0].sum(0, keepdim=True, dtype=torch.int64), non_blocking=True)
            counted = torch.cuda.Event()
            counted.record()
        mean_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        grid = self.density_grid
        full = self.iter_density < 16
        for cas in range(C):
            bnd = float(min(2 ** cas, self.bound))
            if full:
                idx, m = None, n_cells
            else:
                n = n_cells // 4
                # n uniformly random cells + n random occupied cells (with replacement), chosen on the device in three
                # launches and grouped by slices of the Morton range (inr_occ_sample_cells; upstream: randint coords,
                # nonzero -> sync, randint picks - here no host round trip and no tensor-op chain)
                u = torch.rand(4 * n, dtype=torch.float32, device=dev)
                idx = torch.empty(2 * n, dtype=torch.int32, device=dev)
                work = torch.empty(lib.inr_occ_sample_workspace_bytes(n_cells) // 8 + 1, dtype=torch.int64, device=dev)
                check(lib.inr_occ_sample_cells(ptr(grid[cas], torch.float32, "density_grid"), n_cells, ptr(u), n, ptr(idx),
                                               ptr(work), st), "occ_sample_cells")
                m = 2 * n
            xyz = torch.empty(m, 3, dtype=torch.float32, device=dev)
            noise = torch.rand_like(xyz)
            check(lib.inr_occ_cell_positions(ptr(idx, torch.int32, "morton_idx", allow_none=True),
                                             ptr(noise, torch.float32, "noise"), m, H, bnd, ptr(xyz), st),
                  "occ_cell_positions")
            sigma = self.density_sigma(xyz).reshape(-1).detach().float().contiguous()
            tmp = None if full else torch.empty(n_cells, dtype=torch.float32, device=dev)
            check(lib.inr_occ_update(ptr(grid[cas], torch.float32, "density_grid"), ptr(sigma, torch.float32, "sigma"),
                                     ptr(idx, torch.int32, "morton_idx", allow_none=True), n_cells, m, float(decay),
                                     float(self.density_scale), ptr(tmp, allow_none=True), ptr(mean_sum), st),
                  "occ_update")
        stats = torch.empty(2, dtype=torch.float64, device=dev)
        check(lib.inr_packbits_mean(ptr(grid, torch.float32, "density_grid"), C * n_cells, ptr(mean_sum),
                                    float(self.density_thresh), ptr(self.density_bitfield, torch.uint8, "density_bitfield"),
                                    None, ptr(self.step_counter, torch.int32, "step_counter"), max(total_step, 1),
                                    self.step_counter.stride(0), ptr(stats), st), "packbits_mean")
        self.iter_density += 1
        self.__dict__["_mean_density_dev"] = stats         # [mean density, sum of the sample totals]: read on demand
        if counted is not None:
            counted.synchronize()                          # reached before the first kernel of this update ran
            self.mean_count = int(float(host[0]) / total_step)
        self.local_step = 0

    # ----------------------------------------------------------------------------------------
    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """rays_o, rays_d [B,N,3] -> dict of [B,N,...] tensors (upstream signature)."""
        _run = self.run_cuda if self.cuda_ray else self.run
        B, N = rays_o.shape[:2]
        # upstream chunks staged renders to fit a 24 GB card; a 640 000-ray frame needs ~2 GB of the 288 GB here, and
        # rays are independent (chunking never changes a result), so chunks are at least `min_staged_batch` rays.
        # Set model.min_staged_batch = 0 for upstream's exact chunk size.
        if self.cuda_ray:
            max_ray_batch = max(int(max_ray_batch), int(self.min_staged_batch))
        if staged and N > max_ray_batch:
            if not self.training and kwargs.get("infer_mode", "auto") == "auto":
                # one mode per frame: every chunk of a staged render takes the same kernel path
                kwargs = dict(kwargs, infer_mode="fused_terminate" if self._recent_skippable() > self.terminate_above else "fused")
            chunks = {}
            for b in range(B):
                head = 0
                while head < N:
                    tail = min(head + max_ray_batch, N)
                    r = _run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                    for k, v in r.items():
                        # per-ray results only ([1, n, ...]); the sample counters of a chunk are not concatenated
                        if torch.is_tensor(v) and v.dim() >= 2 and v.shape[:2] == (1, tail - head):
                            chunks.setdefault((k, b), []).append(v)
                    head += max_ray_batch
            keys = sorted({k for k, _ in chunks})
            n_chunks = (N + max_ray_batch - 1) // max_ray_batch
            keys = [k for k in keys if all(len(chunks.get((k, b), ())) == n_chunks for b in range(B))]
            return {k: torch.cat([torch.cat(chunks[(k, b)], 1) for b in range(B)], 0) for k in keys}
        return _run(rays_o, rays_d, **kwargs)


class FramePipeline:
    """View-after-view rendering on two alternating streams: while the field kernel of view i runs, the compositing of
    view i-1 and the ray/box test + march of view i+1 (VALU work with a host read-back of the sample count in the
    middle) run beside it.  The field kernels themselves stay one after the other (``field_gate``): two of them at once
    only halve each other's cache.  In-stream order bounds the look-ahead to one view.

    ``render`` returns when its view is queued; the results live on the stream returned with them
    (``out["stream"]``): use them there, or ``synchronize()`` first.  Overlap placement (include/inr.h,
    inr_set_overlap_placement) is on while the pipeline is open.  Upstream has no counterpart (its loop renders one view
    at a time on the default stream); images are bit identical to ``net.render``."""

    def __init__(self, net, device=None):
        self.net = net
        self.streams = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)]
        self._turn = 0
        self._field_done = None
        self.open()

    def open(self):
        """(Re)opens a closed pipeline: overlap placement on.  The two streams live as long as the object."""
        # INR_PIPELINE_PLACEMENT=0: A/B switch (with the hybrid tile schedule the placement is worth 1.3 %, 6.34-6.39
        # against 6.26-6.30 Gsamples/s; with the static deal it was the difference between winning and losing)
        raymarching.set_overlap_placement(os.environ.get("INR_PIPELINE_PLACEMENT", "1") != "0")

    # field_gate protocol of NeRFRenderer.run_cuda
    def acquire(self):
        if self._field_done is not None:
            torch.cuda.current_stream().wait_event(self._field_done)

    def release(self):
        self._field_done = torch.cuda.Event()
        self._field_done.record(torch.cuda.current_stream())

    def next_stream(self):
        st = self.streams[self._turn]
        self._turn ^= 1
        return st

    def render(self, rays_o, rays_d, stream=None, **kwargs):
        """``stream``: the pipeline stream the rays were produced on (from ``next_stream()``), or None when they come
        from the current stream."""
        if kwargs.pop("staged", False):
            raise RuntimeError("FramePipeline renders a whole view per call (staged=False)")
        if stream is None:
            stream = self.next_stream()
            stream.wait_stream(torch.cuda.current_stream())
            rays_o.record_stream(stream)
            rays_d.record_stream(stream)
        with torch.cuda.stream(stream):
            out = self.net.render(rays_o, rays_d, staged=False, field_gate=self, **kwargs)
        out["stream"] = stream
        return out

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def close(self):
        self.synchronize()
        raymarching.set_overlap_placement(False)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
