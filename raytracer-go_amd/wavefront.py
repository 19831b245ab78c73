"""A wavefront path tracer in thirty lines of torch over the library's path building blocks (include/rtx.h, "path
building blocks"): rtx_camera_rays_device -> (rtx_trace_device -> rtx_shade_device) x max_depth.

This is Ray.GetColor (ray.go:32-54) of the reference with the recursion turned into rounds over all paths at once.  It
is the example an integrator of one's own starts from (a light tracer, an AOV pass, a torch-side estimator; direct
lighting is render(direct=True) below, over rtx_direct_device), and the loop the tests hold to the oracle: on a scene
that keeps the caller's tree its image equals rtx_render_region_device's bit for bit on every pixel, because camera
rays, hits and scatters are computed by the render's own device code and the colour arithmetic below is the render's:
float32, one rounding per multiply and per add, in the same order (torch's eager `a * b` and `a + b` are separate kernels; nothing here may
be replaced by addcmul or a compiled graph that fuses them).  On the library's own trees a trace may resolve a rare
grazing hit differently from the render's walk: 4 pixels of a 1920x1080x8 frame.

The megakernel renders the same frame many times faster (scripts/shade_rates.py measures how much): every round here
reads and writes each path's records in HBM and launches a dozen small torch kernels."""
from __future__ import annotations

import rtx

_MISS = -1  # RTX_HIT_NONE seen through an int32 view


def render(dev: "rtx.DeviceScene", cam: "rtx.Camera", seed: int, region: "rtx.Region", compact: bool = False,
           counters: bool = False, direct: bool = False, mis: bool = False):
    """The region's shard rendered on the current device: a float32 torch tensor [rows, width, 3] there (on the
    caller's tree every value is the one rtx_render_region_device gives).  compact=True drops ended paths between rounds (torch indexing) instead
    of carrying them as misses.  counters=True also returns the dict of sums {segments, hits, rng_draws,
    texel_fetches} of the render's rtx_stats (each round then waits for its counting shade).

    direct=True is the next-event estimator of DESIGN.md §37 over trace -> shade -> rtx_direct_device: at a Lambertian
    hit of segment s with s + 1 < max_depth one light sample is added when its shadow ray is free, and the radiance
    the bounce after a Lambertian hit would have found by hitting an emitter is left out.  Same mean as the plain
    render, another image; with no emitter in the scene it IS the plain render.  rng_draws then includes the light
    samples' draws.

    direct=True, mis=True is the estimator of DESIGN.md §42 (rtx.h, "multiple importance sampling of the direct light"):
    the light sample is weighted by wl = 1 / (1 + g * g) of its own geom, and the emission a bounce after a Lambertian
    hit finds is kept, weighted by rtx_emitter_weight_device's wb of (the previous round's hit, this hit).  mis without
    direct changes nothing."""
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    cuda = torch.device("cuda", torch.cuda.current_device())
    rows, width, spp = rtx.region_rows(region), region.width, cam.samples_per_pixel
    n = spp * rows * width
    L = torch.zeros((n, 3), dtype=torch.float32, device=cuda)
    work = {"segments": 0, "hits": 0, "rng_draws": 0, "texel_fetches": 0}
    if n:
        # records as rows of 32-bit words: ray 8, key 4, hit 12, bounce 16 (rtx.h); torch allocations are 16-B aligned
        rays = torch.empty((n, 8), dtype=torch.float32, device=cuda)
        keys = torch.empty((n, 4), dtype=torch.int32, device=cuda)
        hits = torch.empty((n, 12), dtype=torch.int32, device=cuda)
        bounce = torch.empty((n, 16), dtype=torch.float32, device=cuda)
        rtx.camera_rays_device(cam, seed, region, 0, spp, rays.data_ptr(), keys.data_ptr(), stream)
        if counters:
            work["rng_draws"] += int(keys[:, 3].sum())
        T = torch.ones((n, 3), dtype=torch.float32, device=cuda)
        background = torch.tensor(list(cam.background), dtype=torch.float32, device=cuda)
        path = torch.arange(n, device=cuda)        # the row of L each record adds to
        alive = torch.ones(n, dtype=torch.bool, device=cuda)
        flags = rtx.RTX_SHADE_COUNTERS if counters else 0
        n_lights = len(dev.lights()) if direct else 0
        if n_lights:
            light = torch.empty((n, 16), dtype=torch.float32, device=cuda)  # rtx_direct_sample: 16 words
            diffuse = torch.zeros(n, dtype=torch.bool, device=cuda)          # the last bounce left a Lambertian
            if mis:
                prev = hits                                                  # the previous round's hit records
                weight = torch.empty((n, 4), dtype=torch.float32, device=cuda)  # rtx_emitter_weight_record: 4 words
                one = torch.ones((), dtype=torch.float32, device=cuda)
        for s in range(cam.max_depth):
            m = rays.shape[0]
            if counters:
                work["segments"] += int(alive.sum())
            dev.trace_device(rays.data_ptr(), m, hits.data_ptr(), rtx.RTX_TRACE_UV, stream)
            st = dev.shade_device(seed, rays.data_ptr(), hits.data_ptr(), keys.data_ptr(), m, bounce.data_ptr(), flags,
                                  stream, stats=counters)
            if counters:
                work["hits"] += st.hits
                work["rng_draws"] += st.rng_draws
                work["texel_fetches"] += st.texel_fetches
            b = bounce[:m]
            bits = b.view(torch.int32)[:, 3]
            hit = alive & (hits[:m, 1] != _MISS)
            miss = alive & ~hit
            emits = hit & ((bits & rtx.RTX_BOUNCE_EMITS) != 0)
            alive = hit & ((bits & rtx.RTX_BOUNCE_SCATTERED) != 0)
            if n_lights:
                if mis and s > 0 and bool(diffuse.any()):  # the bounce's share of the emitter point it found
                    dev.emitter_weight_device(prev.data_ptr(), hits.data_ptr(), m, weight.data_ptr(), 0, stream)
                    shared = emits & diffuse
                    wb = weight[:m, 0]
                    L[path[shared]] = L[path[shared]] + T[shared] * (b[shared, 4:7] * wb[shared][:, None])
                emits = emits & ~diffuse  # a light sample at the last hit stood for this radiance
            L[path[miss]] = L[path[miss]] + T[miss] * background          # ray.go:52
            L[path[emits]] = L[path[emits]] + T[emits] * b[emits, 4:7]    # ray.go:41, 47
            if n_lights and s + 1 < cam.max_depth:
                st = dev.direct_device(seed, hits.data_ptr(), keys.data_ptr(), m, light.data_ptr(),
                                       rtx.RTX_DIRECT_COUNTERS if counters else 0, stream, stats=counters)
                if counters:
                    work["rng_draws"] += st.rng_draws
                d = light[:m]
                words = d.view(torch.int32)
                # (only a Lambertian hit draws: rng_draws != 0 names the material without a table of its own.  `diffuse`
                # is therefore set only in rounds where the block ran; the one round where it does not, the last, reads
                # the flag of the round before and sets none that is read: the same as `diffuse = lam` every round)
                diffuse = alive & (words[:, 13] != 0)
                lit = diffuse & ((words[:, 3] & rtx.RTX_DIRECT_VISIBLE) != 0)
                if mis:
                    g = d[lit, 14]
                    L[path[lit]] = L[path[lit]] + T[lit] * (d[lit, 0:3] * (one / (one + g * g))[:, None])
                else:
                    L[path[lit]] = L[path[lit]] + T[lit] * d[lit, 0:3]
            if compact:
                if not bool(alive.any()):
                    break
                T = T[alive] * b[alive, 0:3]                              # ray.go:47-50
                rays, keys, path = b[alive, 8:16].contiguous(), keys[alive].contiguous(), path[alive]
                if n_lights:
                    diffuse = diffuse[alive]
                    if mis:
                        prev = hits[:m][alive].contiguous()
                alive = torch.ones(rays.shape[0], dtype=torch.bool, device=cuda)
            else:
                T = torch.where(alive[:, None], T * b[:, 0:3], T)
                rays = b[:, 8:16].contiguous()  # an ended path's bounce ray is all zero: a miss from now on
                if n_lights and mis:
                    prev = hits.clone()
            keys[:, 2] += 1  # the next scatter's event
    # camera.go:254-263: the samples summed in k order, times float32(1 / spp)
    per_sample = L.view(spp, rows * width, 3)
    total = torch.zeros((rows * width, 3), dtype=torch.float32, device=cuda)
    for k in range(spp):
        total = total + per_sample[k]
    one = torch.ones((), dtype=torch.float32, device=cuda)
    image = (total * (one / float(spp))).view(rows, width, 3)
    return (image, work) if counters else image
