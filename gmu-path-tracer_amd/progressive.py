"""Headless progressive front-end: what Window::loop + GUI do around Renderer::update()/draw() in the reference
(Source/Window.cpp:60-90, Source/GUI.cpp:43-131), without a window.

A session iterates continuously; between frames it applies the events the reference takes from its GUI -- camera motion (with the
accumulation-reset hysteresis of Camera.cpp:72-83, implemented in the host camera), light edits (buffer re-upload + restart,
GUI.cpp:125-130), resolution switches (Renderer.cpp:408-413) -- and every `preview_every` frames it gathers the row-band tiles of all
ranks to rank 0 (tiles.gather_tiles: RCCL over xGMI with the "nccl" backend, gloo in the CPU tests) and hands the frame to a callback.
The renderer / camera objects are the C-ABI wrappers of capi (or anything with the same methods).
"""
import numpy as np

from . import tiles


def to_rgba8(frame):
    """The 8-bit image Renderer::captureScreen writes (Source/Renderer.cpp:383-394): uint8 = float * 255 truncated, alpha 255."""
    out = np.empty(frame.shape, np.uint8)
    out[..., :3] = (frame[..., :3] * 255.0).astype(np.uint8)
    out[..., 3] = 255
    return out


class ProgressiveSession:
    def __init__(self, renderer, camera, width, height, rank=0, world=1, dist=None, preview_every=32, on_preview=None, motion=False):
        self.renderer, self.camera = renderer, camera
        self.width, self.height = width, height
        self.rank, self.world, self.dist = rank, world, dist
        self.preview_every, self.on_preview = preview_every, on_preview
        self.frames = 0
        self.previews = 0
        self.temporal = None   # the history handle of denoised_temporal, created on first use
        self.converge = None   # the convergence monitor of run_until, created on first use
        self.adaptive = None   # the sampling plan of run_until(adaptive=True), created on first use
        self._planned = False  # the plan is attached to the renderer
        self.motion = bool(motion)   # denoised_temporal goes through the motion entry point (also set by set_vertices(keep_history=True))
        self.lbvh = None       # the GPU tree builder of rebuild(), created on first use
        self._indices = None   # the index list of the last rebuild()
        self.normals = None    # the capi.Normals of set_vertices(normals="smooth"), created on first use, dropped by rebuild()
        self.baseline = None   # the tree cost (sah) that set_vertices(rebuild_above=...) compares a refitted tree with; rebuild() forgets it
        self._epoch = 0        # accumulations started (a frame that cleared the target, a resize): what denoised_temporal(lens_guides=True) folds its history by
        self._guided_epoch = None   # the epoch of its last call
        self.projection = None # the capi.projection.Projection of set_projection(); None = the pinhole
        self._shutter_fraction = None   # set_shutter(fraction=f): the session sets the close pose of every frame
        self._shutter_prev = None       # ... from the pose of the frame before (a capi.shutter.Shutter), None after a resize

    # ---- events (applied before the next frame, like the GUI callbacks of the reference)
    def move_camera(self, mouse_dx=0.0, mouse_dy=0.0, w=False, s=False, a=False, d=False):
        self.camera.set_input(mouse_dx, mouse_dy, w, s, a, d)

    def set_lights(self, light_buffer, lights, count):
        """GUI light editor: re-upload the light array, set lightCount, restart the accumulation (GUI.cpp:125-130)."""
        light_buffer.update(lights)
        self.camera.buffer.lightCount = count
        self.camera.reset_accumulation()
        if self.temporal is not None:
            self.temporal.reset()                    # the history was lit by the old lights
        self._reset_converge()

    def set_lens(self, aperture, focus=None, focus_at=None):
        """Depth of field (capi.lens, include/gmupt_lens.h): from the next frame on every fresh camera path starts on a disk of radius
        `aperture` (scene units) around the camera position and aims through its pinhole ray's point on the focal plane; aperture 0
        detaches the lens.  The plane is `focus` (its distance along the camera's forward axis) or, with focus_at=(px, py), the depth
        of what that whole-frame pixel sees under the camera of the frame just drawn (GmuptError when it sees nothing); exactly one
        of the two with an aperture > 0.  The accumulation restarts like after a camera move: the temporal history stays and is
        reprojected as usual (pick, the AOV planes and the projection stay on the pinhole centre ray).  Returns the capi.lens.Lens."""
        from .capi import lens as L
        if aperture > 0 and self.projection is not None:
            raise ValueError("set_lens: a projection is attached (set_projection): lens and projection do not combine")
        if aperture > 0 and (focus is None) == (focus_at is None):
            raise ValueError("set_lens: an open aperture takes either focus=distance or focus_at=(px, py)")
        if aperture > 0 and focus_at is not None:
            lens = L.focus_at(self.renderer, focus_at[0], focus_at[1], int(self.camera.buffer.lightCount), aperture_radius=aperture)
        elif focus is not None:
            lens = L.lens_params(aperture_radius=aperture, focus_distance=focus)
        else:
            lens = L.lens_params(aperture_radius=aperture)
        L.set_lens(self.renderer, lens)
        self.camera.reset_accumulation()
        self._reset_converge()                       # the batches seen so far are of the old lens
        return lens

    def set_shutter(self, close_camera=None, fraction=None):
        """Camera motion blur (capi.shutter, include/gmupt_shutter.h): from the next frame on every fresh camera path draws a time in
        [0, 1) and leaves the camera interpolated between the session's camera (shutter open) and a close pose; an attached lens or
        projection runs on that camera.  set_shutter() with no argument detaches.
        close_camera: an explicit close pose, a capi.CameraBuffer (or a camera with a `buffer`); it stays where it is put while the
        session's camera goes on moving, until the next set_shutter or a resize(), which detaches it.
        fraction=f in (0, 1]: the session sets the close pose itself on each later camera event -- a frame whose pose differs from the
        pose of the frame before -- by one rule: the shutter spans the last f of the way from the previous pose to the new one, open =
        the new camera, close = camera + (previous - camera) * f for the twelve pose components, in binary32.  (The box shutter does
        not tell open from close, so the exposure is the segment of that motion that ends at the new pose; no later pose is needed.)
        The close pose is then held: every frame of the accumulation that the event starts is made with the same shutter, until the
        next event.  While the camera moves every frame is an event.  Before the first event, and after a resize() until the next
        one, there is no previous pose of that aspect and nothing is attached: those frames are the frames without a shutter.
        The accumulation restarts like after set_lens: the temporal history stays and is reprojected as usual (pick, the AOV planes
        and the projection stay at t = 0), the convergence monitor is reset.  Returns the attached capi.shutter.Shutter, None when
        detached or when the first close pose is still to come (fraction)."""
        from .capi import shutter as S
        if close_camera is not None and fraction is not None:
            raise ValueError("set_shutter: either close_camera=pose or fraction=f, not both")
        if fraction is not None and not (0.0 < float(fraction) <= 1.0):
            raise ValueError("set_shutter: fraction=%r (a float in (0, 1])" % (fraction,))
        self._shutter_fraction = float(fraction) if fraction is not None else None
        self._shutter_prev = None
        sh = S.from_camera(getattr(close_camera, "buffer", close_camera)) if close_camera is not None else None
        S.set_shutter(self.renderer, sh)
        self.camera.reset_accumulation()
        self._reset_converge()                       # the batches seen so far are of the old shutter
        return sh

    def _follow_shutter(self):
        """fraction mode, before the frame's camera is set: on a camera event the close pose of the accumulation it starts (set_shutter
        has the rule); on any other frame nothing, the attached shutter is held."""
        from .capi import shutter as S
        cam = S.from_camera(self.camera.buffer)
        prev, self._shutter_prev = self._shutter_prev, cam
        if prev is None:
            S.set_shutter(self.renderer, None)       # no previous pose of this aspect yet
            return
        if bytes(prev) == bytes(cam):
            return
        sh, f = S.from_camera(self.camera.buffer), np.float32(self._shutter_fraction)
        for name in ("position", "upperLeftCorner", "horizontal", "vertical"):
            a, b = np.array(getattr(cam, name)[:], np.float32), np.array(getattr(prev, name)[:], np.float32)
            getattr(sh, name)[:] = [float(x) for x in (a + ((b - a).astype(np.float32) * f).astype(np.float32)).astype(np.float32)]
        S.set_shutter(self.renderer, sh)

    def set_projection(self, kind, fov=None, extent=None):
        """Another camera projection (capi.projection, include/gmupt_projection.h): kind "orthographic" (extent: the world-space height
        of the view), "fisheye" (fov: the angle across the image circle in radians, default pi), "equirect" (the 360-degree panorama)
        or "pinhole" / None, which detaches.  From the next frame on every fresh camera path gets that projection's ray, and the
        accumulation restarts like after a camera move.  While a projection is attached pick(), aovs() and denoised() go through the
        projected entry points (pinhole guides would show a different picture); denoised(infill=...) is the projected preview chain
        (the infill takes the projected records as they are), and preview() is a tile gather without guides, so it needs no routing.  What inverts a pinhole refuses with ValueError:
        denoised_temporal(), set_vertices / set_pose with keep_history=True, and set_lens with an aperture.  While a lens with an
        aperture is attached the library refuses the projection (GmuptError, ERR_UNSUPPORTED).  Returns the capi.projection.Projection (None when detached)."""
        from .capi import projection as P
        kind = P.KINDS.get(kind, kind) if kind is not None else P.PINHOLE
        fields = {k: v for k, v in (("fov", fov), ("extent", extent)) if v is not None}
        proj = P.projection_params(kind, **fields)
        P.set_projection(self.renderer, proj)        # GmuptError (ERR_UNSUPPORTED) while a lens with an aperture is attached
        self.projection = proj if proj.kind != P.PINHOLE else None
        self.camera.reset_accumulation()
        if self.temporal is not None:
            self.temporal.reset()                    # the history is another picture
        self._reset_converge()
        return self.projection

    def _no_projection(self, who):
        if self.projection is not None:
            raise ValueError("%s: a projection is attached (set_projection), and the temporal projection inverts a pinhole" % who)

    def set_vertices(self, scene_buffers, verts, normals=None, keep_history=False, indices=None, rebuild_above=None, optimize=0):
        """The geometry moved (same vertex count, same triangles): upload the vertices, and `normals` (when given) into the property
        records, refit the tree and the renderer's traversal tables on the GPU (gmupt_renderer_refit), restart the accumulation.  The
        temporal history shows the old surface and is dropped; with keep_history=True it is kept, and denoised_temporal() from then on
        looks it up where each surface point was (gmupt_render_denoised_temporal_motion).  The first such call still drops a history
        that earlier denoised_temporal() calls wrote, because its record sets carry no vertex pose; ProgressiveSession(..., motion=True)
        uses the motion entry point from the first preview on, so that nothing is dropped.  scene_buffers: the capi.SceneBuffers the
        renderer is bound to.  Returns the refit info dict.
        verts: a numpy array, or a torch tensor on the renderer's GPU (float32, contiguous), which goes from device memory to the vertex
        buffer without a trip through the host (Buffer.update_from_device).
        normals: None leaves the property records alone; an array is patched in through the host; "smooth" recomputes area-weighted
        vertex normals on the GPU before the refit (capi.Normals, created on first use and kept until rebuild() or close()), no host
        round trip.  Its index list is `indices` ((n, 3) int32, numpy or a torch device tensor; given only with the first "smooth"
        call, or to replace the list), else the list of the last rebuild(), else the triangle records the scene is bound to -- in which
        a triangle that the SBVH's spatial splits put into several leaves appears, and counts, several times.
        rebuild_above: None (the default) refits and never rebuilds.  A float > 1 is the refit-or-rebuild policy on the tree cost
        (capi.Renderer.tree_cost, measured on the GPU): the session's baseline is the sah of the tree as bound, taken before the upload
        when there is none yet.  After the refit, cost = the sah of the refitted tree.  When cost > rebuild_above * baseline, an LBVH
        candidate is built from the device-resident vertices (the indices and materials rebuild() would pick, its default leaf size)
        and its sah measured before anything is bound.  A cheaper candidate is adopted exactly as by rebuild() -- buffers swapped, bound,
        the Normals handle and the temporal history dropped -- and its cost is the new baseline; a candidate that is no cheaper is
        closed, the refitted tree stays and its cost becomes the baseline, so that a losing candidate is not built again every frame.
        A candidate the builder refuses with GMUPT_ERR_UNSUPPORTED (rule 9 of the LBVH: a tree deeper than 64 levels) is a candidate
        that lost: no exception, the refitted tree stays and its cost becomes the baseline, candidate_cost stays None and the dict
        also holds candidate_refused, the library's message.  Every other error of the build propagates.
        optimize: 0 (the default) leaves the candidate as built.  N > 0 runs N passes of the treelet optimiser on it (capi.TreeOptimizer,
        include/gmupt.h "Tree optimisation"): the optimised tree is the candidate that is measured, compared and bound, and
        candidate_cost is its cost.  An optimiser refusal with GMUPT_ERR_UNSUPPORTED (deeper than 64 levels) counts like the builder's.
        A baseline of 0 (a root without area) never triggers.  The returned dict then also holds cost, baseline (the value the
        decision was made against), candidate_cost (None when none was built) and tree_rebuilt.  There is no default threshold:
        DESIGN.md "Tree cost" has the measurements."""
        if keep_history:
            self._no_projection("set_vertices(keep_history=True)")
        rebuild_above = self._moved_args("set_vertices", normals, rebuild_above)
        if hasattr(verts, "is_cuda"):
            scene_buffers.verts.update_from_device(verts)
        else:
            scene_buffers.verts.update(np.ascontiguousarray(verts, np.float32))
        return self._after_vertices(scene_buffers, normals, keep_history, indices, rebuild_above, optimize)

    def set_pose(self, scene_buffers, pose, joint_mats, target_weights=None, normals=None, keep_history=False, indices=None, rebuild_above=None,
                 optimize=0):
        """The geometry moved because its rig did: pose.update(joint_mats, target_weights) (capi.Pose: skinning and morph targets on the
        GPU, a few kilobytes of input, no vertex array crosses the bus) writes the vertex buffer the renderer is bound to, then exactly
        what set_vertices does after its upload -- normals, refit, accumulation restart, history, the rebuild policy; the baseline of
        rebuild_above is taken before the pose.  The other arguments and the returned dict are set_vertices'.  joint_mats /
        target_weights: numpy arrays or torch device tensors.  The session does not own `pose`: a rebuild() that keeps the vertex count
        keeps it valid, and closing it is the caller's business (the renderer closes it at the latest)."""
        if keep_history:
            self._no_projection("set_pose(keep_history=True)")
        rebuild_above = self._moved_args("set_pose", normals, rebuild_above)
        pose.update(joint_mats, target_weights)
        return self._after_vertices(scene_buffers, normals, keep_history, indices, rebuild_above, optimize)

    def _moved_args(self, who, normals, rebuild_above):
        """The argument checks set_vertices and set_pose share, and the baseline of the rebuild policy, measured before the vertices
        change; returns rebuild_above as a float or None."""
        if isinstance(normals, str) and normals != "smooth":
            raise ValueError("%s: normals=%r (None, an array or \"smooth\")" % (who, normals))
        if rebuild_above is not None:
            rebuild_above = float(rebuild_above)
            if not rebuild_above > 1.0:
                raise ValueError("%s: rebuild_above=%r (None or a float > 1)" % (who, rebuild_above))
            if self.baseline is None:
                self.baseline = self.renderer.tree_cost()["sah"]
        return rebuild_above

    def _after_vertices(self, scene_buffers, normals, keep_history, indices, rebuild_above, optimize=0):
        """What follows new contents of the bound vertex buffer (set_vertices documents it): normals, refit, restart, history, policy."""
        if isinstance(normals, str):
            from . import capi
            if indices is not None and self.normals is not None:
                self.normals.close(); self.normals = None
            if self.normals is None:
                if indices is None:
                    indices = self._indices if self._indices is not None else scene_buffers.tris.read(capi.triangle_dtype)["v"]
                self.normals = capi.Normals(self.renderer, indices)
            self.normals.update()
        elif normals is not None:
            from . import capi
            props = scene_buffers.props.read(capi.tri_props_dtype)
            props["normal"] = np.asarray(normals, np.float32).reshape(-1, 3)
            scene_buffers.props.update(props)
        info = self.renderer.refit()
        self.camera.reset_accumulation()
        if keep_history and not self.motion:
            # from here on the previews go through the motion entry point.  Record sets that the plain entry point wrote carry no
            # pose and would be reprojected onto the moved surface as if it stood still: drop them once, as the default does
            if self.temporal is not None:
                self.temporal.reset()
            self.motion = True
        elif not keep_history and self.temporal is not None:
            self.temporal.reset()
        self._reset_converge()                       # the batches seen so far are of the old geometry
        if rebuild_above is None:
            return info
        cost = self.renderer.tree_cost()["sah"]                  # on the renderer's stream, behind the refit
        info = dict(info, cost=cost, baseline=self.baseline, candidate_cost=None, tree_rebuilt=False)
        if self.baseline > 0 and cost > rebuild_above * self.baseline:
            from . import capi
            try:
                nodes, tris, _, picked = self._build_candidate(scene_buffers, None, None, 4, optimize)
            except capi.GmuptError as e:
                if e.code != capi.ERR_UNSUPPORTED:
                    raise
                info["candidate_refused"] = str(e)       # a tree the builder refuses (deeper than 64 levels) is a candidate that lost
                self.baseline = cost
                return info
            info["candidate_cost"] = self.renderer.tree_cost(nodes=nodes)["sah"]
            if info["candidate_cost"] < cost:
                self._adopt(scene_buffers, nodes, tris, picked)
                info["tree_rebuilt"] = True
                self.baseline = info["candidate_cost"]
            else:
                nodes.close(); tris.close()
                self.baseline = cost
        return info

    def _build_candidate(self, scene_buffers, indices, vertex_material, max_leaf_size, optimize=0):
        """An LBVH over the device-resident vertices of `scene_buffers`, not bound yet: (nodes, tris, gmupt_lbvh_info dict, indices used).
        optimize > 0: after that many passes of the treelet optimiser."""
        from . import capi
        if indices is None:
            indices = self._indices if self._indices is not None else scene_buffers.tris.read(capi.triangle_dtype)["v"]
        if vertex_material is None:
            vertex_material = np.ascontiguousarray(scene_buffers.props.read(capi.tri_props_dtype)["materialID"])
        if self.lbvh is None:
            self.lbvh = capi.Lbvh(self.renderer.dev)
        nodes, tris, info = self.lbvh.build(scene_buffers.verts, indices, vertex_material, max_leaf_size=max_leaf_size, optimize=optimize)
        return nodes, tris, info, indices

    def _adopt(self, scene_buffers, nodes, tris, indices):
        """A freshly built tree takes the place of the bound one: a new binding is a new geometry."""
        old = (scene_buffers.nodes, scene_buffers.tris)
        scene_buffers.nodes, scene_buffers.tris = nodes, tris
        self.renderer.bind_scene(scene_buffers)      # waits for the renderer's stream before it touches anything
        for b in old:
            b.close()
        self._indices = indices
        if self.normals is not None:                 # a new triangle list needs a new adjacency
            self.normals.close(); self.normals = None
        self.camera.reset_accumulation()
        if self.temporal is not None:
            self.temporal.reset()
        self._reset_converge()

    def rebuild(self, scene_buffers, verts=None, indices=None, vertex_material=None, max_leaf_size=4, optimize=0):
        """The geometry changed beyond what a refit covers -- vertices that moved far, or another triangle list (a cut, a spawn, an LOD
        switch): upload `verts` when given (at most the vertex count the buffer was created with), build an LBVH on the GPU from the
        device-resident vertices (capi.Lbvh, gmupt_lbvh_build), put its node and triangle buffers into `scene_buffers` (the old ones are
        closed), bind, restart the accumulation and drop the temporal history: a new binding is a new geometry.
        indices: (n, 3) int32, numpy or a torch device tensor; None = the list of the last rebuild(), or, before any, the triangle
        records the scene is bound to (an SBVH's spatial splits then appear as repeated triangles).  vertex_material: per vertex; None =
        the materialID column of the property records.  optimize: N > 0 runs N passes of the treelet optimiser on the new tree before it
        is bound (capi.Lbvh.build(optimize=N); the dict then holds "optimize", the optimiser's info).  Returns the gmupt_lbvh_info dict.
        The baseline of set_vertices(rebuild_above=...) is forgotten: the next such call measures the new tree."""
        if verts is not None:
            scene_buffers.verts.update(np.ascontiguousarray(verts, np.float32))
        nodes, tris, info, indices = self._build_candidate(scene_buffers, indices, vertex_material, max_leaf_size, optimize)
        self._adopt(scene_buffers, nodes, tris, indices)
        self.baseline = None                         # of the tree that is gone
        return info

    def _reset_converge(self):
        if self.converge is not None:
            self.converge.reset()
        self._detach_plan()                          # a plan is made from the error plane of the accumulation that just ended

    def _detach_plan(self):
        if self._planned:
            self._attach_plan(None)
            self._planned = False

    def _attach_plan(self, plan):
        """A renderer with adaptive() and set_adaptive() of its own (a stand-in, a host's own class) is asked itself; capi.Renderer has
        neither method and is served by capi.adaptive."""
        if hasattr(self.renderer, "set_adaptive"):
            self.renderer.set_adaptive(plan)
        else:
            from .capi import adaptive
            adaptive.set_adaptive(self.renderer, plan)

    def _new_plan(self):
        if hasattr(self.renderer, "adaptive"):
            return self.renderer.adaptive()
        from .capi import adaptive
        return adaptive.Adaptive(self.renderer)

    def close(self):
        """Releases what the session itself created: the tree builder of rebuild(), the Normals of set_vertices(normals="smooth"), the
        history handle of denoised_temporal(), the convergence monitor of run_until() and its sampling plan."""
        self._detach_plan()
        if self.adaptive is not None:
            self.adaptive.close(); self.adaptive = None
        if self.converge is not None:
            self.converge.close(); self.converge = None
        if self.normals is not None:
            self.normals.close(); self.normals = None
        if self.lbvh is not None:
            self.lbvh.close(); self.lbvh = None
        if self.temporal is not None:
            self.temporal.close(); self.temporal = None

    def resize(self, width, height, rows=None):
        """Resolution switch (Renderer.cpp:146-150,408-413): new accumulation target, camera vectors for the new aspect, restart."""
        self.width, self.height = width, height
        self.renderer.resize(width, rows if rows is not None else height)
        self.camera.update_resolution(width, height)
        self._shutter_prev = None                    # the renderer detached the shutter: a close pose is one of the old aspect
        self._epoch += 1
        self._reset_converge()

    def pick(self, px, py):
        """What lies under whole-frame pixel (px, py) for the GUI's light / material editor: the un-jittered primary ray of the current
        camera through the renderer's closest-hit query, light spheres up to the session's lightCount included.  Returns a dict:
        triangle (reference index, -1: none), material (of that triangle), light (0, or 1 + the light sphere in front of every
        triangle), t and the world-space point origin + direction * t (None when nothing was hit)."""
        if self.projection is not None:              # the attached projection's ray, not the pinhole's
            from .capi import projection as P
            ray, hit = P.pick(self.renderer, px, py, int(self.camera.buffer.lightCount))
        else:
            ray, hit = self.renderer.pick(px, py, int(self.camera.buffer.lightCount))
        o = np.array(ray.origin[:], np.float32); d = np.array(ray.direction[:], np.float32)
        found = hit.triangle >= 0 or hit.light > 0
        return {"triangle": int(hit.triangle), "material": int(hit.material), "light": int(hit.light), "t": float(hit.t),
                "point": (o + d * np.float32(hit.t)) if found else None}

    def aovs(self, samples=1):
        """The G-buffer of the session's current camera for a denoiser or a compositor: capi.Renderer.aovs (gmupt_render_aovs), split by
        capi.aov_fields into named numpy arrays of shape (H, W) / (H, W, 3) -- albedo, normal, depth, position, roughness, metallic,
        triangle, material, light, coverage.  samples: 1..8 stratified samples per axis for the albedo / normal planes.  Like pick, it
        uses the camera the renderer was last given (the frame just drawn)."""
        from . import capi
        if self.projection is not None:              # samples^2 stratified rays of the attached projection, no centre ray
            return capi.aov_fields(capi.projection.aovs(self.renderer, samples))
        return capi.aov_fields(self.renderer.aovs(samples))

    def _guide_lens(self, lens_guides):
        """The renderer's attached lens when lens guides are asked for and one is attached, else None (the pinhole records)."""
        if not lens_guides:
            return None
        from .capi import lens as L
        lens = L.get_lens(self.renderer)
        return lens if lens.aperture_radius > 0 else None

    def denoised(self, aov_samples=1, infill=False, lens_guides=False, **params):
        """A clean preview of the session's current frame: capi.Renderer.denoise (gmupt_render_denoised) as an (H, W, 4) float32 numpy
        array -- rgb denoised, alpha the sample-count bits -- so to_rgba8 and the frame writers take it as they take a preview.  On a
        tile renderer it is this rank's tile, denoised on its own (tile edges are image edges).  params: the gmupt_denoise_params fields.
        infill: True, or a dict of capi.infill_params fields -- surface pixels without a sample take a colour from the sampled pixels of
        their surface before the filter runs (capi.Renderer.preview, gmupt_render_preview); False keeps today's bits.
        lens_guides: True with a lens attached (set_lens) -- the guide records are the lens-filtered ones (capi.lens_aov,
        include/gmupt_lens_aov.h: aov_samples^2 rays per pixel through the lens), so that out-of-focus silhouettes are filtered like
        the beauty shows them; without a lens, or False (the default), the pinhole records and today's bits."""
        if self.projection is not None:              # the guides follow the projection; the infill takes its records as they are
            from . import capi
            if infill is None or infill is False:
                return capi.projection.denoise(self.renderer, aov_samples, **params).cpu().numpy()
            beauty, aov = capi.projection.guided_inputs(self.renderer, aov_samples)
            filled = capi.infill_image(self.renderer, beauty, aov, **(infill if isinstance(infill, dict) else {}))
            return capi.denoise_image(self.renderer, filled, aov, **params).cpu().numpy()
        lens = self._guide_lens(lens_guides)
        if lens is not None:
            from . import capi
            if infill is None or infill is False:
                return capi.lens_aov.denoise(self.renderer, aov_samples, **params).cpu().numpy()
            beauty, aov = capi.lens_aov.guided_inputs(self.renderer, aov_samples)
            filled = capi.infill_image(self.renderer, beauty, aov, **(infill if isinstance(infill, dict) else {}))
            return capi.denoise_image(self.renderer, filled, aov, **params).cpu().numpy()
        if infill is not None and infill is not False:
            return self.renderer.preview(aov_samples=aov_samples, infill=infill, **params).cpu().numpy()
        return self.renderer.denoise(aov_samples, **params).cpu().numpy()

    def denoised_temporal(self, aov_samples=1, infill=False, lens_guides=False, **params):
        """A preview that survives camera motion: capi.Renderer.denoise_temporal (gmupt_render_denoised_temporal) with a history handle the
        session owns, as an (H, W, 4) float32 numpy array -- rgb denoised, alpha the effective sample-count bits.  Pixels the new
        accumulation has not reached yet show the reprojected history of the frames before the restart.  set_lights drops the history;
        resize keeps it.  On a tile renderer each rank keeps its own tile's history.  params: the capi.temporal_params fields.
        infill: as denoised() -- the pixels without a sample that have no consistent history either (first frame, light edit,
        disocclusion) are filled after the integration; filled colour never enters the history.  False keeps today's bits.
        lens_guides: as denoised() -- with a lens attached the lens records and a copy of the frame go through
        capi.temporal_denoise_image (gmupt_temporal_denoise_image) on the same handle; the history folds when a frame of this session
        has cleared the target, or a resize happened, since the last such call.  The projection reprojects the record's position, with
        lens records a mean over the surface samples, and the motion plane stays a pinhole's and is not used on this path; one
        history should be fed by one kind of record."""
        self._no_projection("denoised_temporal")
        if self.temporal is None:
            from . import capi
            self.temporal = capi.Temporal(self.renderer)
        lens = self._guide_lens(lens_guides)
        if lens is not None:
            from . import capi
            beauty, aov = capi.lens_aov.guided_inputs(self.renderer, aov_samples)
            fold = self._guided_epoch is None or self._guided_epoch != self._epoch
            d = getattr(self.renderer, "desc", None)
            origin = (int(d.tile_x0), int(d.tile_y0)) if d is not None and d.tile_enabled else (0, 0)
            out = capi.temporal_denoise_image(self.temporal, beauty, aov, self.camera.buffer, fold, origin=origin,
                                              infill=infill if infill is not None and infill is not False else None, **params)
            self._guided_epoch = self._epoch
            return out.cpu().numpy()
        if infill is not None and infill is not False:
            return self.renderer.preview(self.temporal, motion=self.motion, aov_samples=aov_samples, infill=infill, **params).cpu().numpy()
        call = self.renderer.denoise_temporal_motion if self.motion else self.renderer.denoise_temporal
        return call(self.temporal, aov_samples, **params).cpu().numpy()

    # ---- frames
    def frame(self, dt=0.0):
        self.camera.update(dt)                       # Renderer::update: camera vectors, iterationCounter, randomSeed
        if getattr(getattr(self.camera, "buffer", None), "iterationCounter", 1) == 0:
            self._epoch += 1                         # this frame clears the target: a new accumulation
            if self._planned:
                self._detach_plan()                  # the restarted frame has no error plane yet
        if self._shutter_fraction is not None:
            self._follow_shutter()
        self.renderer.set_camera(self.camera.buffer)
        self.renderer.iterate()                      # Renderer::draw
        self.frames += 1
        if self.preview_every and self.frames % self.preview_every == 0:
            return self.preview()
        return None

    def run(self, frames, dt=0.0):
        last = None
        for _ in range(frames):
            out = self.frame(dt)
            last = out if out is not None else last
        return last

    def run_until(self, threshold, check_every=8, max_frames=4096, min_batches=2, allow_pixels=0, dt=0.0, adaptive=False, max_repeat=1,
                  uniform_every=0):
        """Frames until the image is done: after every `check_every` frames the session's convergence monitor (capi.Converge,
        include/gmupt.h "Convergence", created on first use and kept until close()) estimates the standard error of every pixel's
        tone-mapped luminance mean, and the loop ends at the first check at which all but `allow_pixels` pixels have seen
        `min_batches` batches and lie at or below `threshold` (display units: 1 / 255 is one 8-bit step) -- or after max_frames.
        Returns the last check's info dict with "frames", the frames this call ran, added (no check ran: only "frames" and
        converged = False).  Light, geometry and resolution events reset the monitor as they reset the temporal history.
        With dist and world > 1 every rank judges its own tile, and the ranks agree through one all_reduce (MAX of "not converged")
        per check, so that all of them leave in the same frame: a rank that stopped alone would hang the next tile gather.  The
        returned `converged` is the agreed one; the other fields are this rank's.
        The monitor comes from renderer.converge() (capi.Renderer has it; a stand-in returns anything with update(**params), reset()
        and close()).
        adaptive=True: after every check that does not end the loop the monitor's error plane becomes a sampling plan (capi.adaptive.Adaptive,
        include/gmupt_adaptive.h, created on first use and kept until close()): the next frames send their new camera
        paths to the pixels still above `threshold`, up to `max_repeat` entries each, every `uniform_every`-th path (0 = none) to
        the pixel it would have gone to anyway.  The info dict then holds "plan", the last selection's summary.  A converged return
        detaches the plan.  A return at max_frames leaves it attached -- the image is not done, and frame() and run() go on sampling
        by it -- until an event that resets the monitor, a frame that clears the target, or a run_until without `adaptive` detaches it.  With world > 1 each rank plans its own tile.
        The plan is a capi.adaptive.Adaptive of the renderer, attached with capi.adaptive.set_adaptive; a renderer that has adaptive()
        and set_adaptive(plan) itself is asked instead (a stand-in returns anything with select(error, **params) and close()), and the
        monitor's update(error=True, **params) returns (info, error plane)."""
        if check_every < 1:
            raise ValueError("run_until: check_every=%r (at least 1)" % (check_every,))
        if self.converge is None:
            self.converge = self.renderer.converge()
        if not adaptive:
            self._detach_plan()                      # of an earlier adaptive call
        elif self.adaptive is None:
            self.adaptive = self._new_plan()
        info = {"converged": False}
        plan = None
        ran = 0
        while ran < max_frames:
            self.frame(dt)
            ran += 1
            if ran % check_every:
                continue
            if adaptive:
                info, error = self.converge.update(error=True, threshold=threshold, min_batches=min_batches, allow_pixels=allow_pixels)
                info = dict(info)
            else:
                info = dict(self.converge.update(threshold=threshold, min_batches=min_batches, allow_pixels=allow_pixels))
            if self.dist is not None and self.world > 1:
                import torch
                flag = torch.tensor([0 if info["converged"] else 1], dtype=torch.int32)
                if self.dist.get_backend() == "nccl":
                    flag = flag.cuda()
                self.dist.all_reduce(flag, op=self.dist.ReduceOp.MAX)
                info["converged"] = int(flag.item()) == 0
            if info["converged"]:
                self._detach_plan()                  # the image is done: later frames are plain ones
                break
            if adaptive:
                plan = self.adaptive.select(error, threshold=threshold, max_repeat=max_repeat, uniform_every=uniform_every)
                self._attach_plan(self.adaptive)
                self._planned = True
        if plan is not None:
            info["plan"] = plan
        info["frames"] = ran
        return info

    def preview(self):
        """Gathers the tiles; rank 0 gets the assembled float frame (and calls on_preview), the other ranks None."""
        import torch
        local = torch.from_numpy(np.ascontiguousarray(self.renderer.framebuffer()))
        if self.dist is not None and self.world > 1 and self.dist.get_backend() == "nccl":
            local = local.cuda()
        frame = tiles.gather_tiles(local, self.width, self.height, self.rank, self.world, self.dist if self.world > 1 else None)
        frame = frame.cpu().numpy() if frame is not None else None
        self.previews += 1
        if frame is not None and self.on_preview is not None:
            self.on_preview(self.frames, frame)
        return frame
