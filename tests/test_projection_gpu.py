"""GPU tests of the camera projections (include/gmupt_projection.h; csrc/pt_projection.hip): k_proj_retarget against its host rule bit
for bit at the sizes at which it can go wrong, whole iterations against a renderer whose fresh slots are patched on the host between
the shipped stages, attach / detach and the life cycle, the lens x projection refusal, the records of gmupt_render_aovs_projected
against the oracle's per-ray shading, three checks of the picture from the records alone, picking, the denoiser and the session.
The method and the shapes are test_lens_gpu.py's: Cornell at 32 x 18 with a pool of 4096."""
import ctypes as C
import math

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import adaptive_util as AU
import lens_aov_util as LA
import lens_util as LU
import projection_util as PU
from test_aov_gpu import compare_records, oracle_rays, per_ray, pixels

pytestmark = pytest.mark.gpu

W, H, POOL = 32, 18, 4096
RECT = (7, 5, 11, 6)
F = np.float32


@pytest.fixture(params=["wide", "cast0"])
def shipped_kernel(request, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", request.param)
    return request.param


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


def make(pkg, device, scene, tile=None, budget=0, pool=POOL, live=0, size=(W, H)):
    """tile: (x0, y0, w, h) of a tile renderer of the frame."""
    sb = pkg.capi.SceneBuffers(device, scene)
    if tile is None:
        r = pkg.capi.Renderer(device, size[0], size[1], pool_paths=pool, live_paths=live, path_budget=budget)
    else:
        r = pkg.capi.Renderer(device, tile[2], tile[3], pool_paths=pool, live_paths=live, tile=(tile[0], tile[1]), path_budget=budget)
    r.bind_scene(sb)
    cam = pkg.capi.Camera(*size); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return r, sb, cam


def close(*things):
    for t in things:
        t.close()


def step(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()


def snapshot(r):
    r.synchronize()
    return r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters()


def same(a, b):
    return np.array_equal(LU.bits(a[0]), LU.bits(b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def host_rays(pkg, cb, proj, raw, pool, q, slots):
    """gmupt_projection_ray_host of the fresh slots: their queue indices and the screen coordinates the state holds."""
    xy = LU.state_screen(raw, pool)[slots]
    return pkg.capi.projection.projection_rays_host(cb, proj, q, xy[:, 0], xy[:, 1])


def kinds(pkg):
    p = PU.projections(pkg.capi)
    return {"ortho": p["ortho"], "fisheye": p["fisheye180"], "equirect": p["equirect"]}


# name: (make() arguments, iterations before the stage, render the budget out first, attach the identity plan, what the fresh count must look like)
STAGE_CASES = {
    "first_stage_16_blocks": (dict(), 0, False, False, lambda n: n == POOL),
    "live_3000_of_4096": (dict(live=3000), 0, False, False, lambda n: n == 3000 and n % 256),
    "fourth_iteration_ragged": (dict(), 3, False, False, lambda n: 0 < n < POOL and n % 256),
    "budget_retires_part": (dict(budget=2500), 0, False, False, lambda n: n == POOL),
    "nothing_ended": (dict(budget=1000), 0, True, False, lambda n: n == 0),
    "tile_origin_7_5": (dict(tile=RECT, pool=1024), 0, False, False, lambda n: n == 1024),
    "identity_plan": (dict(), 0, False, True, lambda n: n == POOL),
}


@pytest.mark.parametrize("kind", ["ortho", "fisheye", "equirect"])
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_stage_equals_the_host_rule(pkg, device, wide, cornell_scene, case, kind):
    kw, before, render_out, planned, count_ok = STAGE_CASES[case]
    pool, live, budget = kw.get("pool", POOL), kw.get("live", 0) or kw.get("pool", POOL), kw.get("budget", 0)
    proj = kinds(pkg)[kind]
    runs = []
    for attached in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene, **kw)
        plan = None
        if planned:
            plan = pkg.capi.adaptive.Adaptive(r)
            plan.set_list(AU.rect_list(W, 0, 0, W, H), W, H)
            pkg.capi.adaptive.set_adaptive(r, plan)
        if render_out:
            r.render_budget(cam)
        step(r, cam, before)
        if attached:
            pkg.capi.projection.set_projection(r, proj)
        cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(pkg.capi.STAGE_SHADE)
        runs.append(snapshot(r) + (cam.buffer_copy(),))
        if plan is not None:
            pkg.capi.adaptive.set_adaptive(r, None); plan.close()
        close(r, sb, cam)
    plain, projected = runs
    qc = projected[3]
    n_new = min(int(qc[0]), live)
    q, slots = LU.fresh(qc, projected[2], live, budget)
    print("%s %s: new-path count %d, fresh after the guards %d, lastPathCnt %d" % (case, kind, n_new, q.size, int(qc[1])))
    assert count_ok(n_new), n_new
    if case == "budget_retires_part":
        assert q.size == 2500 and slots.size < n_new
    if case == "tile_origin_7_5":
        xy = LU.state_screen(projected[1], pool)[slots]
        assert xy[:, 0].min() == 7 and xy[:, 1].min() == 5 and xy[:, 0].max() == 17 and xy[:, 1].max() == 10
    assert np.array_equal(LU.bits(plain[0]), LU.bits(projected[0])) and np.array_equal(plain[2], projected[2]) and np.array_equal(plain[3], projected[3])
    want = LU.patch_rays(plain[1], pool, slots, host_rays(pkg, projected[4], proj, plain[1], pool, q, slots)) if q.size else plain[1]
    assert np.array_equal(want, projected[1]), "fresh slots hold the host rule's ray; every other word is the run without a projection"
    if q.size:
        assert not np.array_equal(plain[1], projected[1]), "the rays did change"


@pytest.mark.parametrize("tile", [None, (4, 3, 40, 24)], ids=["frame", "tile"])
def test_whole_iterations_equal_the_patched_stages(pkg, device, shipped_kernel, cornell_scene, tile):
    """A: a fisheye attached, gmupt_iterate.  B: none; per iteration the shipped shading stage, the host rule patched into the fresh
    slots through the debug access, the shipped ray casts.  Equal after 1, 2 and 24 iterations in every word.  64 x 36, so that
    pixels outside the image circle are in the frame (and in the tile)."""
    capi = pkg.capi
    size = (64, 36)
    pool = POOL if tile is None else 1024
    proj = kinds(pkg)["fisheye"]
    a, sba, cama = make(pkg, device, cornell_scene, tile=tile, pool=pool, size=size)
    b, sbb, camb = make(pkg, device, cornell_scene, tile=tile, pool=pool, size=size)
    capi.projection.set_projection(a, proj)
    moved = outside = 0
    for it in range(1, 25):
        step(a, cama, 1)
        camb.update(0.0); b.set_camera(camb.buffer); b.run_stage(capi.STAGE_SHADE)
        raw, queues, qc = b.read_path_state(), b.read_queues(), b.counters()
        q, slots = LU.fresh(qc, queues, pool)
        if q.size:
            rays = host_rays(pkg, camb.buffer_copy(), proj, raw, pool, q, slots)
            outside += int((np.abs(rays[:, 4:7]).max(axis=1) == 0).sum())
            b.write_path_state(LU.patch_rays(raw, pool, slots, rays))
            moved += q.size
        b.run_stage(capi.STAGE_RAYCASTS)
        if it in (1, 2, 24):
            assert same(snapshot(a), snapshot(b)), "iteration %d" % it
    fb = a.framebuffer()
    assert moved > pool and outside > 0 and int(fb[..., 3].view(np.uint32).sum()) > 0 and np.isfinite(fb[..., :3]).all()
    assert a.stats().flags & (capi.STAT_STACK_OVERFLOW | capi.STAT_CAST_ABORTED) == 0, "a zero direction raises no fault flag"
    close(a, sba, cama, b, sbb, camb)


def test_attach_detach_life_cycle_and_refusals(pkg, device, shipped_kernel, cornell_scene):
    capi = pkg.capi
    P, L = capi.projection, capi.lens
    lib = capi.lib()

    def run(prepare):
        r, sb, cam = make(pkg, device, cornell_scene)
        prepare(r)
        step(r, cam, 12)
        out = snapshot(r)
        close(r, sb, cam)
        return out

    def attach_and_detach(r):
        P.set_projection(r, P.fisheye(180.0))
        P.set_projection(r, None)

    def attach_and_pinhole(r):
        P.set_projection(r, P.equirect())
        P.set_projection(r, P.projection_params(P.PINHOLE, fov=float("nan")))     # the pinhole kind detaches whatever the fields say

    plain = run(lambda r: None)
    assert int(plain[0][..., 3].view(np.uint32).sum()) > 0
    for prepare in (lambda r: P.set_projection(r, None), attach_and_detach, attach_and_pinhole):
        assert same(plain, run(prepare))
    assert not same(plain, run(lambda r: P.set_projection(r, P.equirect()))), "a projection does change the frame"
    # the value round-trips and survives gmupt_resize and gmupt_set_camera
    r, sb, cam = make(pkg, device, cornell_scene)
    d = P.get_projection(r)
    assert (d.kind, d.fov, d.extent, d.pad) == (P.PINHOLE, F(3.14159274), 1.0, 0)
    proj = P.projection_params(P.FISHEYE, fov=2.5, extent=7.0)
    P.set_projection(r, proj)
    tup = lambda p: (p.kind, p.fov, p.extent, p.pad)
    assert tup(P.get_projection(r)) == (P.FISHEYE, 2.5, 7.0, 0)
    step(r, cam, 2)
    r.resize(24, 12); cam.update_resolution(24, 12)
    step(r, cam, 2)
    assert tup(P.get_projection(r)) == (P.FISHEYE, 2.5, 7.0, 0), "the projection survives gmupt_resize and gmupt_set_camera"
    cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(capi.STAGE_SHADE)      # and it is still launched, at the new size
    _, raw, queues, qc = snapshot(r)
    q, slots = LU.fresh(qc, queues, POOL)
    rays = host_rays(pkg, cam.buffer_copy(), proj, raw, POOL, q, slots)
    o, dd = LU.state_rays(raw, POOL)
    assert q.size > 0 and np.array_equal(LU.bits(o[slots]), LU.bits(rays[:, 0:3])) and np.array_equal(LU.bits(dd[slots]), LU.bits(rays[:, 4:7]))
    # a bad projection leaves the attached one
    bad = P.projection_params(P.FISHEYE, fov=-1.0)
    assert lib.gmupt_renderer_set_projection(r.h, C.byref(bad)) == capi.ERR_INVALID_ARGUMENT and b"gmupt_renderer_set_projection" in lib.gmupt_last_error()
    assert lib.gmupt_renderer_get_projection(r.h, None) == capi.ERR_INVALID_ARGUMENT
    assert tup(P.get_projection(r)) == (P.FISHEYE, 2.5, 7.0, 0)
    # lens and projection do not combine, in both directions
    open_lens = L.lens_params(aperture_radius=0.3, focus_distance=13.0)
    assert lib.gmupt_renderer_set_lens(r.h, C.byref(open_lens)) == capi.ERR_UNSUPPORTED and b"do not combine" in lib.gmupt_last_error()
    assert L.get_lens(r).aperture_radius == 0.0
    L.set_lens(r, L.lens_params(aperture_radius=0.0, focus_distance=2.0))            # no aperture: nothing to refuse
    P.set_projection(r, None)
    L.set_lens(r, open_lens)                                                         # no projection attached: as before
    assert L.get_lens(r).aperture_radius == F(0.3)
    fish = P.fisheye(180.0)
    assert lib.gmupt_renderer_set_projection(r.h, C.byref(fish)) == capi.ERR_UNSUPPORTED and b"do not combine" in lib.gmupt_last_error()
    assert P.get_projection(r).kind == P.PINHOLE
    P.set_projection(r, P.projection_params(P.PINHOLE))                              # the pinhole is no projection: accepted
    L.set_lens(r, None)
    P.set_projection(r, fish)
    assert P.get_projection(r).kind == P.FISHEYE
    close(r, sb, cam)


# ---------------------------------------------------------------------------------------------------- AOV records
ENV = (0.1, 0.3, 0.6)


def aov_camera(pkg, scene, Wc, Hc, pose=None, lights=None):
    cam = pkg.capi.Camera(Wc, Hc)
    cam.set_pose(*(pose or scene["camera"])); cam.buffer.lightCount = scene["light_count"] if lights is None else lights; cam.update(0.0)
    for i, v in enumerate(ENV):
        cam.buffer.envColor[i] = v
    return cam


@pytest.fixture(scope="module")
def textured(pkg):
    return pkg.scenes.build_scene(pkg.scenes.textured_mesh())


@pytest.mark.parametrize("kind", ["ortho", "fisheye", "equirect"])
@pytest.mark.parametrize("size, s", [((16, 8), 1), ((16, 8), 2), ((16, 8), 3), ((33, 17), 1), ((33, 17), 2), ((33, 17), 3)])
def test_records_match_the_oracle(pkg, device, wide, textured, kind, size, s):
    """The rays k_paov_raygen wrote, read back from the chunk scratch (gmupt_debug_read_aov_rays; the frame is one chunk), are bit for
    bit gmupt_aov_projected_ray's in all eight words, and the records are the oracle's per-ray shading of exactly those rays under the
    stated sums."""
    scene = textured
    Wc, Hc = size
    proj = kinds(pkg)[kind]
    cam = aov_camera(pkg, scene, Wc, Hc)
    xs, ys = pixels(Wc, Hc)
    rays = pkg.capi.projection.aov_projected_rays(cam.buffer, proj, xs, ys, s)
    truth = oracle_rays(scene, rays.reshape(-1, 8), cam.buffer)
    v = per_ray(scene, rays.reshape(-1, 8), truth, cam.buffer)
    exp, rec, names = LA.reduce_records(v, rays)
    assert v["surface"].any()
    if kind == "fisheye":
        assert (np.abs(rays[..., 4:7]).max(axis=-1) == 0).any() and not v["surface"].all(), "pixels outside the image circle"
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    lib = pkg.capi.lib()
    probe = np.zeros((1, 8), F)
    assert lib.gmupt_debug_read_aov_rays(r.h, probe.ctypes.data_as(C.c_void_p), 1) == pkg.capi.ERR_NOT_BOUND, "no AOV call yet"
    info = pkg.capi.TraceInfo()
    got = pkg.capi.projection.aovs(r, s, proj, info=info)
    on_device = pkg.capi.projection.read_aov_rays(r, Wc * Hc * s * s)
    assert np.array_equal(LU.bits(on_device), LU.bits(rays.reshape(-1, 8))), "k_paov_raygen wrote the host rule's rays: origin, tmax, direction, pad"
    assert lib.gmupt_debug_read_aov_rays(r.h, None, 1) == pkg.capi.ERR_INVALID_ARGUMENT and lib.gmupt_debug_read_aov_rays(None, probe.ctypes.data_as(C.c_void_p), 1) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_debug_read_aov_rays(r.h, probe.ctypes.data_as(C.c_void_p), pkg.capi.AOV_CHUNK_RAYS + 1) == pkg.capi.ERR_INVALID_ARGUMENT
    assert got.shape == (Hc, Wc, 16) and got.dtype == torch.float32 and got.is_cuda and info.flags & pkg.capi.STAT_CAST_WIDE
    compare_records(scene, got.cpu().numpy(), exp, rec, names)
    # NULL is the attached projection
    pkg.capi.projection.set_projection(r, proj)
    assert np.array_equal(LU.bits(pkg.capi.projection.aovs(r, s).cpu().numpy()), LU.bits(got.cpu().numpy()))
    close(r, sb, cam)


def test_tile_renderer_returns_its_sub_rectangle(pkg, device, wide, textured):
    Wc, Hc = 33, 17
    cam = aov_camera(pkg, textured, Wc, Hc)
    sb = pkg.capi.SceneBuffers(device, textured)
    r = pkg.capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    x0, y0, tw, th = 7, 5, 11, 6
    rt = pkg.capi.Renderer(device, tw, th, pool_paths=POOL, tile=(x0, y0))
    rt.bind_scene(sb); rt.set_camera(cam.buffer)
    for kind, proj in kinds(pkg).items():
        for s in (1, 2):
            whole = LU.bits(pkg.capi.projection.aovs(r, s, proj).cpu().numpy())
            tile = LU.bits(pkg.capi.projection.aovs(rt, s, proj).cpu().numpy())
            assert tile.shape == (th, tw, 16) and np.array_equal(tile, whole[y0:y0 + th, x0:x0 + tw]), (kind, s)
    close(rt, r, sb, cam)


def test_a_frame_of_two_chunks_equals_single_chunk_tiles(pkg, device, wide, textured):
    """test_lens_aov_gpu's chunk seam under a projection: the three paths run one chunk loop.  On the CPU oracle this frame (the textured
    scene from its own camera under the 180-degree fisheye) has 5988 pixels with coverage > 0 of the 13495 that have a ray inside the
    image circle."""
    s = pkg.capi.AOV_MAX_SAMPLES
    Wc = 256
    rows = pkg.capi.AOV_CHUNK_RAYS // (Wc * s * s)           # 128 rows of 256 * 64 rays fill a chunk
    Hc = rows + 1                                            # one more: a second chunk of one row
    assert rows * Wc * s * s == pkg.capi.AOV_CHUNK_RAYS and Wc * Hc * s * s > pkg.capi.AOV_CHUNK_RAYS
    proj = kinds(pkg)["fisheye"]
    cam = aov_camera(pkg, textured, Wc, Hc)
    sb = pkg.capi.SceneBuffers(device, textured)
    r = pkg.capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    whole = pkg.capi.projection.aovs(r, s, proj).cpu().numpy().view(np.uint32)
    assert (pkg.capi.aov_fields(whole.view(np.float32))["coverage"] > 0).sum() > 1000
    for y0, th in [(0, 64), (64, 64), (rows, 1)]:            # the last tile is the second chunk's row
        rt = pkg.capi.Renderer(device, Wc, th, pool_paths=POOL, tile=(0, y0))
        rt.bind_scene(sb); rt.set_camera(cam.buffer)
        assert np.array_equal(pkg.capi.projection.aovs(rt, s, proj).cpu().numpy().view(np.uint32), whole[y0:y0 + th]), y0
        rt.close()
    close(r, sb, cam)


def custom_scene(pkg, verts, normals, indices):
    mesh = dict(pkg.scenes.cornell_mesh())
    mesh.update(verts=np.asarray(verts, np.float32), normals=np.asarray(normals, np.float32), indices=np.asarray(indices, np.int32),
                vertex_material=np.zeros(len(verts), np.uint32))
    return pkg.scenes.build_scene(mesh)


def test_orthographic_quads_at_two_depths_cover_the_same_pixels(pkg, device, wide):
    """Two equal axis-aligned squares of side 2 facing the camera, at depths 9 and 12.  Under the orthographic projection both cover the
    pixels whose ray origin -- a lattice of pitch p = extent / H -- lies in a square of side a = 2 / p pixels; an interval of length a
    holds floor(a) or floor(a) + 1 lattice points, so both counts lie in [n^2, (n + 1)^2] with n = floor(a), and they differ by at most
    2 n + 1 <= perimeter / 2 + 1 pixels.  Under the pinhole the nearer one is (12 / 9)^2 times larger."""
    capi = pkg.capi
    quad = lambda cx, cy, z: [(cx - 1, cy - 1, z), (cx + 1, cy - 1, z), (cx + 1, cy + 1, z), (cx - 1, cy + 1, z)]
    verts = quad(-1.53, 3.07, -1.0) + quad(1.91, 3.39, -4.0)
    scene = custom_scene(pkg, verts, [(0, 0, 1)] * 8, [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)])
    Wc, Hc, E = 64, 36, 8.0
    cam = aov_camera(pkg, scene, Wc, Hc, pose=(0.0, 3.0, 8.0, 0.0, 270.0), lights=0)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    f = capi.aov_fields(capi.projection.aovs(r, 1, capi.projection.orthographic(E)))
    surf = f["triangle"] >= 0
    near, far = surf & (f["position"][..., 2] > -2.5), surf & (f["position"][..., 2] < -2.5)
    a = 2.0 / (E / Hc)
    n = math.floor(a)
    print("orthographic: %d and %d pixels, side %.2f px, bound %d" % (near.sum(), far.sum(), a, 2 * n + 1))
    assert n * n <= near.sum() <= (n + 1) ** 2 and n * n <= far.sum() <= (n + 1) ** 2
    assert abs(int(near.sum()) - int(far.sum())) <= 2 * n + 1 <= 4 * a / 2 + 1
    assert np.abs(f["depth"][near] - 9.0).max() < 1e-4 and np.abs(f["depth"][far] - 12.0).max() < 1e-4, "depth is the distance from the ray's own origin"
    g = capi.aov_fields(r.aovs(1))
    pn, pf = (g["triangle"] >= 0) & (g["position"][..., 2] > -2.5), (g["triangle"] >= 0) & (g["position"][..., 2] < -2.5)
    assert pn.sum() > 1.5 * pf.sum() > 0, "the pinhole shows them at different sizes"
    close(r, sb, cam)


@pytest.fixture(scope="module")
def sphere(pkg):
    """A subdivided icosphere of radius 4 around (0, 3, 0), seen from its centre."""
    v, tris = pkg.scenes.icosphere(2)
    centre, R = np.array([0.0, 3.0, 0.0]), 4.0
    verts = (v * R + centre).astype(np.float32)
    scene = custom_scene(pkg, verts, v, tris)
    w = verts.astype(np.float64) - centre
    a, b, c = w[tris[:, 0]], w[tris[:, 1]], w[tris[:, 2]]
    nrm = np.cross(b - a, c - a)
    plane = np.abs((nrm * a).sum(axis=1)) / np.linalg.norm(nrm, axis=1)
    return scene, centre, float(plane.min()), float(np.linalg.norm(w, axis=1).max())


def test_equirect_inside_a_sphere_sees_surface_everywhere(pkg, device, wide, sphere):
    scene, centre, lo, hi = sphere
    capi = pkg.capi
    Wc, Hc = 64, 32
    cam = aov_camera(pkg, scene, Wc, Hc, pose=(centre[0], centre[1], centre[2], 10.0, 200.0), lights=0)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    f = capi.aov_fields(capi.projection.aovs(r, 1, capi.projection.equirect()))
    eps = 16 * 2.0 ** -23 * hi      # t of one ray: a dozen binary32 operations on lengths <= the radius
    print("equirect: depth %.6f .. %.6f, plane distance %.6f, circumradius %.6f" % (f["depth"].min(), f["depth"].max(), lo, hi))
    assert (f["triangle"] >= 0).all() and (f["coverage"] == 1).all() and (f["light"] == 0).all()
    assert lo < hi and f["depth"].min() >= lo - eps and f["depth"].max() <= hi + eps
    assert len(np.unique(f["triangle"])) > 100, "the panorama sees all around"
    close(r, sb, cam)


def test_fisheye_inside_a_sphere_misses_exactly_outside_the_circle(pkg, device, wide, oracle, sphere):
    scene, centre, lo, hi = sphere
    capi = pkg.capi
    Wc, Hc = 48, 30
    cam = aov_camera(pkg, scene, Wc, Hc, pose=(centre[0], centre[1], centre[2], -5.0, 30.0), lights=0)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, Wc, Hc, pool_paths=POOL)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    proj = capi.projection.projection_params(capi.projection.FISHEYE, fov=2 * math.pi)
    f = capi.aov_fields(capi.projection.aovs(r, 1, proj))
    ys, xs = np.mgrid[0:Hc, 0:Wc]
    _, d = PU.rule_pixel(oracle, cam.buffer, proj, xs.astype(F), ys.astype(F))
    outside = np.abs(d).max(axis=-1) == 0                    # r > 1 of the restated rule
    miss = (f["triangle"] < 0) & (f["light"] == 0)
    env = (LU.bits(f["albedo"]) == LU.bits(np.array(ENV, F))).all(axis=-1)
    assert outside.any() and (~outside).any() and np.array_equal(miss, outside) and np.array_equal(miss & env, outside)
    assert (f["coverage"][outside] == 0).all() and (f["coverage"][~outside] == 1).all() and not LU.bits(f["position"][outside]).any()
    close(r, sb, cam)


# ---------------------------------------------------------------------------------------------------- picking, denoiser, session
def test_pick_projected_is_trace_rays_on_the_pick_ray(pkg, device, wide, cornell_scene):
    capi = pkg.capi
    P = capi.projection
    r, sb, cam = make(pkg, device, cornell_scene)
    cam.update(0.0); r.set_camera(cam.buffer)
    cb = cam.buffer_copy()
    for kind, proj in list(kinds(pkg).items()) + [("pinhole", None)]:
        P.set_projection(r, proj)
        for px, py in [(18.0, 4.0), (3.25, 9.5), (0.0, 0.0), (16.0, 9.0)]:
            ray, hit = P.pick(r, px, py, cornell_scene["light_count"])
            want = P.pick_ray(cb, proj if proj is not None else P.projection_params(P.PINHOLE), px, py)
            assert bytes(ray) == bytes(want), (kind, px, py)
            hits, _ = r.trace(closest=np.frombuffer(bytes(want), F).reshape(1, 8).copy(), light_count=cornell_scene["light_count"])
            assert np.array_equal(np.frombuffer(bytes(hit), np.uint32), LU.bits(hits).reshape(-1)), (kind, px, py)
        if proj is None:
            ray, hit = P.pick(r, 18.0, 4.0, 0)
            ray2, hit2 = r.pick(18.0, 4.0, 0)
            assert bytes(ray) == bytes(ray2) and bytes(hit) == bytes(hit2), "nothing attached: gmupt_pick"
    close(r, sb, cam)


def test_denoised_projected_is_the_host_denoiser_on_the_projected_records(pkg, device, wide, cornell_scene):
    capi = pkg.capi
    P = capi.projection
    r, sb, cam = make(pkg, device, cornell_scene)
    proj = kinds(pkg)["fisheye"]
    P.set_projection(r, proj)
    step(r, cam, 6)
    got = P.denoise(r, 2).cpu().numpy()
    aov = P.aovs(r, 2).cpu().numpy()
    want = capi.denoise_host(r.framebuffer(), aov)
    assert got.shape == (H, W, 4) and np.array_equal(LU.bits(got), LU.bits(np.asarray(want, F)))
    pin = r.denoise(2).cpu().numpy()
    assert not np.array_equal(LU.bits(got), LU.bits(pin)), "pinhole guides are another picture"
    close(r, sb, cam)


def test_session_routes_through_the_projected_calls(pkg, device, wide, cornell_scene):
    capi = pkg.capi
    P = capi.projection
    r, sb, cam = make(pkg, device, cornell_scene)
    s = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    s.run(4)
    before = int(r.framebuffer()[..., 3].view(np.uint32).max())
    proj = s.set_projection("equirect")
    assert proj.kind == P.EQUIRECT and P.get_projection(r).kind == P.EQUIRECT
    s.run(1)
    r.synchronize()
    assert cam.buffer.iterationCounter == 0, "the frame after set_projection clears the target"
    s.run(2)
    assert before > 0 and int(r.framebuffer()[..., 3].view(np.uint32).max()) > 0
    got = s.pick(18, 4)
    ray, hit = P.pick(r, 18, 4, int(cam.buffer.lightCount))
    assert got["triangle"] == hit.triangle and got["t"] == hit.t and np.array_equal(got["point"], np.array(ray.origin[:], F) + np.array(ray.direction[:], F) * F(hit.t))
    a = s.aovs(2)
    assert np.array_equal(LU.bits(a["depth"]), LU.bits(capi.aov_fields(P.aovs(r, 2))["depth"]))
    assert not np.array_equal(LU.bits(a["depth"]), LU.bits(capi.aov_fields(r.aovs(2))["depth"]))
    assert np.array_equal(LU.bits(s.denoised(2)), LU.bits(P.denoise(r, 2).cpu().numpy()))
    filled = s.denoised(1, infill=True)
    assert filled.shape == (H, W, 4) and np.isfinite(filled[..., :3]).all()
    for refused in (lambda: s.denoised_temporal(), lambda: s.set_lens(0.3, focus=13.0), lambda: s.set_vertices(sb, None, keep_history=True),
                    lambda: s.set_pose(sb, None, None, keep_history=True)):
        with pytest.raises(ValueError, match="projection"):
            refused()
    assert s.set_projection(None) is None and P.get_projection(r).kind == P.PINHOLE
    s.run(2)
    assert s.denoised_temporal().shape == (H, W, 4)
    s.close()
    close(r, sb, cam)
