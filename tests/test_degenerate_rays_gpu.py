"""GPU tests of the ray casts on degenerate rays: NaN, infinite, signed-zero, denormal, huge and tiny components, odd tmax, tiny batches.

include/gmupt.h (gmupt_trace_rays, "Degenerate rays") states what such rays get; every sentence there is asserted here, bit for bit
against the CPU oracle (trace_util.oracle_truth) wherever the oracle has the stage, and by the header's own derivation for the tmax of
closest-hit rays (trace_util.expected_closest_with_tmax).  The rays come from trace_util.degenerate_classes / mixed_rays, whose census
tests/test_degenerate_rays_cpu.py checks on the oracle alone.  The ordinary rays that share a wave with a degenerate one are the point of
the mixed batches: k_cast_w chooses between the general and the ordered slab test per WAVE.

Why every class terminates (k_cast_w, its exact walk, and k_cast_f; read before the first run):
  - the walks follow child links of a finite tree and never revisit a node: a step either descends into a child whose slab test passed or
    pops; what a ray's bits can change is only WHICH tests pass.  A comparison with a NaN is false, so a NaN slab result (t1 >= t0 or
    t1 > 0 with a NaN, ray_box(..) > 0 with a NaN) is "not hit": fewer children, never more than four pushes per step, which the stack
    room is checked for before the step (a full stack parks the ray for the exact walk, whose overflow stack is bounds-checked);
  - the triangles of a leaf are walked from the leaf's first record to the record that carries the `last` flag: the count is the table's,
    not the ray's; a NaN or infinite t, u or v only fails the acceptance comparisons;
  - nothing in a walk iterates "until t exceeds something": tmax and the hit distance only enter comparisons, so tmax = NaN, 0, -1 or +inf
    changes results, not trip counts; the light-sphere loop runs light_count times;
  - the queues are consumed by counters, independent of the rays; one ray or an uneven pair of batches only changes how many lanes idle;
  - the watchdog (castLoopCap iterations per wave) is the backstop: it would set GMUPT_STAT_CAST_ABORTED, which every test here asserts absent.
"""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import oracle_lib as O
import parity_util as PU
import trace_util as T

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scenes(soup_scene, spheres_small_scene):
    return {"soup": soup_scene, "spheres": spheres_small_scene}


@pytest.fixture(scope="module")
def classes(soup_scene):
    """{class: (closest, any_rays, {light_count: oracle truth})} on the soup: computed once, read-only."""
    out = {}
    for name, (c, a) in T.degenerate_classes(soup_scene, 1024).items():
        out[name] = (c, a, {lc: T.oracle_truth(soup_scene, c, a, lc) for lc in (0, soup_scene["light_count"])})
    return out


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def renderer(pkg, device, scene, pool=4096, **kw):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, 32, 18, pool_paths=pool, **kw)
    r.bind_scene(sb)
    return r, sb


def traced(pkg, r, closest, any_rays, lc):
    """(hits, occluded) as numpy; the launch was the wide kernel and raised no fault flag."""
    info = pkg.capi.TraceInfo()
    hits, occ = r.trace(gpu(closest) if len(closest) else None, gpu(any_rays) if len(any_rays) else None, light_count=lc, info=info)
    assert info.flags & pkg.capi.STAT_CAST_WIDE and not (info.flags & (pkg.capi.STAT_STACK_OVERFLOW | pkg.capi.STAT_CAST_ABORTED)), "flags %#x" % info.flags
    return hits.cpu().numpy(), occ.cpu().numpy()


def test_one_wave_of_each_class(pkg, device, wide, soup_scene, classes):
    # the smallest launch first: 64 closest-hit and 64 any-hit rays of one class
    r, sb = renderer(pkg, device, soup_scene)
    lc = soup_scene["light_count"]
    for name, (c, a, truth) in classes.items():
        h, o = traced(pkg, r, c[:64], a[:64], lc)
        T.assert_matches_oracle(soup_scene, c[:64], a[:64], h, o, lc, truth=truth[lc])
    r.close(); sb.close()


@pytest.mark.parametrize("name", list(T.RAY_CLASSES) + ["tmax_any"])
def test_whole_wave_classes_match_the_oracle(pkg, device, wide, soup_scene, classes, name):
    c, a, truth = classes[name]
    r, sb = renderer(pkg, device, soup_scene)
    for lc in (0, soup_scene["light_count"]):
        h, o = traced(pkg, r, c, a, lc)
        T.assert_matches_oracle(soup_scene, c, a, h, o, lc, truth=truth[lc])
        f = pkg.capi.hit_fields(h)
        if name in T.MISS_CLASSES:      # include/gmupt.h: a miss of every triangle and light, occluded = 0
            assert (f["triangle"] == -1).all() and (f["t"] == T.FLT_MAX).all() and not f["light"].any() and not f["material"].any() and not o.any()
            assert not f["u"].any() and not f["v"].any()
        elif name != "tmax_any":        # "a zero or denormal direction component alone is an ordinary ray"
            assert (f["triangle"] >= 0).sum() >= 100
        if name == "tmax_any":          # include/gmupt.h: tmax <= 0 or NaN never occludes
            with np.errstate(invalid="ignore"):
                assert not o[~(a[:, 3] > 0)].any() and o[np.isposinf(a[:, 3])].sum() > 10
    r.close(); sb.close()


def test_closest_hit_tmax_follows_the_header(pkg, device, wide, soup_scene):
    # include/gmupt.h: tmax <= 0 (-0.0 included) or NaN: the miss record with t = the bits of tmax; +inf: the FLT_MAX record, a miss has t = +inf
    n = 1024
    closest, _ = T.random_rays(soup_scene, n, np.random.default_rng(5))
    r, sb = renderer(pkg, device, soup_scene)
    base, _ = traced(pkg, r, closest, closest[:0], 0)
    T.assert_matches_oracle(soup_scene, closest, closest[:0], base, np.zeros(0, np.uint32), 0)
    limited = closest.copy(); limited[:, 3] = T.CLOSEST_TMAX[np.arange(n) % len(T.CLOSEST_TMAX)]
    got, _ = traced(pkg, r, limited, closest[:0], 0)
    exp = T.expected_closest_with_tmax(base.view(np.uint32), limited[:, 3])
    bad = np.nonzero((got.view(np.uint32) != exp).any(axis=1))[0]
    assert len(bad) == 0, "%d records differ, first ray %d (tmax %r): got %r expected %r" % (len(bad), bad[0], limited[bad[0], 3], got.view(np.uint32)[bad[0]], exp[bad[0]])
    # with the scene's light spheres: still nothing below a tmax <= 0 or NaN
    lit, _ = traced(pkg, r, limited, closest[:0], soup_scene["light_count"])
    with np.errstate(invalid="ignore"):
        none = ~(limited[:, 3] > 0)
    assert np.array_equal(lit.view(np.uint32)[none], exp[none])
    r.close(); sb.close()


@pytest.mark.parametrize("scene_name,k", [("soup", 1), ("soup", 7), ("soup", 32), ("soup", 63), ("spheres", 7), ("spheres", 32)])
def test_mixed_waves(pkg, device, wide, scenes, scene_name, k):
    scene = scenes[scene_name]
    lc = scene["light_count"]
    closest, any_rays, mask, base_c, base_a = T.mixed_rays(scene, 4096, k, seed=5)
    r, sb = renderer(pkg, device, scene)
    h, o = traced(pkg, r, closest, any_rays, lc)
    T.assert_matches_oracle(scene, closest, any_rays, h, o, lc)
    # GPU against GPU: the ordinary lanes get the records they get in a batch without any degenerate ray (the wave-level choice of slab test)
    h0, o0 = traced(pkg, r, base_c, base_a, lc)
    assert np.array_equal(h.view(np.uint32)[~mask], h0.view(np.uint32)[~mask]) and np.array_equal(o[~mask], o0[~mask])
    assert (pkg.capi.hit_fields(h0)["triangle"][~mask] >= 0).any() and o0[~mask].any()
    r.close(); sb.close()


@pytest.mark.parametrize("n_closest,n_any", [(1, 0), (0, 1), (1, 1), (63, 65), (65, 63), (127, 129), (129, 1)])
def test_tiny_and_uneven_batches(pkg, device, wide, soup_scene, n_closest, n_any):
    closest, any_rays, mask, _, _ = T.mixed_rays(soup_scene, 256, 32, seed=11)
    first = int(np.nonzero(mask)[0][0])                      # a one-ray batch is a degenerate ray
    c, a = closest[first: first + n_closest], any_rays[first + 1: first + 1 + n_any]
    lc = soup_scene["light_count"]
    r, sb = renderer(pkg, device, soup_scene)
    h, o = traced(pkg, r, c, a, lc)
    assert h.shape == (n_closest, 8) and o.shape == (n_any,)
    T.assert_matches_oracle(soup_scene, c, a, h, o, lc)
    r.close(); sb.close()


# ---- the renderer's own cast (StateIO of k_cast_w, and k_cast_f) on the same rays: a frozen path state against the oracle's two stages
FIELDS = ["surfacePoint", "baryCoord", "triangle", "isEmitter", "hitDistance", "inShadow"]


def frozen_state(pkg, scene, closest, any_rays):
    """The oracle with the rays in its path state, identity queues, after its extension and shadow stages; and the state before them."""
    P = len(closest)
    orc = O.Renderer(scene, 32, 18, P, threads=8)
    st = orc.path_state()
    f32 = lambda name: O.state_field(st, P, name).view(np.float32)
    f32("rayOrigin")[:] = closest[:, 0:3]; f32("rayDirection")[:] = closest[:, 4:7]
    f32("shadowrayOrigin")[:] = any_rays[:, 0:3]; f32("shadowrayDirection")[:] = any_rays[:, 4:7]
    f32("lightDistance")[:, 0] = any_rays[:, 3]
    orc.queues()[3][:] = np.arange(P, dtype=np.uint32); orc.queues()[4][:] = np.arange(P, dtype=np.uint32)
    qc = orc.counters(); qc[:] = 0; qc[6] = P; qc[7] = P
    cam = pkg.capi.Camera(32, 18); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    cb = cam.buffer_copy(); cam.close()
    orc.set_camera(cb)
    before = (orc.path_state().copy(), orc.queues().copy(), orc.counters().copy())
    orc.stage("extension"); orc.stage("shadow")
    return orc, before, cb


@pytest.fixture(scope="module")
def frozen(pkg, soup_scene):
    closest, any_rays, mask, base_c, base_a = T.mixed_rays(soup_scene, 4096, 7, seed=5)
    mixed = frozen_state(pkg, soup_scene, closest, any_rays)
    control = frozen_state(pkg, soup_scene, base_c, base_a)
    yield {"mixed": mixed, "control": control}
    mixed[0].close(); control[0].close()


def run_raycasts(pkg, dev, scene, state):
    orc, before, cb = state
    P = orc.pool
    sb = pkg.capi.SceneBuffers(dev, scene)
    hip = pkg.capi.Renderer(dev, 32, 18, pool_paths=P, collect_stats=True)
    hip.bind_scene(sb); hip.set_camera(cb)
    hip.write_path_state(before[0]); hip.write_queues(before[1]); hip.write_counters(before[2])
    hip.run_stage(pkg.capi.STAGE_RAYCASTS)
    bad = PU.compare_state(orc, hip, P, P, fields=FIELDS)
    st = hip.stats()
    hip.close(); sb.close()
    assert not bad, bad[:3]
    assert not (st.flags & (pkg.capi.STAT_STACK_OVERFLOW | pkg.capi.STAT_CAST_ABORTED)), "flags %#x" % st.flags
    return st


@pytest.mark.parametrize("traversal", ["wide", "cast0"])
def test_renderer_cast_on_mixed_waves(pkg, device, monkeypatch, soup_scene, frozen, traversal):
    monkeypatch.setenv("GMUPT_TRAVERSAL", traversal)
    st = run_raycasts(pkg, device, soup_scene, frozen["mixed"])
    ctl = run_raycasts(pkg, device, soup_scene, frozen["control"])
    if traversal == "wide":
        assert st.flags & pkg.capi.STAT_CAST_WIDE and ctl.flags & pkg.capi.STAT_CAST_WIDE
        print("wide_general_iterations / wide_iterations: mixed %d / %d, control %d / %d" % (st.wide_general_iterations, st.wide_iterations, ctl.wide_general_iterations, ctl.wide_iterations))
        assert 0 < st.wide_general_iterations <= st.wide_iterations
        # every component of the control batch is a non-zero normal number (test_degenerate_rays_cpu.py): ordered slab tests only
        assert ctl.wide_general_iterations == 0 and ctl.wide_iterations > 0
    else:
        assert st.flags & pkg.capi.STAT_CAST_FETCH and not (st.flags & pkg.capi.STAT_CAST_WIDE), "flags %#x" % st.flags


def test_renderer_cast_on_mixed_waves_with_tiny_stacks(pkg, monkeypatch, soup_scene, frozen):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    with pkg.capi.use_build("wides8"):
        dev = pkg.capi.Device(0)
        st = run_raycasts(pkg, dev, soup_scene, frozen["mixed"])
        dev.close()
    assert st.flags & pkg.capi.STAT_CAST_WIDE and st.cast_redo_rays > 0 and 0 < st.wide_general_iterations <= st.wide_iterations


# ---- consumers: pick and the AOVs under a camera whose axes are exactly axis-aligned
def test_pick_and_aovs_with_axis_aligned_primary_rays(pkg, device, wide, cornell_scene):
    scene = cornell_scene
    W, H = 32, 18
    lc = scene["light_count"]
    x, y, z, _, _ = scene["camera"]
    cam = pkg.capi.Camera(W, H); cam.set_pose(x, y, z, 0.0, 270.0); cam.buffer.lightCount = lc; cam.update(0.0)
    hor, ver = list(cam.buffer.horizontal)[:3], list(cam.buffer.vertical)[:3]
    assert hor[1] == 0.0 and hor[2] == 0.0 and ver[0] == 0.0 and ver[2] == 0.0, (hor, ver)
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([np.frombuffer(bytes(pkg.capi.camera_pick_ray(cam.buffer, px, py)), np.float32) for px, py in zip(xs.ravel(), ys.ravel())])
    zero = rays[:, 4:7] == 0
    assert zero[:, 0].sum() == H and zero[:, 1].sum() == W, "the centre column and the middle row have an exact zero component"
    r, sb = renderer(pkg, device, scene)
    r.set_camera(cam.buffer)
    hits, _ = traced(pkg, r, rays, rays[:0], lc)
    T.assert_matches_oracle(scene, rays, rays[:0], hits, np.zeros(0, np.uint32), lc)
    f = pkg.capi.hit_fields(hits)
    assert (f["triangle"][zero.any(axis=1)] >= 0).sum() > 10
    # the camera's sums round x + (-x) to +0.0, never to -0.0: the same rays with their zeros negated (an editor's mirrored camera)
    neg = rays.copy(); neg[:, 4:7][zero] = np.float32(-0.0)
    hn, _ = traced(pkg, r, neg, rays[:0], lc)
    T.assert_matches_oracle(scene, neg, rays[:0], hn, np.zeros(0, np.uint32), lc)
    # pick: the pixels with zero components, the corners and one ordinary pixel
    special = np.nonzero(zero.any(axis=1))[0]
    for k in [0, W * H - 1, W * 5 + 3] + special[:: max(1, len(special) // 8)].tolist():
        ray, hit = r.pick(xs.ravel()[k], ys.ravel()[k], lc)
        assert bytes(ray) == rays[k].tobytes() and bytes(hit) == hits[k].tobytes(), k
    # AOVs at one sample per pixel: the centre ray's t, ids and position
    a = pkg.capi.aov_fields(r.aovs(1))
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32)
    assert np.array_equal(bits(a["depth"].ravel()), bits(f["t"])) and np.array_equal(a["triangle"].ravel(), f["triangle"])
    assert np.array_equal(a["material"].ravel(), f["material"]) and np.array_equal(a["light"].ravel(), f["light"])
    found = (f["triangle"] >= 0) | (f["light"] > 0)
    with np.errstate(over="ignore"):
        pos = (rays[:, 0:3] + rays[:, 4:7] * f["t"][:, None]).astype(np.float32)
    assert np.array_equal(bits(a["position"].reshape(-1, 3)[found]), bits(pos[found])) and not a["position"].reshape(-1, 3)[~found].any()
    r.close(); sb.close(); cam.close()
