"""GPU tests of the image stages on non-finite and extreme pixels: k_dn_prepare / k_dn_variance / k_dn_atrous, k_tp_integrate /
k_tp_integrate_mv and k_mv_resolve against their host twins on the crafted frames of image_edges_util, under same_or_nan (bits, except
that a NaN on the host matches any NaN on the device, in the same words).  tests/test_image_edges_cpu.py holds the host side against
float64 and the stated rule, and asserts that at least half of the colour words of every frame compared here are compared on bits."""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import image_edges_util as E

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def renderer(pkg, device):
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)          # the image stages need no scene: any renderer's stream and scratch
    yield r
    r.close()


def test_tensors_carry_nan_bits_to_the_device_and_back():
    a = np.array([0x7F800001, 0xFFC00000, 0x7FC00001, 0x80000000, 0x00000001], np.uint32).view(np.float32)
    assert np.array_equal(E.bits(cuda(a).clone()), E.bits(a)), "a signalling NaN pattern survives the copies the tests make"


@pytest.mark.parametrize("layout", ["isolated", "dense"])
def test_denoiser_matches_the_host_filter_on_crafted_frames(pkg, renderer, layout):
    capi = pkg.capi
    excused = compared = 0
    for (name, b, a, pl, passes) in E.denoise_cases():
        if "/" + layout + "/" not in name:
            continue
        bt, at = cuda(b), cuda(a)
        for params in E.PSETS:
            for p in passes:
                got = capi.denoise_image(renderer, bt, at, passes=p, **params)
                nan = E.same_or_nan(got, capi.denoise_host(b, a, threads=16, passes=p, **params), (name, p, params), pl)
                excused += int(nan.sum()); compared += nan.size
    assert 0 < excused < compared // 2


def test_denormal_plane_on_the_device(pkg, renderer):
    capi = pkg.capi
    b, a = E.denormal_plane()
    for p in (1, 3, 5):
        got = capi.denoise_image(renderer, cuda(b), cuda(a), passes=p)
        assert np.array_equal(E.bits(got), E.bits(capi.denoise_host(b, a, passes=p))), p
        assert (E.bits(got)[..., :3] != 0).all() and (E.bits(got)[..., :3] < 0x00800000).all(), "non-zero denormals: nothing was flushed"


def run_sequence(capi, renderer, calls, what):
    """calls: (beauty, aov, cam, origin, new_accumulation, keywords).  The device handle against the host chain under same_or_nan, and
    consequence (b): the device output is the device denoiser on the host-integrated image.  Returns the pixels that took history."""
    t = capi.Temporal(renderer)
    chain = E.Chain(capi)
    used = 0
    for k, (b, a, cam, origin, new, kw) in enumerate(calls):
        dev_kw = dict(kw)
        if dev_kw.get("motion") is not None:
            dev_kw["motion"] = cuda(dev_kw["motion"])
        got = capi.temporal_denoise_image(t, cuda(b), cuda(a), cam, new, origin, **dev_kw)
        exp = chain.call(b, a, cam, origin, new, **kw)
        E.same_or_nan(got, exp, (what, "call", k))
        assert E.comparable_share(exp, E.valid_mask32(chain.integrated, a)) >= 0.5, (what, k)
        if kw.get("infill") is None:
            spatial = {k2: v for k2, v in kw.items() if k2 in E.SPATIAL}
            E.same_or_nan(got, capi.denoise_image(renderer, cuda(chain.integrated), cuda(a), **spatial), (what, "(b)", k))
        used = int((E.bits(chain.integrated)[..., 3] != E.bits(b)[..., 3]).sum())
    t.close()
    return used


def test_temporal_matches_the_host_chain_on_crafted_sequences(pkg, renderer):
    """The poisoned first call's records become the history; the second call comes from a moved pose: with and without new_accumulation,
    history_cap 0 and 65536, a sub-rectangle origin, a motion plane with non-finite records, the infill in front of the filter; the
    projection edges (lambda 0 / denormal / NaN, u or v at +-2^31, +-1e30, +-inf, fu = -1 and W - 1) under three previous cameras; and
    a history and a frame of denormal colours, whose blend a flush to zero in k_tp_integrate would change."""
    seen = set()
    for (name, calls) in E.temporal_cases(pkg):
        used = run_sequence(pkg.capi, renderer, calls, name)
        assert (used > 0) == (name != "cap 0" and "zero_" not in name), name
        seen.add(name.split("/")[0])
    assert seen == {"fold", "no fold, then fold", "cap 0", "motion", "infill", "sub-rectangle", "projection", "denormal history"}


def test_motion_plane_with_non_finite_previous_vertices(pkg, device, monkeypatch):
    """k_mv_resolve against gmupt_motion_host with NaN and inf vertices in the previous pose only: bprev == bnow is false for NaN."""
    from test_motion_gpu import host_motion, make_camera
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.cornell_mesh())
    W, H = 48, 27
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=2048)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    r.set_camera(cam.buffer)
    now = scene["verts"]
    prev = pkg.scenes.wobble(scene, 0.3, 0.05).copy()
    n = len(prev)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e38, 1e-40, -0.0)):
        prev[(k * 3 + 1) % n::11, k % 3] = v
    aov, mv = r.aovs_motion(cuda(prev), 1)
    want = host_motion(pkg, r, scene, cam.buffer, aov, now, prev, W, H).view(np.float32).reshape(H, W, 4)
    nan = E.same_or_nan(mv, want, "motion plane")
    f = capi.motion_fields(mv)
    moved = f["flags"] == 1
    assert nan.any() and np.isinf(f["prev_position"]).any()
    assert nan[..., :3][moved].mean() <= 0.5, "at least half of the moved records' position words are compared on bits"
    assert np.isfinite(f["prev_position"][moved]).all(-1).mean() > 0.1
    # the records go on into the integration: device == host chain.  This AOV image comes from a device render, so the half-of-words
    # cap of this one sequence is asserted here, on the host chain's output inside run_sequence, not in the CPU file.
    b = np.zeros((H, W, 4), np.float32)
    b[..., :3] = np.clip(aov.cpu().numpy()[..., :3] * 0.6, 0, 1); b[..., 3] = np.uint32(1).view(np.float32)
    an = aov.cpu().numpy()
    calls = [(b, an, cam.buffer_copy(), (0, 0), 1, {}), (b, an, cam.buffer_copy(), (0, 0), 1, {"motion": mv.cpu().numpy()})]
    run_sequence(capi, r, calls, "motion records")
    r.close(); sb.close(); cam.close()
