"""Shared helpers of the ray-query tests (test_trace_gpu.py, test_degenerate_rays_*.py): rays, the oracle's answer to them, the comparison.

Truth is the CPU oracle's own extension / shadow stages on a frozen state: the query's rays are written into rayOrigin / rayDirection /
shadowrayOrigin / shadowrayDirection / lightDistance with identity queues, orc.stage("extension") and orc.stage("shadow") run, and the
answers are compared bit for bit (t <-> hitDistance, u, v <-> baryCoord[1:], tris[triangle] <-> triangle, light <-> isEmitter,
occluded <-> inShadow).

The second half builds DEGENERATE rays -- NaN, infinities, signed zeros, denormals, huge and tiny magnitudes, odd tmax -- from ordinary
random rays: whole batches of one class (degenerate_classes) and ordinary batches with some lanes of every 64-ray wave replaced (mixed_rays).
"""
import numpy as np

import oracle_lib as O

FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny          # smallest normal
NO_TRI = 0xFFFFFFFF


def make_rays(origins, dirs, tmax):
    r = np.zeros((len(origins), 8), np.float32)
    r[:, 0:3] = origins; r[:, 3] = tmax; r[:, 4:7] = dirs
    return r


def oracle_truth(scene, closest, any_rays, light_count):
    """The oracle's extension / shadow stages on the query's rays: dict of per-ray fields (uint32 bit patterns)."""
    nC, nA = len(closest), len(any_rays)
    P = max(nC, nA, 64)
    orc = O.Renderer(scene, 32, 18, P)
    st = orc.path_state()
    O.state_field(st, P, "triangle")[:] = NO_TRI
    O.state_field(st, P, "baryCoord")[:] = NO_TRI
    if nC:
        O.state_field(st, P, "rayOrigin").view(np.float32)[:nC] = closest[:, 0:3]
        O.state_field(st, P, "rayDirection").view(np.float32)[:nC] = closest[:, 4:7]
    if nA:
        O.state_field(st, P, "shadowrayOrigin").view(np.float32)[:nA] = any_rays[:, 0:3]
        O.state_field(st, P, "shadowrayDirection").view(np.float32)[:nA] = any_rays[:, 4:7]
        O.state_field(st, P, "lightDistance").view(np.float32)[:nA, 0] = any_rays[:, 3]
    q = orc.queues(); q[3][:] = np.arange(P, dtype=np.uint32); q[4][:] = np.arange(P, dtype=np.uint32)
    qc = orc.counters(); qc[:] = 0; qc[7] = nC; qc[6] = nA
    cam = O.Camera(32, 18); cam.set_pose(*scene["camera"]); cam.update(); cam.buffer.lightCount = light_count
    orc.set_camera(cam.buffer)
    orc.stage("extension"); orc.stage("shadow")
    st = orc.path_state()
    out = {k: O.state_field(st, P, k).copy() for k in ("hitDistance", "baryCoord", "triangle", "isEmitter", "inShadow")}
    orc.close()
    return out


def assert_matches_oracle(scene, closest, any_rays, hits, occ, light_count, truth=None):
    t = truth or oracle_truth(scene, closest, any_rays, light_count)
    nC, nA = len(closest), len(any_rays)
    h = hits.view(np.uint32).reshape(-1, 8)
    hf = hits.view(np.float32).reshape(-1, 8)
    assert np.array_equal(h[:, 0], t["hitDistance"][:nC, 0]), "t"
    assert np.array_equal(h[:, 4], t["isEmitter"][:nC, 0]), "light"
    tri = h[:, 3].view(np.int32)
    hit = tri >= 0
    assert np.array_equal(hit, t["triangle"][:nC, 0] != NO_TRI), "which rays hit a triangle"
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    assert np.array_equal(recs[tri[hit]], t["triangle"][:nC][hit]), "triangle record"
    assert np.array_equal(h[hit, 5], recs[tri[hit], 3]), "material"
    assert np.array_equal(h[hit, 1:3], t["baryCoord"][:nC][hit, 1:3]), "u, v"
    assert not hf[~hit, 1:3].any() and (tri[~hit] == -1).all()
    assert np.array_equal(occ.astype(np.uint32), t["inShadow"][:nA, 0]), "occluded"


def random_rays(scene, n, rng, tmax_any=None):
    v = scene["verts"].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    o = (lo + rng.uniform(-0.1, 1.1, (n, 3)) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 2] /= np.linalg.norm(d[: n // 2], axis=1, keepdims=True)
    d = d.astype(np.float32)
    closest = make_rays(o, d, FLT_MAX)
    any_rays = make_rays(o, d, rng.uniform(0.05, 1.5, n).astype(np.float32) * np.float32(np.linalg.norm(ext)))
    return closest, any_rays


# ---------------------------------------------------------------------------------------------------------------- degenerate rays
# One class = one function (o, d, rng) that overwrites the (n, 3) float32 origins / directions of ordinary rays in place.
DENORMAL_INF = np.float32(1e-42)     # 1 / d overflows to infinity
DENORMAL_FINITE = np.float32(5e-39)  # still denormal (< 1.18e-38), 1 / d = 2e38 is finite


def _axis(n, rng):
    return np.arange(n), rng.integers(0, 3, n)


def _signs(n, rng):
    return np.where(rng.random(n) < 0.5, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


def _one_component(value):
    def f(o, d, rng):
        d[_axis(len(d), rng)] = np.float32(value) * _signs(len(d), rng)
    return f


def _two_denormals(o, d, rng):
    rows, k = _axis(len(d), rng)
    d[rows, k] = DENORMAL_INF * _signs(len(d), rng)
    d[rows, (k + 1 + rng.integers(0, 2, len(d))) % 3] = np.where(rng.random(len(d)) < 0.5, DENORMAL_INF, DENORMAL_FINITE) * _signs(len(d), rng)


def _negative_zero_component(o, d, rng):
    d[_axis(len(d), rng)] = np.float32(-0.0)     # (the other two components of a random_rays direction are non-zero)


def _signed_zero_axis(o, d, rng):
    rows, k = _axis(len(d), rng)
    d[:] = np.where(rng.random(d.shape) < 0.5, np.float32(-0.0), np.float32(0.0))
    d[rows, k] = _signs(len(d), rng)


def _zero_direction(o, d, rng):
    d[:] = np.float32(0.0)
    d[len(d) // 2:] = np.where(rng.random((len(d) - len(d) // 2, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))


def _scale_direction(s):
    def f(o, d, rng):
        d *= np.float32(s)
    return f


def _origin_component(value):
    def f(o, d, rng):
        o[_axis(len(o), rng)] = np.float32(value) * _signs(len(o), rng)
    return f


def _far_origin(o, d, rng):
    o *= np.float32(1e20)


RAY_CLASSES = {
    "denormal_inf": _one_component(DENORMAL_INF), "denormal_finite": _one_component(DENORMAL_FINITE), "denormal_two": _two_denormals,
    "negzero_component": _negative_zero_component, "signed_zero_axis": _signed_zero_axis,
    "nan_direction": _one_component(np.nan), "inf_direction": _one_component(np.inf), "zero_direction": _zero_direction,
    "huge_direction": _scale_direction(1e30), "tiny_direction": _scale_direction(1e-30),
    "nan_origin": _origin_component(np.nan), "inf_origin": _origin_component(np.inf), "far_origin": _far_origin,
}
HIT_CLASSES = ("denormal_inf", "denormal_finite", "denormal_two", "negzero_component", "signed_zero_axis", "huge_direction")   # rays that can hit
MISS_CLASSES = tuple(k for k in RAY_CLASSES if k not in HIT_CLASSES)                                                          # include/gmupt.h: a miss of everything
ANY_TMAX = np.array([0.0, -1.0, np.nan, np.inf, 1e-45, FLT_MAX], np.float32)
CLOSEST_TMAX = np.array([0.0, -1.0, np.nan, np.inf, -0.0], np.float32)


def degenerate_classes(scene, n=1024, seed=5):
    """{class: (closest, any_rays)}: the same n ordinary rays (random_rays) with one class applied to all of them, plus `tmax_any`:
    ordinary rays whose any-hit tmax cycles through ANY_TMAX."""
    base_c, base_a = random_rays(scene, n, np.random.default_rng(seed))
    out = {}
    with np.errstate(all="ignore"):
        for k, (name, f) in enumerate(RAY_CLASSES.items()):
            o, d = base_c[:, 0:3].copy(), base_c[:, 4:7].copy()
            f(o, d, np.random.default_rng([seed, k]))
            out[name] = (make_rays(o, d, FLT_MAX), make_rays(o, d, base_a[:, 3]))
    a = base_a.copy(); a[:, 3] = ANY_TMAX[np.arange(n) % len(ANY_TMAX)]
    out["tmax_any"] = (base_c.copy(), a)
    return out


def mixed_rays(scene, n, k, seed):
    """n ordinary rays in which k lanes of every 64-ray wave (seeded positions) carry degenerate rays of all RAY_CLASSES in turn; a third
    of those any-hit rays also get a tmax of ANY_TMAX.  Returns (closest, any_rays, degenerate mask, ordinary closest, ordinary any_rays)."""
    rng = np.random.default_rng([seed, k])
    base_c, base_a = random_rays(scene, n, np.random.default_rng(seed))
    lanes = np.concatenate([w + np.sort(rng.permutation(min(64, n - w))[:k]) for w in range(0, n, 64)])
    lanes = lanes[lanes < n]
    o, d, tmax = base_c[:, 0:3].copy(), base_c[:, 4:7].copy(), base_a[:, 3].copy()
    with np.errstate(all="ignore"):
        for j, f in enumerate(RAY_CLASSES.values()):
            rows = lanes[j::len(RAY_CLASSES)]
            oo, dd = o[rows], d[rows]
            f(oo, dd, rng)
            o[rows], d[rows] = oo, dd
    odd = lanes[::3]
    tmax[odd] = ANY_TMAX[np.arange(len(odd)) % len(ANY_TMAX)]
    mask = np.zeros(n, bool); mask[lanes] = True
    return make_rays(o, d, FLT_MAX), make_rays(o, d, tmax), mask, base_c, base_a


def is_miss_record(truth, n):
    """Per ray: the oracle's record is the miss record (no triangle, hitDistance = FLT_MAX, not in shadow)."""
    return ((truth["triangle"][:n, 0] == NO_TRI) & (truth["hitDistance"][:n, 0] == np.float32(FLT_MAX).view(np.uint32)) &
            (truth["inShadow"][:n, 0] == 0))


def expected_closest_with_tmax(hits_flt_max, tmax):
    """include/gmupt.h on tmax of a closest-hit ray, applied to the (n, 8) uint32 hit records the same rays get with tmax = FLT_MAX:
    tmax <= 0 or NaN -> the miss record with t = the bits of tmax; +inf -> the FLT_MAX record, a miss carrying t = +inf."""
    tmax = np.asarray(tmax, np.float32)
    exp = np.array(hits_flt_max, np.uint32).reshape(-1, 8).copy()
    with np.errstate(invalid="ignore"):
        none = ~(tmax > 0)                                      # <= 0, -0.0 and NaN
    miss = np.zeros(8, np.uint32); miss[3] = NO_TRI
    exp[none] = miss
    exp[none, 0] = tmax.view(np.uint32)[none]
    assert np.isposinf(tmax[~none]).all(), "only +inf is derived from the FLT_MAX record"
    was_miss = (exp[:, 3] == NO_TRI) & (exp[:, 4] == 0) & ~none
    exp[was_miss, 0] = np.float32(np.inf).view(np.uint32)
    return exp
