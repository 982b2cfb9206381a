"""What the lens tests share: a numpy restatement of the rule of include/gmupt_lens.h, written from the header in float32 arrays with
the oracle's sin / cos (oracle_lib.detmath), the camera poses, and the helpers that take rays out of a path state."""
import ctypes as C

import numpy as np

F = np.float32
K_PI, K_INV_PI = F(3.14159274), F(0.318309873)          # structs.h:14,15 as binary32
TWO_PI = F(6.2831853)

# the default camera of the scenes (Scene.cpp:59) first; two more poses off the axes
POSES = [(1.0, 3.0, 8.0, 0.0, 270.0), (0.7, 1.3, 2.1, -12.0, 250.0), (-1.5, 0.4, -0.8, 25.0, 140.0)]
RESOLUTIONS = [(32, 18), (1920, 1080)]


def _frac(x):
    return (x - np.floor(x)).astype(F)


class Rng:
    """random.h:6-12 for an array of seeds."""

    def __init__(self, O, q, rs0, rs1):
        fi = np.asarray(q, np.uint32).astype(F)
        self.O = O
        self.sx, self.sy = _frac(fi * K_INV_PI), _frac(fi * K_PI)
        self.rsx, self.rsy = F(rs0), F(rs1)

    def next(self):
        self.sx = (self.sx - self.rsx).astype(F)
        self.sy = (self.sy - self.rsy).astype(F)
        d = ((self.sx * F(12.9898)).astype(F) + (self.sy * F(78.233)).astype(F)).astype(F)
        return _frac((self.O.detmath(0, d) * F(43758.5453)).astype(F))


def dot3(a, b):
    return (((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)).astype(F)


def normalize3(a):
    inv = (F(1.0) / np.sqrt(dot3(a, a)).astype(F)).astype(F)
    return (a * inv[..., None]).astype(F) if inv.ndim else (a * inv).astype(F)


def cam_vectors(cb):
    return tuple(np.array(list(v)[:3], F) for v in (cb.position, cb.upperLeftCorner, cb.horizontal, cb.vertical))


def rule(O, cb, aperture, focus, q, cx, cy):
    """The five steps of the header for arrays (q, cx, cy).  Returns a dict of float32 arrays: d (step 1), jx, jy, lx, ly (step 2),
    right, up, fn (step 3), Pf (step 4), origin, direction (step 5)."""
    pos, ulc, hor, ver = cam_vectors(cb)
    ps = (F(cb.pixelSize[0]), F(cb.pixelSize[1]))
    g = Rng(O, q, cb.randomSeed[0], cb.randomSeed[1])
    jx = ((g.next() * F(2.0)).astype(F) - F(1.0)).astype(F)
    jy = ((g.next() * F(2.0)).astype(F) - F(1.0)).astype(F)
    u = ((np.asarray(cx, np.uint32).astype(F) + jx).astype(F) * ps[0]).astype(F)
    v = ((np.asarray(cy, np.uint32).astype(F) + jy).astype(F) * ps[1]).astype(F)
    d = normalize3(((ulc + (hor * u[:, None]).astype(F)).astype(F) - (ver * v[:, None]).astype(F)).astype(F))
    r1, r2 = g.next(), g.next()
    rad = (F(aperture) * np.sqrt(r1).astype(F)).astype(F)
    phi = (r2 * TWO_PI).astype(F)
    lx = (rad * O.detmath(1, phi)).astype(F)
    ly = (rad * O.detmath(0, phi)).astype(F)
    right, up = normalize3(hor), normalize3(ver)
    fn = normalize3(((ulc + (hor * F(0.5)).astype(F)).astype(F) - (ver * F(0.5)).astype(F)).astype(F))
    t = (F(focus) / dot3(d, fn)).astype(F)
    Pf = (pos + (d * t[:, None]).astype(F)).astype(F)
    origin = ((pos + (right * lx[:, None]).astype(F)).astype(F) + (up * ly[:, None]).astype(F)).astype(F)
    direction = normalize3((Pf - origin).astype(F))
    return dict(d=d, jx=jx, jy=jy, lx=lx, ly=ly, right=right, up=up, fn=fn, Pf=Pf, origin=origin, direction=direction)


def camera(capi, W, H, pose, updates=1):
    """A capi.Camera of a W x H frame at `pose`, updated `updates` times (each update draws a new randomSeed)."""
    cam = capi.Camera(W, H)
    cam.set_pose(*pose)
    for _ in range(updates):
        cam.update(0.0)
    return cam


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the path state in the reference layout (structs.h:19-48; gmupt_debug_read_path_state): field arrays one after the other, a
# float3 in a 16-byte slot
def state_rays(raw, pool):
    """(origin, direction) as (pool, 3) float32 views of a read_path_state() array."""
    o = raw[0:16 * pool].view(F).reshape(pool, 4)[:, :3]
    d = raw[16 * pool:32 * pool].view(F).reshape(pool, 4)[:, :3]
    return o, d


def state_screen(raw, pool):
    """(pool, 2) uint32: screenCoord of every slot (byte 236 of a path)."""
    return raw[236 * pool:244 * pool].view(np.uint32).reshape(pool, 2)


def patch_rays(raw, pool, slots, rays):
    """A copy of `raw` with origin and direction of `slots` replaced by the (N, 8) gmupt_ray records `rays`."""
    out = raw.copy()
    o, d = state_rays(out, pool)
    o[slots] = rays[:, 0:3]
    d[slots] = rays[:, 4:7]
    return out


def fresh(counters, queues, live, budget=0):
    """(queue indices, slots) of the fresh camera paths after a shading stage: the guards of k_lens_retarget on the host.  counters
    and queues are those read after the stage (lastPathCnt is advanced by the ray cast, later); live = the renderer's live paths."""
    n_new = min(int(counters[0]), int(live))
    q = np.arange(n_new, dtype=np.uint32)
    slots = queues[0][:n_new].astype(np.int64)
    keep = slots < live
    if budget:
        keep &= ((np.uint32(counters[1]) + q).astype(np.uint32) < np.uint32(budget))
    return q[keep], slots[keep]


def ray_words(ray):
    return np.frombuffer(bytes(ray), F).copy()


def lens_struct(capi, aperture, focus):
    return capi.lens.lens_params(aperture_radius=aperture, focus_distance=focus)


def null(t):
    return C.cast(None, C.POINTER(t))
