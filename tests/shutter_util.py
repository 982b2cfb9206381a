"""What the shutter tests share: a numpy restatement of the rule of include/gmupt_shutter.h, written from the header in float32 with the
oracle's sin / cos (through the restatements of lens_util.py and projection_util.py, which take one camera: the camera of a path is
built here, path by path), the pose pairs, and the helpers of the GPU tests."""
import numpy as np

import lens_util as LU
import projection_util as PU

F = np.float32
VECTORS = ("position", "upperLeftCorner", "horizontal", "vertical")

# (open pose, close pose): a pure translation, a pure yaw of 3 degrees, both
POSE_PAIRS = {
    "translation": ((1.0, 3.0, 8.0, 0.0, 270.0), (1.6, 3.1, 7.8, 0.0, 270.0)),
    "yaw3": ((0.7, 1.3, 2.1, -12.0, 250.0), (0.7, 1.3, 2.1, -12.0, 253.0)),
    "both": ((-1.5, 0.4, -0.8, 25.0, 140.0), (-1.2, 0.5, -1.1, 25.0, 143.0)),
}
RESOLUTIONS = LU.RESOLUTIONS
QS = [0, 1, 255, 256, 65535, (1 << 21) - 1]


def copy_buffer(cb):
    return type(cb).from_buffer_copy(bytes(cb))


def pair(capi, W, H, name, updates=1):
    """(open CameraBuffer, Shutter of the close pose) of POSE_PAIRS[name] at W x H."""
    a, b = POSE_PAIRS[name]
    cam = LU.camera(capi, W, H, a, updates=updates)
    close = LU.camera(capi, W, H, b)
    cb, sh = cam.buffer_copy(), capi.shutter.from_camera(close.buffer_copy())
    cam.close(); close.close()
    return cb, sh


def draws(O, cb, q, n=5):
    """The first n draws of the generator of the fresh paths q: an (n, N) float32 array.  Row 4 is the time (step 1)."""
    g = LU.Rng(O, np.asarray(q, np.uint32), cb.randomSeed[0], cb.randomSeed[1])
    return np.stack([g.next() for _ in range(n)])


def time(O, cb, q):
    return draws(O, cb, q)[4]


def camera_at(cb, sh, t):
    """Step 2: a copy of cb whose twelve pose components are a + (b - a) * t in binary32."""
    out = copy_buffer(cb)
    t = F(t)
    for name in VECTORS:
        a, b = np.array(getattr(cb, name)[:3], F), np.array(getattr(sh, name)[:3], F)
        c = (a + ((b - a).astype(F) * t).astype(F)).astype(F)
        for k in range(3):
            getattr(out, name)[k] = float(c[k])
    return out


def pinhole(O, cb, q, cx, cy):
    """origin = position, direction = step 1 of the lens rule."""
    pos, ulc, hor, ver = LU.cam_vectors(cb)
    u, v, _, _ = PU.jittered_uv(O, cb, q, cx, cy)
    d = LU.normalize3(((ulc + (hor * u[:, None]).astype(F)).astype(F) - (ver * v[:, None]).astype(F)).astype(F))
    return np.broadcast_to(pos, d.shape).copy(), d


def rule(O, cb, sh, q, cx, cy, lens=None, proj=None):
    """The three steps for arrays (q, cx, cy): (N, 8) gmupt_ray words, and the times."""
    q, cx, cy = (np.asarray(x, np.uint32) for x in (q, cx, cy))
    ts = time(O, cb, q)
    out = np.zeros((q.size, 8), F)
    for i in range(q.size):
        c = camera_at(cb, sh, ts[i])
        qi, xi, yi = q[i:i + 1], cx[i:i + 1], cy[i:i + 1]
        if lens is not None:
            r = LU.rule(O, c, lens.aperture_radius, lens.focus_distance, qi, xi, yi)
            o, d = r["origin"], r["direction"]
        elif proj is not None:
            o, d = PU.rule_fresh(O, c, proj, qi, xi, yi)
        else:
            o, d = pinhole(O, c, qi, xi, yi)
        out[i] = PU.words(o, d)[0]
    return out, ts


def samples(W, H):
    """(q, cx, cy): every q of QS at the corners of the frame, a tile-origin pixel and a pixel inside."""
    pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 3, H // 3), (W // 2 + 1, H // 2)]
    q = np.repeat(np.array(QS, np.uint32), len(pix))
    xy = np.tile(np.array(pix, np.uint32), (len(QS), 1))
    return q, xy[:, 0].copy(), xy[:, 1].copy()


def has_negative_zero(cb):
    return any(np.signbit(F(getattr(cb, n)[k])) and getattr(cb, n)[k] == 0.0 for n in VECTORS for k in range(3))


def host_rays(capi, cb, sh, raw, pool, q, slots, lens=None, proj=None):
    """gmupt_shutter_ray_host of the fresh slots: their queue indices and the screen coordinates the state holds."""
    xy = LU.state_screen(raw, pool)[slots]
    return capi.shutter.rays_host(cb, sh, q, xy[:, 0], xy[:, 1], lens=lens, projection=proj)
