"""What the feature modules share on the way into the library: the renderer's torch device, staging of arrays and images, the params
builder and the base of the handle classes.  A helper that raises takes the caller's name for the message.  torch is imported inside
the functions that need it, so that importing the binding does not touch the GPU runtime."""
import ctypes as C

import numpy as np

from ._abi import _P, ERR_INVALID_ARGUMENT, GmuptError, Ray, aov_dtype
from ._lib import _check, lib


def torch_device(dev):
    """(torch, the torch device of `dev`): dev is a Device or anything with its `index` (a stand-in without one means GPU 0)."""
    import torch
    return torch, torch.device("cuda", getattr(dev, "index", 0))


def device_tensor(a, device, np_dtype, shape, ok, error):
    """`a` as a contiguous tensor on `device`: a torch tensor that `ok` accepts is used in place (else GmuptError(error)), anything else
    is a host array, uploaded as `np_dtype` in `shape` (None: its own)."""
    import torch
    if isinstance(a, torch.Tensor):
        if not ok(a):
            raise GmuptError(error, ERR_INVALID_ARGUMENT)
        return a.contiguous()
    a = np.ascontiguousarray(a, dtype=np_dtype)
    return torch.from_numpy(a if shape is None else a.reshape(shape)).to(device)


def host_words(x, records=None):
    """numpy or torch -> a contiguous float32 numpy array; an array of the `records` dtype becomes its float32 words on a new last axis."""
    a = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    if records is not None and a.dtype == records:
        a = a.view(np.float32).reshape(a.shape + (records.itemsize // 4,))
    return np.ascontiguousarray(a, dtype=np.float32)


def device_images(who, beauty, aov):
    """The (H, W, 4) beauty and (H, W, 16) AOV float32 tensors on the GPU of an *_image call, checked and contiguous."""
    import torch
    if beauty.dim() != 3 or beauty.shape[2] != 4 or aov.dim() != 3 or aov.shape[2] != 16 or tuple(aov.shape[:2]) != tuple(beauty.shape[:2]):
        raise GmuptError("%s: beauty must be (H, W, 4) and aov (H, W, 16)" % who, ERR_INVALID_ARGUMENT)
    if beauty.dtype != torch.float32 or aov.dtype != torch.float32 or not beauty.is_cuda or not aov.is_cuda:
        raise GmuptError("%s: float32 tensors on the GPU" % who, ERR_INVALID_ARGUMENT)
    return beauty.contiguous(), aov.contiguous()


def host_images(who, beauty, aov):
    """The (H, W, 4) beauty and (H, W, 16) AOV images of a *_host call (numpy or torch; aov also as (H, W) records) as float32 arrays."""
    b, a = host_words(beauty), host_words(aov, aov_dtype)
    if b.ndim != 3 or b.shape[2] != 4 or a.shape != b.shape[:2] + (16,):
        raise GmuptError("%s: beauty must be (H, W, 4) and aov (H, W, 16)" % who, ERR_INVALID_ARGUMENT)
    return b, a


def make_params(struct, defaults, what, params, fields, inner=None, inner_fields=()):
    """struct() filled by the library's `defaults` function, then every given parameter set: one of `fields` on the structure, one of
    `inner_fields` on its member `inner`; any other name is a TypeError about an unknown `what` parameter."""
    p = struct()
    getattr(lib(), defaults)(C.byref(p))
    for k, v in params.items():
        if k in fields:
            setattr(p, k, v)
        elif k in inner_fields:
            setattr(getattr(p, inner), k, v)
        else:
            raise TypeError("unknown %s parameter %r" % (what, k))
    return p


def opt_ref(struct):
    """byref(struct), or NULL for None: an optional structure argument (`lens_or_null`, `proj_or_null`)."""
    return C.byref(struct) if struct is not None else None


def aov_ray_table(fn, cam_buffer, rule, xs, ys, samples):
    """All s*s-ray-plan AOV rays of the pixels (xs[i], ys[i]) as an (N, R, 8) float32 array of gmupt_ray records (R = samples^2):
    fn(cam, rule, x, y, samples, k, ray) is gmupt_aov_lens_ray or gmupt_aov_projected_ray, `rule` its Lens or Projection."""
    R = samples * samples
    out = np.empty((len(xs), R, 8), np.float32)
    ray = Ray()
    pc, pp, pr = C.byref(cam_buffer), C.byref(rule), C.byref(ray)
    for i, (x, y) in enumerate(zip(xs, ys)):
        for k in range(R):
            _check(fn(pc, pp, int(x), int(y), int(samples), k, pr))
            out[i, k] = np.frombuffer(ray, np.float32)
    return out


def guided_inputs(renderer, aov):
    """(beauty, aov) for an *_image stage: the renderer's frame as an (H, W, 4) float32 tensor (gmupt_copy_framebuffer_to_device) next to
    the (H, W, 16) records `aov`, on their GPU."""
    import torch
    beauty = torch.empty(tuple(aov.shape[:2]) + (4,), dtype=torch.float32, device=aov.device)
    renderer.copy_framebuffer_to_device(beauty.data_ptr(), beauty.numel() * 4)
    return beauty, aov


# Base of every class that wraps a library object in `h`: close() destroys it through the function the subclass names in _destroy;
# closing twice, or after the owner, is harmless.  _open() is the create of the handles made from an owner (a renderer or a device); a
# subclass that names the owner's list in _siblings registers there, the owner closes what is in it, and close() takes it out again.
# (A comment, not a docstring: a subclass without a docstring would show this one.)
class Handle:
    _destroy = _siblings = None

    def _open(self, owner, create, *args):
        self.h = _P()
        _check(getattr(lib(), create)(owner.h, *args, C.byref(self.h)))
        self._owner = owner
        if self._siblings:
            getattr(owner, self._siblings).append(self)

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = _P()
            if self._siblings and self in getattr(self._owner, self._siblings):   # (the owner's close() walks a copy of the list)
                getattr(self._owner, self._siblings).remove(self)
