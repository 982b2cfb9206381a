"""The device and what lives in its memory: Device, Buffer, TextureArray, the PNG and texture helpers, SceneBuffers."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import (_P, BUFFER_BVH_NODES, BUFFER_LIGHTS, BUFFER_MATERIALS, BUFFER_TRI_PROPS, BUFFER_TRIANGLES, BUFFER_VERTICES,
                   ERR_INVALID_ARGUMENT, GmuptError)
from ._lib import _check, _ptr, lib
from ._stage import Handle, torch_device


class Device(Handle):
    _destroy = "gmupt_device_destroy"

    def __init__(self, index=0):
        self.h = _P()
        _check(lib().gmupt_device_create(index, C.byref(self.h)))
        _lib._devices_created += 1
        self.index = index

    def detmath(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty_like(x)
        _check(lib().gmupt_debug_detmath(self.h, fn, _ptr(x), _ptr(y), _ptr(out), x.size))
        return out


class Buffer(Handle):
    _destroy = "gmupt_buffer_destroy"

    def __init__(self, dev, kind, array):
        array = np.ascontiguousarray(array)
        self.h = _P()
        self.dev = dev
        _check(lib().gmupt_buffer_create(dev.h, kind, _ptr(array), array.nbytes, C.byref(self.h)))

    @classmethod
    def wrap(cls, dev, handle):
        """A Buffer around a gmupt_buffer the library created (gmupt_lbvh_build); close() destroys it like any other."""
        self = cls.__new__(cls)
        self.h, self.dev = handle, dev
        return self

    def update(self, array):
        array = np.ascontiguousarray(array)
        _check(lib().gmupt_buffer_update(self.h, _ptr(array), array.nbytes))

    def update_from_device(self, tensor):
        """gmupt_buffer_update_device: the buffer's first bytes from a torch tensor on this buffer's GPU (e.g. a pose computed there),
        without a trip through the host.  torch's current stream is synchronised first."""
        torch, device = torch_device(self.dev)
        if not isinstance(tensor, torch.Tensor) or tensor.device != device or not tensor.is_contiguous():
            raise GmuptError("update_from_device: a contiguous tensor on %s" % device, ERR_INVALID_ARGUMENT)
        nbytes = tensor.numel() * tensor.element_size()
        if nbytes > int(lib().gmupt_buffer_size(self.h)):
            raise GmuptError("update_from_device: %d bytes into a %d-byte buffer" % (nbytes, int(lib().gmupt_buffer_size(self.h))), ERR_INVALID_ARGUMENT)
        torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_buffer_update_device(self.h, C.c_void_p(tensor.data_ptr()), nbytes))

    def read(self, dtype=np.uint8):
        """The buffer's bytes as a new array of `dtype` (gmupt_buffer_read: synchronous)."""
        dtype = np.dtype(dtype)
        nbytes = int(lib().gmupt_buffer_size(self.h))
        out = np.empty(nbytes // dtype.itemsize, dtype=dtype)
        _check(lib().gmupt_buffer_read(self.h, _ptr(out), out.nbytes))
        return out


class TextureArray(Handle):
    """R8G8B8A8_UNORM Texture2DArray: (layers, size, size, 4) uint8."""
    _destroy = "gmupt_buffer_destroy"

    def __init__(self, dev, array):
        array = np.ascontiguousarray(array, dtype=np.uint8)
        assert array.ndim == 4 and array.shape[1] == array.shape[2] and array.shape[3] == 4
        self.h = _P()
        _check(lib().gmupt_texture_array_create(dev.h, _ptr(array), array.shape[1], array.shape[0], C.byref(self.h)))


def decode_png(data):
    """PNG file bytes -> (h, w, 4) uint8 through gmupt_image_decode_png (the reference's lodepng::decode call, Scene.cpp:226)."""
    w, h, mem = C.c_uint32(), C.c_uint32(), _P()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    _check(lib().gmupt_image_decode_png(buf, len(data), C.byref(w), C.byref(h), C.byref(mem)))
    try:
        out = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_uint8)), shape=(h.value, w.value, 4)).copy()
    finally:
        lib().gmupt_image_free(mem)
    return out


def resize_square(rgba, new_size):
    """Square RGBA8 resize: the bytes of the reference's avir call (Scene.cpp:276-279; host/AvirResize.cpp restates avir's pipeline for it)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    assert rgba.ndim == 3 and rgba.shape[0] == rgba.shape[1] and rgba.shape[2] == 4
    out = np.empty((new_size, new_size, 4), dtype=np.uint8)
    _check(lib().gmupt_image_resize_square(_ptr(rgba), rgba.shape[0], new_size, _ptr(out)))
    return out


def texture_common_size(layer_bytes):
    arr = (C.c_size_t * len(layer_bytes))(*layer_bytes)
    return int(lib().gmupt_texture_common_size(arr, len(layer_bytes)))


def texture_array_from_png(files):
    """Layers from encoded PNG files in material order, as Scene::loadSpecificTexture + createTextures: decode, pick the common size by
    the median rule, resize the layers that differ.  Returns (layers, size, size, 4) uint8."""
    layers = [decode_png(f) for f in files]
    for l in layers:
        if l.shape[0] != l.shape[1]:
            raise GmuptError("texture is not square")
    size = texture_common_size([l.size for l in layers])
    return np.stack([l if l.shape[0] == size else resize_square(l, size) for l in layers])


class SceneBuffers:
    """The six scene resources of Renderer::draw (t0-t4, b1) uploaded through gmupt_buffer_create."""

    def __init__(self, dev, scene):
        self.nodes = Buffer(dev, BUFFER_BVH_NODES, scene["nodes"])
        self.tris = Buffer(dev, BUFFER_TRIANGLES, scene["tris"])
        self.verts = Buffer(dev, BUFFER_VERTICES, scene["verts"])
        self.lights = Buffer(dev, BUFFER_LIGHTS, scene["lights"])
        self.props = Buffer(dev, BUFFER_TRI_PROPS, scene["props"])
        self.materials = Buffer(dev, BUFFER_MATERIALS, scene["materials"])
        self.textures = [TextureArray(dev, scene[k]) if scene.get(k) is not None else None
                         for k in ("tex_diffuse", "tex_metallic_roughness", "tex_normal")]

    def all(self):
        return [self.nodes, self.tris, self.verts, self.lights, self.props, self.materials]

    def close(self):
        for b in self.all():
            b.close()
        for t in self.textures:
            if t is not None:
                t.close()
