"""Mesh updates on the device: smooth vertex normals (Normals) and skinning / morph targets (Pose), with their rules on the CPU."""
import ctypes as C

import numpy as np

from ._abi import ERR_INVALID_ARGUMENT, GmuptError, NormalsInfo, PoseInfo, _info_dict
from ._lib import _check, _ptr, lib
from ._stage import Handle, device_tensor, torch_device


class Normals(Handle):
    """gmupt_normals: smooth vertex normals of one index list, recomputed on the GPU from the vertex buffer the renderer is bound to and
    written into the `normal` field of its property records (include/gmupt.h "normals" states the rule).  indices: (n, 3) int32, a numpy
    array (uploaded) or a torch device tensor (used in place; the handle keeps its own copy).  It uses the renderer's device and stream
    and is closed with it at the latest."""
    _destroy, _siblings = "gmupt_normals_destroy", "_normals"

    def __init__(self, renderer, indices):
        torch, device = torch_device(renderer.dev)
        idx = device_tensor(indices, device, np.int32, None, lambda t: t.device == device and t.dtype == torch.int32,
                            "Normals: an index tensor must be int32 on %s" % device).reshape(-1)
        self.renderer = renderer
        torch.cuda.current_stream(device).synchronize()
        self._open(renderer, "gmupt_normals_create", C.c_void_p(idx.data_ptr()) if idx.numel() else None, idx.numel() // 3)

    def update(self, info=False):
        """gmupt_normals_update on the renderer's stream.  info=False: no host synchronisation, returns None.  info=True: synchronises
        and returns the gmupt_normals_info fields as a dict (ms = device time of the two launches)."""
        if not info:
            _check(lib().gmupt_normals_update(self.h, None))
            return None
        ni = NormalsInfo()
        _check(lib().gmupt_normals_update(self.h, C.byref(ni)))
        return _info_dict(ni)


def vertex_normals_host(verts, indices, threads=16):
    """gmupt_vertex_normals_host: the smooth-normal rule of include/gmupt.h on the CPU in binary32, bit for bit what Normals.update()
    writes.  verts (V, 3) float32, indices (n, 3) int32.  Returns (V, 3) float32."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    out = np.empty_like(verts)
    _check(lib().gmupt_vertex_normals_host(_ptr(verts), verts.shape[0], _ptr(indices), indices.shape[0], _ptr(out), int(threads)))
    return out


def _rig_arrays(rest, joints, weights, num_joints, deltas):
    """The arrays of a rig as contiguous numpy arrays of the C-ABI's types (None where the rule ignores them) and V, K, J, T."""
    rest = np.ascontiguousarray(rest, dtype=np.float32).reshape(-1, 3)
    V, J = rest.shape[0], int(num_joints)
    K = 0
    if J:
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(V, -1) if V else np.zeros((0, 1), np.float32)
        K = weights.shape[1]
        joints = np.ascontiguousarray(joints, dtype=np.uint16).reshape(V, K)
    else:
        joints = weights = None
    deltas = None if deltas is None else np.ascontiguousarray(deltas, dtype=np.float32).reshape(-1, V, 3)
    T = 0 if deltas is None else deltas.shape[0]
    return rest, joints, weights, (deltas if T else None), V, K, J, T


class Pose(Handle):
    """gmupt_pose: the rig of one mesh -- rest positions, skinning influences, dense morph targets -- kept on the GPU, and update(), which
    writes the posed vertices into the vertex buffer the renderer is bound to (include/gmupt.h "Pose" states the rule).  rest (V, 3)
    float32, joints (V, K) uint16, weights (V, K) float32, deltas (T, V, 3) float32 or None; each a numpy array (uploaded) or a torch
    device tensor of that dtype (used in place; the handle keeps its own copies).  num_joints = 0: morph only, joints and weights are
    ignored.  It uses the renderer's device and stream and is closed with it at the latest."""
    _destroy, _siblings = "gmupt_pose_destroy", "_poses"

    def __init__(self, renderer, rest, joints, weights, num_joints, deltas=None):
        torch, device = torch_device(renderer.dev)
        J = int(num_joints)

        def dev(a, what):
            if a is None:
                return None
            return device_tensor(a, device, np.float32, None, lambda t: t.device == device and t.dtype == torch.float32,
                                 "Pose: a %s tensor must be %s on %s" % (what, torch.float32, device))

        rest = dev(rest, "rest")
        weights = dev(weights, "weights") if J else None
        if J and not isinstance(joints, torch.Tensor):
            joints = np.ascontiguousarray(joints, dtype=np.uint16).view(np.int16)   # (the bits: torch need not have a uint16)
        joints = device_tensor(joints, device, np.int16, None,
                               lambda t: t.device == device and t.dtype in (getattr(torch, "uint16", torch.int16), torch.int16),
                               "Pose: a joints tensor must be uint16 (or its bits as int16) on %s" % device) if J else None
        deltas = dev(deltas, "deltas")
        V = rest.numel() // 3
        K = (weights.numel() // V if V else 0) if J else 0
        T = deltas.numel() // (3 * V) if (deltas is not None and V) else 0
        if J and (weights.numel() != V * K or joints.numel() != V * K):
            raise GmuptError("Pose: joints and weights must hold the same number of influences for each of the %d vertices" % V, ERR_INVALID_ARGUMENT)
        if deltas is not None and deltas.numel() != T * V * 3:
            raise GmuptError("Pose: deltas must hold 3 floats per vertex and target", ERR_INVALID_ARGUMENT)
        self.renderer = renderer
        self.num_verts, self.influences, self.num_joints, self.num_targets = V, K, J, T
        self._device = device
        self._pending = []     # device tensors of update() calls the stream may not have read yet
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        torch.cuda.current_stream(device).synchronize()
        self._open(renderer, "gmupt_pose_create", p(rest), p(joints), p(weights), K, J, p(deltas) if T else None, T)

    def update(self, joint_mats, target_weights=None, info=False):
        """gmupt_pose_update (numpy / host arrays) or gmupt_pose_update_device (joint_mats a torch device tensor; target_weights then a
        device tensor too, or a host array that is uploaded first) on the renderer's stream.  joint_mats: (J, 12) float32, None for a
        morph-only rig; target_weights: (T,) float32, None = all zero.  info=False: no host synchronisation, returns None.  info=True:
        synchronises and returns the gmupt_pose_info fields as a dict (ms = device time of the copies and the two launches).  Device
        tensors are kept referenced until a synchronising call has shown that the stream is past them."""
        J, T = self.num_joints, self.num_targets
        pi = PoseInfo() if info else None
        on_device = hasattr(joint_mats, "is_cuda") or hasattr(target_weights, "is_cuda")
        if on_device:
            import torch

            def dev(a, n, what):
                if n == 0:
                    return None
                if a is None:
                    return torch.zeros(n, dtype=torch.float32, device=self._device)
                if not isinstance(a, torch.Tensor):
                    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                if a.dtype != torch.float32 or a.numel() != n:
                    raise GmuptError("Pose.update: %s must hold %d float32" % (what, n), ERR_INVALID_ARGUMENT)
                if a.device != self._device:
                    if a.is_cuda:
                        raise GmuptError("Pose.update: %s is on %s, the renderer on %s" % (what, a.device, self._device), ERR_INVALID_ARGUMENT)
                    a = a.to(self._device)
                return a.contiguous()

            jm, tw = dev(joint_mats, 12 * J, "joint_mats"), dev(target_weights, T, "target_weights")
            torch.cuda.current_stream(self._device).synchronize()
            if len(self._pending) >= 64:
                self.renderer.synchronize(); self._pending.clear()
            self._pending.append((jm, tw))
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            _check(lib().gmupt_pose_update_device(self.h, p(jm), p(tw), C.byref(pi) if info else None))
        else:
            jm = None if J == 0 else np.ascontiguousarray(joint_mats, dtype=np.float32).reshape(-1)
            tw = None if T == 0 else (np.zeros(T, np.float32) if target_weights is None else np.ascontiguousarray(target_weights, dtype=np.float32).reshape(-1))
            if (J and jm.size != 12 * J) or (T and tw.size != T):
                raise GmuptError("Pose.update: %d joints need %d matrix floats, %d targets %d weights" % (J, 12 * J, T, T), ERR_INVALID_ARGUMENT)
            _check(lib().gmupt_pose_update(self.h, _ptr(jm) if J else None, _ptr(tw) if T else None, C.byref(pi) if info else None))
        if not info:
            return None
        self._pending.clear()                                    # the call has synchronised the stream
        return _info_dict(pi)

    def close(self):
        Handle.close(self)                                       # gmupt_pose_destroy synchronises the stream
        self._pending = []


def pose_host(rest, joints, weights, num_joints, joint_mats, deltas=None, target_weights=None, threads=16):
    """gmupt_pose_host: the pose rule of include/gmupt.h on the CPU in binary32, bit for bit what Pose.update() writes.  Arrays as for
    Pose and Pose.update (numpy).  Returns (V, 3) float32."""
    rest, joints, weights, deltas, V, K, J, T = _rig_arrays(rest, joints, weights, num_joints, deltas)
    jm = np.ascontiguousarray(joint_mats, dtype=np.float32).reshape(-1) if J else None
    if J and jm.size != 12 * J:
        raise GmuptError("pose_host: %d joints need %d matrix floats" % (J, 12 * J), ERR_INVALID_ARGUMENT)
    tw = None
    if T:
        tw = np.zeros(T, np.float32) if target_weights is None else np.ascontiguousarray(target_weights, dtype=np.float32).reshape(-1)
        if tw.size != T:
            raise GmuptError("pose_host: %d targets need %d weights" % (T, T), ERR_INVALID_ARGUMENT)
    out = np.empty_like(rest)
    p = lambda a: _ptr(a) if a is not None else None
    _check(lib().gmupt_pose_host(p(rest), V, p(joints), p(weights), K, p(jm), J, p(deltas), p(tw), T, _ptr(out), int(threads)))
    return out
