"""Acceleration structures: refit on the host, the traversal tables of a tree, the SBVH and LBVH builders, the tree cost and the treelet
optimiser -- the host functions, and the device handles TreeOptimizer and Lbvh."""
import ctypes as C

import numpy as np

from ._abi import (_P, TRAVTABLE_KINDS, GmuptError, LbvhInfo, LbvhParams, SbvhParams, TreeCostInfo, TreeoptInfo, TreeoptParams,
                   bvh_node_dtype, triangle_dtype)
from ._lib import _check, _ptr, lib
from ._stage import Handle, device_tensor, torch_device
from .device import Buffer


def bvh_refit_host(nodes, tris, verts, threads=16):
    """gmupt_bvh_refit_host on a copy: the nodes with the boxes of the given vertices, topology untouched."""
    out = np.array(nodes, dtype=bvh_node_dtype, copy=True)
    tris = np.ascontiguousarray(tris, dtype=triangle_dtype)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    _check(lib().gmupt_bvh_refit_host(_ptr(out), out.shape[0], _ptr(tris), tris.shape[0], _ptr(verts), verts.shape[0], threads))
    return out


def travtables(nodes, tris, verts, want_wide=True, top_order_bfs=False, node_pairing=True):
    """gmupt_debug_travtables_*: the traversal tables and refit maps a bind would build from these host arrays, no device involved.
    Returns {kind: uint8 array (a copy)} for TRAVTABLE_KINDS."""
    nodes = np.ascontiguousarray(nodes); tris = np.ascontiguousarray(tris)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    h = _P()
    _check(lib().gmupt_debug_travtables_build(_ptr(nodes), nodes.shape[0], _ptr(tris), tris.shape[0], _ptr(verts), verts.shape[0],
                                              int(want_wide), int(top_order_bfs), int(node_pairing), C.byref(h)))
    try:
        out = {}
        for which, kind in enumerate(TRAVTABLE_KINDS):
            n = C.c_size_t(0)
            p = lib().gmupt_debug_travtables_data(h, which, C.byref(n))
            out[kind] = np.frombuffer(C.string_at(p, n.value), np.uint8).copy() if p and n.value else np.zeros(0, np.uint8)
        return out
    finally:
        lib().gmupt_debug_travtables_destroy(h)


def wide_tables_addressable(wide_nodes, num_tris, num_pairs):
    """gmupt_debug_wide_tables_addressable: do tables of these sizes stay within the wide ray cast's 32-bit byte offsets?  No device involved."""
    return bool(lib().gmupt_debug_wide_tables_addressable(int(wide_nodes), int(num_tris), int(num_pairs)))


def sbvh_build(verts, indices, vertex_material=None, params=None):
    """Host SBVH build + flatten (gmupt_sbvh_*).  Returns dict(nodes, tris, ref_triangle, sah, depth)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    h = _P()
    pp = None
    if params is not None:
        pp = SbvhParams()
        lib().gmupt_sbvh_default_params(C.byref(pp))
        for k, v in params.items():
            setattr(pp, k, v)
        pp = C.byref(pp)
    _check(lib().gmupt_sbvh_build(_ptr(verts), verts.shape[0], _ptr(indices), indices.shape[0], pp, C.byref(h)))
    try:
        n = lib().gmupt_sbvh_num_nodes(h)
        nr = lib().gmupt_sbvh_num_references(h)
        nodes = np.zeros(n, dtype=bvh_node_dtype)
        vm = np.ascontiguousarray(vertex_material, dtype=np.uint32) if vertex_material is not None else None
        tris_buf = np.zeros(max(nr, 1), dtype=triangle_dtype)
        ref_buf = np.zeros(max(nr, 1), dtype=np.int32)
        _check(lib().gmupt_sbvh_flatten(h, _ptr(vm) if vm is not None else None, _ptr(nodes), _ptr(tris_buf), _ptr(ref_buf)))
        tris, ref = tris_buf[:nr], ref_buf[:nr]
        return {"nodes": nodes, "tris": tris, "ref_triangle": ref, "sah": float(lib().gmupt_sbvh_sah(h)), "depth": int(lib().gmupt_sbvh_depth(h))}
    finally:
        lib().gmupt_sbvh_destroy(h)


def lbvh_build_host(verts, indices, vertex_material=None, max_leaf_size=4):
    """gmupt_lbvh_build_host: the LBVH rule of include/gmupt.h on host arrays, the reference of Lbvh.build.  Returns the dict of sbvh_build
    (nodes, tris, ref_triangle, sah, depth) plus info (LbvhInfo.as_dict()); sah is the surface-area cost of the tree with the SBVH builder's
    default node / triangle costs of 1 (tree_sah)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    n = indices.shape[0]
    vm = np.ascontiguousarray(vertex_material, dtype=np.uint32) if vertex_material is not None else None
    if vm is not None and vm.shape[0] < verts.shape[0]:
        raise GmuptError("lbvh_build_host: %d vertex materials for %d vertices" % (vm.shape[0], verts.shape[0]), -1)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=bvh_node_dtype)
    tris = np.zeros(max(n, 1), dtype=triangle_dtype)
    ref = np.zeros(max(n, 1), dtype=np.int32)
    pp, info = LbvhParams(int(max_leaf_size)), LbvhInfo()
    _check(lib().gmupt_lbvh_build_host(_ptr(verts), verts.shape[0], _ptr(indices), n, _ptr(vm) if vm is not None else None, C.byref(pp),
                                       _ptr(nodes), _ptr(tris), _ptr(ref), C.byref(info)))
    nodes = nodes[:info.num_nodes].copy()
    return {"nodes": nodes, "tris": tris[:n], "ref_triangle": ref[:n], "sah": tree_sah(nodes), "depth": int(info.depth), "info": info.as_dict()}


def tree_sah(nodes):
    """Surface-area cost of a reference-layout tree: A(node) / A(root) times 2 for an inner node (two box tests) and times the number of
    references for a leaf -- the measure gmupt_sbvh_sah reports at its default costs of 1, from the flattened boxes in float64 instead of
    the builder's running float products.  0 for a root without area."""
    nodes = np.asarray(nodes)
    e = np.maximum(nodes["max"].astype(np.float64) - nodes["min"].astype(np.float64), 0.0)
    area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    if not area[0] > 0:
        return 0.0
    leaf = nodes["isLeaf"] != 0
    count = np.where(leaf, nodes["right"] - nodes["left"], 2)
    return float((area * count).sum() / area[0])


def tree_cost_host(nodes, threads=16):
    """gmupt_tree_cost_host: the tree-cost rule of include/gmupt.h on the CPU, bit for bit what Renderer.tree_cost() returns for the same
    records (ms = 0).  nodes: an array of bvh_node_dtype; any records do, no link is followed.  The thread count changes no bit."""
    nodes = np.ascontiguousarray(nodes, dtype=bvh_node_dtype)
    ti = TreeCostInfo()
    _check(lib().gmupt_tree_cost_host(_ptr(nodes), nodes.shape[0], C.byref(ti), int(threads)))
    return ti.as_dict()


def tree_optimize_host(nodes, passes=3):
    """gmupt_tree_optimize_host: the treelet optimiser of include/gmupt.h ("Tree optimisation") on the CPU, bit for bit what
    TreeOptimizer.run returns for the same records.  Returns (nodes, info dict); ms = 0."""
    nodes = np.ascontiguousarray(nodes, dtype=bvh_node_dtype)
    out = np.zeros(max(nodes.shape[0], 1), dtype=bvh_node_dtype)[:nodes.shape[0]]
    pp, info = TreeoptParams(int(passes)), TreeoptInfo()
    _check(lib().gmupt_tree_optimize_host(_ptr(nodes), nodes.shape[0], C.byref(pp), _ptr(out), C.byref(info)))
    return out, info.as_dict()


class TreeOptimizer(Handle):
    """gmupt_treeopt: the GPU treelet optimiser of one device -- a stream and the scratch of the largest tree optimised so far."""
    _destroy = "gmupt_treeopt_destroy"

    def __init__(self, dev):
        self.dev = dev
        self._open(dev, "gmupt_treeopt_create")

    def run(self, nodes, passes=3):
        """gmupt_treeopt_run on `nodes`, a Buffer of kind BUFFER_BVH_NODES (left as it is).  Returns (a new nodes Buffer the caller closes,
        info dict)."""
        out, info = _P(), TreeoptInfo()
        pp = TreeoptParams(int(passes))
        _check(lib().gmupt_treeopt_run(self.h, nodes.h, C.byref(pp), C.byref(out), C.byref(info)))
        return Buffer.wrap(self.dev, out), info.as_dict()


class Lbvh(Handle):
    """gmupt_lbvh: the GPU LBVH builder of one device -- a stream and the scratch of the largest mesh built so far, kept between builds."""
    _destroy = "gmupt_lbvh_destroy"

    def __init__(self, dev):
        self.dev = dev
        self._open(dev, "gmupt_lbvh_create")
        self.optimizer = None     # the TreeOptimizer of build(optimize=...), created by the first such build

    def build(self, vertex_buffer, indices, vertex_material=None, max_leaf_size=4, ref_triangle=False, optimize=0):
        """gmupt_lbvh_build on the device-resident vertices of `vertex_buffer` (a Buffer of kind BUFFER_VERTICES).  indices / vertex_material:
        torch device tensors (int32 / a 4-byte integer type, used in place) or numpy arrays (uploaded).  Returns (nodes Buffer, tris Buffer,
        info dict); the caller closes the buffers.  ref_triangle=True adds info["ref_triangle"], the source triangle of every record.
        optimize=N > 0 runs N passes of the treelet optimiser (TreeOptimizer.run) on the new tree: the nodes Buffer is the optimised one,
        info["optimize"] its info dict and info["depth"] the new depth; an optimiser error (a tree that became too deep) is raised and no
        buffer is left behind."""
        torch, device = torch_device(self.dev)

        def on_device(x, dtype):
            if not isinstance(x, torch.Tensor):
                x = np.ascontiguousarray(x, dtype=dtype).view(np.int32)     # (the bits; torch has no arithmetic on uint32 and needs none here)
            return device_tensor(x, device, np.int32, None, lambda t: t.device == device and t.element_size() == 4 and not t.is_floating_point(),
                                 "Lbvh.build: a tensor must hold 4-byte integers on %s" % device)

        idx = on_device(indices, np.int32).reshape(-1)
        n = idx.numel() // 3
        vm = on_device(vertex_material, np.uint32).reshape(-1) if vertex_material is not None else None
        nverts = int(lib().gmupt_buffer_size(vertex_buffer.h)) // 12
        if vm is not None and vm.numel() < nverts:
            raise GmuptError("Lbvh.build: %d vertex materials for %d vertices" % (vm.numel(), nverts), -1)
        ref = torch.empty(max(n, 1), dtype=torch.int32, device=device) if ref_triangle else None
        torch.cuda.synchronize(device)    # the builder has its own stream: uploads and the caller's writes are done before it starts
        nodes, tris, info = _P(), _P(), LbvhInfo()
        pp = LbvhParams(int(max_leaf_size))
        _check(lib().gmupt_lbvh_build(self.h, vertex_buffer.h, idx.data_ptr(), n, vm.data_ptr() if vm is not None else None, C.byref(pp),
                                      C.byref(nodes), C.byref(tris), ref.data_ptr() if ref is not None else None, C.byref(info)))
        out = info.as_dict()
        if ref is not None:
            out["ref_triangle"] = ref[:n].cpu().numpy()
        nodes, tris = Buffer.wrap(self.dev, nodes), Buffer.wrap(self.dev, tris)
        if optimize:
            if self.optimizer is None:
                self.optimizer = TreeOptimizer(self.dev)
            try:
                better, out["optimize"] = self.optimizer.run(nodes, passes=optimize)
            except GmuptError:
                tris.close()
                raise
            finally:
                nodes.close()
            nodes = better
            out["depth"] = out["optimize"]["depth_after"]
        return nodes, tris, out

    def close(self):
        if self.optimizer is not None:
            self.optimizer.close()
            self.optimizer = None
        Handle.close(self)
