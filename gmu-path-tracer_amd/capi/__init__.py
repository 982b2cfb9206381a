"""ctypes binding of libgmupt.so -- the binding a Python host would add on top of include/gmupt.h.

This is plumbing only: every call goes straight to the C-ABI, there is no CPU fallback.  If the HIP library is missing or a HIP call
fails, GmuptError is raised with gmupt_last_error().

One module per feature, like csrc/gmupt_capi_*.hip, each re-exported here so that callers write capi.NAME: _abi (the C-ABI's types and
SYMBOLS), _lib (the loaded library, its only owner), _stage (what the rest shares), device, then the feature modules query, denoise,
converge, mesh and accel, then core (Camera, Renderer), which imports the feature modules and is imported by none of them.

adaptive (adaptive sampling) is the exception: it is reached as capi.adaptive.NAME and keeps its structures and prototypes itself, so
that the names at this level, the Renderer class and SYMBOLS stay the recorded surface (tests/golden/capi_surface.json).  lens (the
thin lens, capi.lens.NAME) follows it, and so do lens_aov (the lens-filtered AOV planes, capi.lens_aov.NAME), projection (the camera
projections, capi.projection.NAME) and shutter (camera motion blur, capi.shutter.NAME).
"""
from ._abi import *  # noqa: F401,F403
from ._lib import _check, _ptr, lib, use_build  # noqa: F401
from .device import (Buffer, Device, SceneBuffers, TextureArray, decode_png, resize_square, texture_array_from_png,  # noqa: F401
                     texture_common_size)
from .query import aov_fields, aov_ray, aov_rays, camera_pick_ray, hit_fields, motion_fields, motion_host  # noqa: F401
from .denoise import (TEMPORAL_FIELDS, Temporal, denoise_host, denoise_image, denoise_params, infill_host, infill_image,  # noqa: F401
                      infill_params, temporal_denoise_image, temporal_integrate_host, temporal_integrate_motion_host, temporal_params)
from .converge import Converge, converge_host, converge_params  # noqa: F401
from .mesh import Normals, Pose, pose_host, vertex_normals_host  # noqa: F401
from .accel import (Lbvh, TreeOptimizer, bvh_refit_host, lbvh_build_host, sbvh_build, travtables, tree_cost_host,  # noqa: F401
                    tree_optimize_host, tree_sah, wide_tables_addressable)
from .core import Camera, Renderer  # noqa: F401
from . import adaptive  # noqa: F401,E402
from . import lens  # noqa: F401,E402
from . import lens_aov  # noqa: F401,E402
from . import projection  # noqa: F401,E402
from . import shutter  # noqa: F401,E402
