"""MI355X-native point+line local-BA / pose-optimisation / descriptor-matching core.

Only the hot path of alexandervakhitov/lld-slam lives here: hand-written HIP kernels for gfx950 behind the C ABI
of include/lld_amd.h (csrc/), plus the host-side mirror of the reference interface (host.py) and the synthetic
problem generators (synth.py).  There is no CPU fallback: everything that computes goes through
csrc/liblld_amd.so and fails loudly when the library or the GPU is missing.
"""
from . import abi  # noqa: F401
from .pnp import PnPsolver, PnPsolverBatch  # noqa: F401
from .sim3solver import Sim3Solver, Sim3SolverBatch  # noqa: F401
from .initializer import Initializer, InitializerError, problem_from_scene  # noqa: F401
from .landmarks import LandmarkError, distinctive_line_descriptors, refresh_map_points  # noqa: F401
from .new_points import NewPointsError, triangulate_new_points  # noqa: F401
from .covisibility import CovisibilityError, keyframe_culling, update_connections  # noqa: F401
from .loop_correction import LoopCorrectionError, apply_essential_graph, apply_global_ba, correct_loop  # noqa: F401
from .host import (BABatch, Context, Optimizer, ORBmatcher, PoseBatch, PoseFrame, Tracking, TwoFrameLineMatcher,  # noqa: F401
                   Window)

__all__ = ["abi", "Context", "Optimizer", "ORBmatcher", "TwoFrameLineMatcher", "Tracking", "BABatch", "PoseBatch", "Window",
           "PoseFrame", "PnPsolver", "PnPsolverBatch", "Sim3Solver", "Sim3SolverBatch", "Initializer", "InitializerError",
           "problem_from_scene", "refresh_map_points", "distinctive_line_descriptors", "LandmarkError",
           "triangulate_new_points", "NewPointsError", "update_connections", "keyframe_culling", "CovisibilityError",
           "correct_loop", "apply_essential_graph", "apply_global_ba", "LoopCorrectionError"]
