"""c_orb_slam_amd -- MI355X-native ORB-SLAM2 per-frame hot path.

Host mirror (Python, over the C ABI of include/orbslam_gpu.h) of the reference
junejunejune/c_orb_slam classes on the hot path.  All compute runs in the HIP
library liborbslam_gpu.so (gfx950); there is no CPU fallback.
"""
from ._lib import KP_DTYPE, ORB_DEPTH_F32, ORB_DEPTH_U16, OrbGpuError, device_available, lib  # noqa: F401
from .orb import FeatureVector, Frame, MapPoints, ORBextractor, ORBmatcher  # noqa: F401
from .optimizer import (BundleAdjustment, LocalBundleAdjustment, OptimizeEssentialGraph,  # noqa: F401
                        OptimizeSim3, OptimizeSim3Batch, PoseOptimization, PoseOptimizationBatch)

__all__ = ["ORBextractor", "ORBmatcher", "Frame", "MapPoints", "KP_DTYPE", "OrbGpuError",
           "device_available", "lib"]
from .ransac import Initializer, PnPsolver, Rng, Sim3Solver  # noqa: F401
from .vocabulary import BowVector, ORBVocabulary  # noqa: F401
from .keyframe_database import KeyFrameDatabase  # noqa: F401
from .map import Map  # noqa: F401
from .loop_closing import LoopClosing  # noqa: F401
