"""pyopenvino_amd: MI355X (gfx950) back end for the pyopenvino per-layer ``compute()`` hot path.

``inference_engine`` mirrors the reference's IECore / IENetwork / Executable_Network; ``op_plugins``
holds one module per IR layer type exposing ``compute(node, inputs, kernel_type, debug)`` whose numeric
body is a hand-written HIP kernel reached through the C ABI of ``libpvhip.so`` (``include/pvhip.h``).
"""
from .inference_engine import IECore, IENetwork, Executable_Network  # noqa: F401
from .detections import Detections, DetectionScreen  # noqa: F401
from .gallery import Gallery, GalleryMatch, Matches  # noqa: F401
from .keypoints import Keypoints, PeakScreen  # noqa: F401
from .segments import Segments, SegmentScreen  # noqa: F401
from .maxima import Maxima, MaximaScreen  # noqa: F401
from . import text  # noqa: F401
from .text import Text, TextScreen  # noqa: F401
from . import boxes  # noqa: F401
from .boxes import BoxScreen  # noqa: F401
from .input_format import DetectedRois, LandmarkWarps, PerspectiveInput, RoiInput, WarpInput  # noqa: F401
from .tiled_detections import RegionScreen, TiledScreen  # noqa: F401
from .top_k import TopK  # noqa: F401

__all__ = ['IECore', 'IENetwork', 'Executable_Network', 'RoiInput', 'WarpInput', 'PerspectiveInput', 'DetectedRois', 'LandmarkWarps', 'TopK', 'Detections', 'DetectionScreen', 'TiledScreen', 'RegionScreen', 'Gallery', 'GalleryMatch', 'Matches', 'PeakScreen', 'Keypoints', 'SegmentScreen', 'Segments', 'MaximaScreen', 'Maxima', 'TextScreen', 'Text', 'text', 'BoxScreen', 'boxes']
