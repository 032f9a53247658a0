"""lanefront: MI355X-native line-feature front end for lane-slam (detect, describe,
ground-project, sanity-filter, associate) behind a C ABI (include/lanefront.h).

The package is a thin host-side mirror of the reference's interfaces for this path:
  LineDetectorHIP  <->  line_detector.LineDetectorLSD (LineDetectorInterface plugin)
  LineDetectorHSV  <->  line_detector.LineDetectorHSV: the same plugin with cv2.HoughLinesP in place of LSD (LF_DETECTOR_HOUGH)
  LineDetector2Dense <-> line_detector.LineDetector2Dense: a line per steep-gradient edge pixel (LF_DETECTOR_DENSE)
  LineDetectorEDLines   the same plugin interface over the line_descriptor library's EDLines detector; FrontEnd.keylines_batch /
                        describe_keylines <-> BinaryDescriptor::detect / compute with octaves
  LineAssociator   <->  line_associator node (a stub in the reference) + show_map's segment store: device-resident
                        live map, MFMA Hamming association, colour gating, append / merge updates (lf_map_*)
  PoseGraph             loop closures: key poses, odometry and loop edges, solved on the device (LineAssociator.graph_solve)
                        and applied to the map (LineAssociator.correct)
  BinaryDescriptorMatcher <-> the matcher's dataset form (add / train / match / knnMatch / radiusMatch over several train images, imgIdx)
  LaneFilterHistogram <-> lane_filter.LaneFilterHistogram: the histogram lane filter (lane pose from ground segments) on the
                        device; LaneFilterBatch runs many filter streams over a FrontEnd batch's segments
  OdometryNode     <->  odometry.OdometryNode: wheel commands to the `map -> duck` pose; Odometry integrates a whole log's commands
                        for many robots in one call and samples the poses at the frames' stamps (include/lanefront_odometry.h)
  FrameMotion           the relative motion between frames of a batch from their own segments and LBD codes, with no map: match,
                        hypothesis search and Gauss-Newton refinement for many pairs in one launch (include/lanefront_motion.h)
  KeyFrames             a store of key frames on the device across batches: which stored places a frame looks like (loop-closure
                        candidates), and the frame's motion against a stored key (include/lanefront_places.h)
  FrontEnd         <->  batch form of line_detector_node / ground_projection_node /
                        line_sanity_node callbacks + BinaryDescriptor / BinaryDescriptorMatcher
There is no CPU fallback: importing works anywhere, but creating a detector without the
HIP library or without a GPU raises.
"""
from .config import (COLOR_NAMES, DEFAULT_DETECTOR_CONFIGURATION, RED, WHITE, YELLOW, default_config)
from .frontend import FrontEnd, LanefrontError, Segments
from .lane_filter import LaneFilterBatch, LaneFilterHistogram
from .line_associator import LineAssociator
from .motion import FrameMotion
from .odometry import Odometry, OdometryNode
from .places import KeyFrames
from .pose_graph import PoseGraph
from .matcher import BinaryDescriptorMatcher, BinaryDescriptorParams, DMatch
from .line_detector_hip import Detections, LineDetector2Dense, LineDetectorEDLines, LineDetectorHIP, LineDetectorHSV, LineDetectorInterface

__all__ = ["LaneFilterBatch", "LaneFilterHistogram", "FrameMotion", "KeyFrames", "Odometry", "OdometryNode", "BinaryDescriptorMatcher", "BinaryDescriptorParams", "DMatch", "LineAssociator", "PoseGraph", "FrontEnd", "LanefrontError", "Segments", "LineDetectorHIP", "LineDetectorHSV", "LineDetector2Dense", "LineDetectorEDLines", "LineDetectorInterface", "Detections",
           "default_config", "DEFAULT_DETECTOR_CONFIGURATION", "WHITE", "YELLOW", "RED", "COLOR_NAMES"]
