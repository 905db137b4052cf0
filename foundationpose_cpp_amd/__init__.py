"""foundationpose_cpp_amd -- MI355X-native FoundationPose Register/Track hot path."""
from .api import FoundationPose, FoundationPoseError, PoseError, PoseFit, auc, load_mesh, recall  # noqa: F401
