"""foundationpose_cpp_amd -- MI355X-native FoundationPose Register/Track hot path."""
from .api import BOP19_TAUS, DepthRefine, DepthRegister, FoundationPose, FoundationPoseError, PoseError, PoseColor, PoseFit, PoseSearch, PoseSilhouette, PoseVsd, SilhouetteRefine, auc, load_mesh, recall, vsd_recall  # noqa: F401
