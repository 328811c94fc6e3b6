"""pytorch3d.ops names the reference reaches (models/modules.py:9, models/nodes/smpl.py:14, utils/chamfer_distance.py:35)."""
from bilateral_driving_amd.p3d import knn_points  # noqa: F401
