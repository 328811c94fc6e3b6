"""pytorch3d.ops.knn.knn_points (the path some of the reference's tools import it by)."""
from bilateral_driving_amd.p3d import knn_points  # noqa: F401
