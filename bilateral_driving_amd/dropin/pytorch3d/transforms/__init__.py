"""pytorch3d.transforms names the reference reaches (models/gaussians/basics.py:10, models/human_body.py:12-16, models/nodes/smpl.py,
rigid.py:187, datasets/tools/postprocess.py:6 and the dataset loaders)."""
from bilateral_driving_amd.p3d import (  # noqa: F401
    axis_angle_to_matrix, matrix_to_quaternion, quaternion_to_matrix, standardize_quaternion)
