"""Import surface of pytorch3d as used by bilateral-driving (ops.knn_points and four rotation conversions), served by
bilateral_driving_amd.p3d.  pytorch3d itself has no ROCm build."""
__version__ = "0.7.5+bds.gfx950"
