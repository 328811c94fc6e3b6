"""bilateral-driving's hot path on MI355X.  The modules are imported by name (``from bilateral_driving_amd import rendering``); the
ones listed here are also reachable as attributes of the package, imported on first use."""
import importlib

__all__ = ["metrics", "geometry", "init", "lidar", "pseudo_lidar", "pixels", "sampler", "video", "undistort"]


def __getattr__(name):
    if name in __all__:
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
