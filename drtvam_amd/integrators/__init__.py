from .common import TVAMIntegrator
from .volume import VolumeIntegrator, integrators
from .corner import CornerIntegrator

__all__ = ["TVAMIntegrator", "VolumeIntegrator", "CornerIntegrator", "integrators"]
