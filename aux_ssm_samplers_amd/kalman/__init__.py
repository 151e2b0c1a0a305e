from .generic import get_kernel, KalmanSampler, DeviceChains
from .models import LGConcatModel, SVModel, LorenzModel, MVTModel

__all__ = ["get_kernel", "KalmanSampler", "DeviceChains", "LGConcatModel", "SVModel", "LorenzModel", "MVTModel"]
