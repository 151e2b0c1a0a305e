from .generic import get_kernel, KalmanSampler, DeviceChains
from .models import LGConcatModel, SVModel, LorenzModel, MVTModel, PoissonModel, PoissonLinearModel, BinomialModel, NegBinomialModel
from .._primitives.kalman.smoothing import smoothing, filter_smoothing

__all__ = ["get_kernel", "KalmanSampler", "DeviceChains", "LGConcatModel", "SVModel", "LorenzModel", "MVTModel", "PoissonModel", "PoissonLinearModel", "BinomialModel", "NegBinomialModel", "smoothing", "filter_smoothing"]
