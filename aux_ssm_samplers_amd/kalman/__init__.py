from .generic import get_kernel, KalmanSampler, DeviceChains
from .models import LGConcatModel, SVModel, LorenzModel, MVTModel, PoissonModel, PoissonLinearModel, BinomialModel, NegBinomialModel, BinomialLinearModel, NegBinomialLinearModel
from .._primitives.kalman.smoothing import smoothing, filter_smoothing

__all__ = ["get_kernel", "KalmanSampler", "DeviceChains", "LGConcatModel", "SVModel", "LorenzModel", "MVTModel", "PoissonModel", "PoissonLinearModel", "BinomialModel", "NegBinomialModel", "BinomialLinearModel", "NegBinomialLinearModel", "smoothing", "filter_smoothing"]
