from .base import LGSSM, posterior_logpdf, log_likelihood, prior_logpdf, joint_logpdf
from .filtering import filtering
from .sampling import sampling
from .smoothing import smoothing, filter_smoothing
from .em import smoothing_lag_one, fit_em

__all__ = ["LGSSM", "posterior_logpdf", "log_likelihood", "prior_logpdf", "joint_logpdf", "filtering", "sampling", "smoothing", "filter_smoothing",
           "smoothing_lag_one", "fit_em"]
