from .problem import (FFIProblem, GeodeticData, LogpForwFunc, ParameterLayout,  # noqa: F401
                      SeismicWavemap, prior_logp_func)
from .distributions import get_hyper_name, multivariate_normal_chol  # noqa: F401,E402
from .geometry import GeodeticGeometryProblem, los_vectors  # noqa: F401,E402
from .corrections import (EarthModel, EulerPoleConfig, EulerPoleCorrection, RampConfig,  # noqa: F401,E402
                          RampCorrection, StrainRateConfig, StrainRateCorrection)
from .hypers import HyperModel, dataset_hypers, estimate_hypers  # noqa: F401,E402
from .polarity import PolarityMap, PolarityProblem, polarity_hyper_name  # noqa: F401,E402
from .distributions import polarity_llk  # noqa: F401,E402
