"""augmentedgaussianprocesses.jl_amd -- MI355X-native engine for the SVGP + AnalyticVI/AnalyticSVI hot path of
AugmentedGaussianProcesses.jl, behind the reference's own API names (SVGP / train! / predict_y / ...).

The directory name contains a dot, so import it through the top-level alias module `agp_amd`
(`import agp_amd as AGP`), which loads this package under that name.

Host side mirrors the reference's Julia interface (same names, argument meaning, error behaviour); all numerics run
in hand-written HIP kernels behind the C ABI of include/agp_hip.h.  PyTorch is used only for device memory,
streams and torch.distributed (RCCL).
"""
from .kernels import (  # noqa: F401
    ARDTransform,
    ExponentialKernel,
    Matern32Kernel,
    Matern52Kernel,
    ScaleTransform,
    SqExponentialKernel,
    with_lengthscale,
)
from .likelihoods import (  # noqa: F401
    BayesianSVM,
    GaussianLikelihood,
    HeteroscedasticLikelihood,
    LaplaceLikelihood,
    LogisticLikelihood,
    LogisticSoftMaxLikelihood,
    SoftMaxLikelihood,
    NegBinomialLikelihood,
    PoissonLikelihood,
    StudentTLikelihood,
    loglikelihood,
)
from .svgp import (  # noqa: F401
    ADAM,
    Descent,
    Momentum,
    ELBO,
    elbo_streamed,
    MOSVGP,
    SVGP,
    AnalyticSVI,
    AnalyticVI,
    RobbinsMonro,
    MCIntegrationSVI,
    MCIntegrationVI,
    NumericalSVI,
    NumericalVI,
    QuadratureSVI,
    QuadratureVI,
    objective,
    objective_enqueue,
    objective_fetch,
    SideObjective,
    predict_f,
    predict_y,
    proba_y,
    train_,
)
from .vgp import VGP, n_latent  # noqa: F401
from .gp import GP, Analytic  # noqa: F401
from .movgp import MOVGP  # noqa: F401
from .mcgp import MCGP, GibbsSampling, sample, sample_local  # noqa: F401
from .nvi import gauss_hermite_rule, mc_expectations, mc_normals, quad_expectations  # noqa: F401
from .lpd import log_predictive_density, log_predictive_moments  # noqa: F401
from .predgrad import predict_f_grad  # noqa: F401
from .acquisition import (EI, PI, UCB, LogEI, LogPI, acquisition, acquisition_joint, acquisition_moments,  # noqa: F401
                          maximize_acquisition, maximize_acquisition_batch, maximize_acquisition_joint)
from .pathwise import PathwiseSamples, pathwise_features, sample_paths  # noqa: F401
from .capi import AGPError  # noqa: F401
from .persistence import load_trained_model, save_trained_model  # noqa: F401
from .inducingpoints import ConditionalVariance, KmeansAlg, RandomSubset, inducingpoints  # noqa: F401
from .online import (  # noqa: F401
    OIPS,
    OnlineSVGP,
    online_objective,
    online_predict_f,
    online_predict_y,
    online_proba_y,
    train_online,
)
