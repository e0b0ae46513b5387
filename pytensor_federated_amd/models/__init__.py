"""Worker-side model families (private-data logp+grad blackboxes)."""
from .base import LogpGradModel  # noqa: F401
from .glm import (  # noqa: F401
    GaussianGLMModel,
    PoissonGLMModel,
    generate_gaussian_glm_dataset,
    generate_poisson_dataset,
)
from .linear import GaussianLinearModel, generate_linear_dataset  # noqa: F401
from .logistic import LogisticGLMModel, generate_logistic_dataset  # noqa: F401
from .softmax import SoftmaxGLMModel, generate_softmax_dataset  # noqa: F401
from .ode import ODEModel, generate_ode_dataset, lotka_volterra_rhs  # noqa: F401
