"""gaussian_process_optimization_amd -- MI355X-native exact-GP regression hot path.

Drop-in surface for the path GPyOpt/GPy sit on:

    import gaussian_process_optimization_amd as gpo
    m = gpo.models.GPRegression(X, Y, gpo.kern.RBF(D), noise_var=1e-2)   # GPy.models.GPRegression
    m.log_likelihood(); m.predict(Xs); m.predictive_gradients(Xs); m.optimize()
    bo = gpo.methods.BayesianOptimization(f=None, domain=..., X=X, Y=Y)  # GPyOpt.methods
    mw = gpo.models.InputWarpedGP(X, Y, gpo.kern.Matern52(D))            # GPy.models.InputWarpedGP (Kumaraswamy warping)
    mo = gpo.models.WarpedGP(X, Y, gpo.kern.Matern32(D))                 # GPy.models.WarpedGP (tanh warp of the outputs)
    ms = gpo.models.SparseGPRegression(X, Y, num_inducing=128)           # GPy.models.SparseGPRegression (variational DTC)
    mm = gpo.GPModel_MCMC(n_samples=10)                                  # GPyOpt.models.GPModel_MCMC (HMC over the hyper-parameters)
    acq = gpo.acquisitions.AcquisitionEI(gpo.GPModel(...), ...)           # GPyOpt.acquisitions

Host code is plain Python + ctypes over the C-ABI in include/gphip.h; every
numeric step runs in hand-written HIP kernels for gfx950 (csrc/).  There is no
CPU fallback: importing the package works anywhere, using it needs an MI355X.
"""
import types as _types

from . import _lib
from . import kern
from . import mappings
from .gp_regression import GPRegression, Gaussian, Standardize
from .sparse_gp import SparseGPRegression
from .gpmodel import GPModel, BOModel, GPModel_MCMC, GPClassModel
from .gp_classification import GPClassification, Bernoulli
from . import priors
from .mcmc import HMC
from . import input_warping
from .input_warped_gp import InputWarpedGP, InputWarpedGPModel
from . import warping_functions
from .warped_gp import WarpedGP, WarpedGPModel
from . import cost
from .cost import CostModel
from . import feasibility
from .feasibility import FeasibilityModel
from . import acquisitions
from .acquisitions import (AcquisitionEI, AcquisitionLCB, AcquisitionMPI, AcquisitionBase, AcquisitionLP,
                           LocalPenalization, estimate_L, AcquisitionEI_MCMC, AcquisitionMPI_MCMC, AcquisitionLCB_MCMC,
                           AcquisitionEntropySearch, AcquisitionMES, AcquisitionTS)
from . import joint_ei
from .joint_ei import AcquisitionQEI, JointBatch
from . import knowledge_gradient
from .knowledge_gradient import AcquisitionKG
from . import noisy_ei
from .noisy_ei import AcquisitionNEI
from . import posterior_paths
from .posterior_paths import PosteriorPaths
from . import max_value
from .max_value import MinValueSampler
from . import entropy_search
from .entropy_search import McmcSampler, AffineInvariantEnsembleSampler
from .bayesian_optimization import BayesianOptimization, Design_space, AcquisitionOptimizer
from .sharded import ShardedCandidates, merge_best
from . import multi_objective
from .multi_objective import (AcquisitionEHVI, MultiObjectiveBayesianOptimization, pareto_front, hypervolume,
                              nondominated_cells)

# namespaces named like the reference packages
models = _types.SimpleNamespace(GPRegression=GPRegression, GPClassification=GPClassification, GPClassModel=GPClassModel, SparseGPRegression=SparseGPRegression, GPModel=GPModel, GPModel_MCMC=GPModel_MCMC, InputWarpedGP=InputWarpedGP,
                                InputWarpedGPModel=InputWarpedGPModel, WarpedGP=WarpedGP, WarpedGPModel=WarpedGPModel)
methods = _types.SimpleNamespace(BayesianOptimization=BayesianOptimization)
likelihoods = _types.SimpleNamespace(Gaussian=Gaussian, Bernoulli=Bernoulli)

__all__ = ["GPClassification", "GPClassModel", "Bernoulli", "kern", "mappings", "models", "methods", "likelihoods", "acquisitions", "GPRegression", "SparseGPRegression", "GPModel", "BOModel", "GPModel_MCMC", "priors", "HMC",
           "AcquisitionEI_MCMC", "AcquisitionMPI_MCMC", "AcquisitionLCB_MCMC",
           "AcquisitionTS", "AcquisitionQEI", "JointBatch", "joint_ei", "AcquisitionKG", "knowledge_gradient", "AcquisitionNEI", "noisy_ei", "posterior_paths", "PosteriorPaths", "AcquisitionMES", "max_value", "MinValueSampler", "AcquisitionEntropySearch", "entropy_search", "McmcSampler", "AffineInvariantEnsembleSampler",
           "InputWarpedGP", "InputWarpedGPModel", "input_warping", "WarpedGP", "WarpedGPModel", "warping_functions",
           "AcquisitionEI", "AcquisitionLCB", "AcquisitionMPI", "AcquisitionBase", "AcquisitionLP",
           "LocalPenalization", "estimate_L", "BayesianOptimization",
           "Design_space", "AcquisitionOptimizer", "ShardedCandidates", "merge_best", "Standardize", "cost", "CostModel", "feasibility", "FeasibilityModel",
           "multi_objective", "AcquisitionEHVI", "MultiObjectiveBayesianOptimization", "pareto_front", "hypervolume",
           "nondominated_cells"]
