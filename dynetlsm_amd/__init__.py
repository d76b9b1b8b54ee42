"""dynetlsm_amd: MI355X-native engine for DynetLSM's Metropolis-within-Gibbs
hot path (network log-likelihoods, latent-position sweep, label block update).

Importing the package does not touch the GPU; the HIP library is loaded on
first use and there is no CPU fallback (``dynetlsm_amd._lib.load`` raises when
``libdynetlsm_hip.so`` has not been built).
"""
from .engine import Chain, SamplerGrid, EngineError  # noqa
from .sparse import SparseNetwork  # noqa
from . import network_likelihoods  # noqa
from .lsm import DynamicNetworkLSM  # noqa
from .hdp_lpcm import DynamicNetworkHDPLPCM  # noqa
from .lpcm import DynamicNetworkLPCM  # noqa
from .case_control import DirectedCaseControlSampler  # noqa
from . import metrics  # noqa
from . import model_selection  # noqa
from .gof import posterior_predictive_check, GofResult  # noqa
from .ic import information_criteria, compare_information_criteria, ICResult  # noqa
from .loo import loo, compare_loo, LooResult  # noqa
from .scores import in_sample_scores, ScoreResult  # noqa
from .convergence import convergence_diagnostics, ConvergenceResult  # noqa
from .probabilities import edge_probabilities, EdgeProbabilityResult  # noqa
from . import ranking  # noqa
from .ranking import top_dyads, TopDyadsResult, top_partners, TopPartnersResult  # noqa
from . import dynamics  # noqa
from .dynamics import tie_dynamics, TieDynamicsResult  # noqa
from . import community  # noqa
from .community import community_structure, CommunityResult  # noqa
from . import forecast  # noqa  (the one-step module; calling it is forecast_paths.forecast)
from .forecast_paths import ForecastResult  # noqa

__version__ = '0.1.0'
__all__ = ['Chain', 'SamplerGrid', 'EngineError', 'SparseNetwork', 'network_likelihoods',
           'DynamicNetworkLSM', 'DynamicNetworkHDPLPCM', 'DynamicNetworkLPCM',
           'DirectedCaseControlSampler', 'posterior_predictive_check', 'GofResult',
           'information_criteria', 'compare_information_criteria', 'ICResult', 'loo', 'compare_loo', 'LooResult',
           'in_sample_scores', 'ScoreResult', 'convergence_diagnostics', 'ConvergenceResult', 'forecast',
           'ForecastResult', 'edge_probabilities', 'EdgeProbabilityResult', 'dynamics', 'tie_dynamics',
           'TieDynamicsResult', 'community', 'community_structure', 'CommunityResult', 'ranking', 'top_dyads',
           'TopDyadsResult', 'top_partners', 'TopPartnersResult']
