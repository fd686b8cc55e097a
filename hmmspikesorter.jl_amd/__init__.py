"""hmmspikesorter.jl_amd -- MI355X-native HMM spike-sorting hot path (forward/backward/update,
viterbi, reconstruct_signal of grero/HMMSpikeSorter.jl) behind libhmmsort_hip.so.

The directory name is the one the build contract fixes; it is not a valid Python identifier, so
import it through the root-level shim:  `import hmmsort_amd`.
"""
from . import _lib, dist, synth
from ._lib import (ENGINE_AUTO, ENGINE_BLOCKED, ENGINE_RING, ENGINE_STRICT, ENGINE_WAVE, HmmsortError, device_count,
                   get_option, set_option, shutdown)
from .api import (Correlograms, Footprints, HMMSpikeTemplateModel, HMMSpikingModel, ModelTrack, Posteriors, SpikeFit, StateMatrix, UnitQuality,
                  backward, extract_spiketimes, fit, fit_adaptive, fit_channels, fit_step_channels, forward, get_energy,
                  quality_from_summary, spike_fit, unit_quality, correlograms, duplicate_units, footprints, unit_locations,
                  footprint_similarity, resolve_duplicates,
                  Isolation, SnippetFeatures, cluster_isolation, isolation_scores, pca_basis, snippet_features,
                  unassigned_events, unit_gaussians, UnitStability, quantile_fractions, unit_stability,
                  Whitening, channel_mix, noise_covariance, noise_sums, whiten, whitening_matrix,
                  posterior_decode, posteriors, predict, design_fir, preprocess, reconstruct_signal, reconstruct_tracked, seed_templates, spike_confidence, train_model, train_step, unroll_mlseq, update,
                  viterbi, viterbi_step)
from .device import Plan, stats_blend, stats_sum
from .postprocess import (condense_candidates, condense_templates, find_best_overlap, match_templates,
                          prune_templates, remove_small, remove_sparse)
from .sortdata import get_lp, learn_templates, sort_data
from .synth import create_signal, create_spike_template

__all__ = ["StateMatrix", "HMMSpikeTemplateModel", "HMMSpikingModel", "forward", "backward",
           "update", "train_model", "train_step", "viterbi", "reconstruct_signal", "unroll_mlseq",
           "fit", "fit_channels", "fit_step_channels", "stats_sum", "predict", "extract_spiketimes", "Plan", "create_signal", "create_spike_template", "HmmsortError",
           "set_option", "get_option", "shutdown", "device_count", "ENGINE_AUTO", "ENGINE_STRICT",
           "ENGINE_RING", "ENGINE_BLOCKED", "ENGINE_WAVE", "get_lp", "sort_data", "find_best_overlap",
           "condense_candidates", "condense_templates", "remove_sparse", "remove_small", "prune_templates",
           "match_templates", "Posteriors", "posteriors", "posterior_decode", "spike_confidence",
           "viterbi_step", "fit_adaptive", "reconstruct_tracked", "ModelTrack", "stats_blend", "seed_templates",
           "learn_templates", "SpikeFit", "UnitQuality", "spike_fit", "unit_quality", "quality_from_summary",
           "get_energy", "Correlograms", "correlograms", "duplicate_units", "design_fir", "preprocess", "Footprints",
           "footprints", "unit_locations", "footprint_similarity", "resolve_duplicates", "Whitening", "channel_mix",
           "noise_covariance", "noise_sums", "whiten", "whitening_matrix", "Isolation", "SnippetFeatures",
           "cluster_isolation", "isolation_scores", "pca_basis", "snippet_features", "unassigned_events",
           "unit_gaussians", "UnitStability", "quantile_fractions", "unit_stability"]
