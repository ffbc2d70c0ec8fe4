"""ctypes binding of include/linearham_amd.h (liblinearham_hip.so).  No numerics live here."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

c_i32p = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
c_f64p = C.POINTER(C.c_double)


class _Segments(C.Structure):
    _fields_ = [("n_genes", C.c_int32), ("offsets", c_i32p), ("xmsa_inds", c_i32p)]


class _Junction(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_left", C.c_int32), ("n_right", C.c_int32),
                ("enter_trans", c_f64p), ("enter_lo", c_f64p), ("left_trans", c_f64p),
                ("left_lo", c_f64p), ("left_xmsa", c_i32p), ("right_gp_nli", c_f64p),
                ("right_ntt", c_f64p), ("right_nlo", c_f64p), ("right_trans", c_f64p),
                ("right_gp_li", c_f64p), ("right_xmsa", c_i32p), ("nti_xmsa", c_i32p),
                ("exit_nlo", c_f64p), ("exit_trans", c_f64p), ("exit_gp_li", c_f64p)]


class _FamilyDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("has_d", C.c_int32), ("n_seqs", C.c_int32),
                ("n_sites", C.c_int32), ("msa", c_u8p), ("n_xmsa", C.c_int32),
                ("xmsa_site", c_i32p), ("xmsa_naive_base", c_u8p),
                ("vpadding", _Segments), ("vgerm", _Segments), ("dgerm", _Segments),
                ("jgerm", _Segments), ("jpadding", _Segments),
                ("vgerm_gene_prob", c_f64p), ("vpadding_transition", c_f64p),
                ("vgerm_trans_prod", c_f64p), ("jpadding_transition", c_f64p),
                ("vd", _Junction), ("dj", _Junction)]


class _EvalOutputs(C.Structure):
    _fields_ = [("rates", c_f64p), ("xmsa_emission", c_f64p), ("forward", c_f64p),
                ("scaler_counts", c_i32p)]


EXPORTS = ["lh_last_error", "lh_device_count", "lh_family_create", "lh_family_destroy",
           "lh_forward_size", "lh_scaler_size", "lh_family_info", "lh_family_consensus_sets", "lh_schedule_tree", "lh_eval_batch",
           "lh_eval_batch_device", "lh_forward_batch", "lh_asr_batch", "lh_asr_batch_device",
           "lh_profile_enable", "lh_profile_read", "lh_asr_profile_read", "lh_family_set_extended_range", "lh_warmup", "lh_host_alloc", "lh_host_free", "lh_family_set_sampler",
           "lh_sample_words", "lh_sample_states", "lh_eval_sample_batch", "lh_set_device", "lh_family_status",
           "lh_eval_sample_batch_device", "lh_family_prune_form", "lh_family_forward_form",
           "lh_family_forward_dj_samples", "lh_family_forward_dj_waves"]
# K4 and K5 on caller-supplied emissions
CRAFTED_EXPORTS = ["lh_sample_forward_batch", "lh_posterior_forward_batch"]
EXPORTS += CRAFTED_EXPORTS
# K5 (exact posterior state marginals)
POSTERIOR_EXPORTS = ["lh_eval_posterior_batch", "lh_eval_posterior_batch_device", "lh_posterior_profile_read"]
EXPORTS += POSTERIOR_EXPORTS
# K6 (exact posterior probabilities of candidate naive sequences)
CANDIDATE_EXPORTS = ["lh_family_set_candidates", "lh_eval_candidates_batch", "lh_eval_candidates_batch_device",
                     "lh_candidates_profile_read", "lh_candidates_info", "lh_candidates_layout"]
EXPORTS += CANDIDATE_EXPORTS
# K6c (naive sequences of sampled states, the candidate store)
COLLECT_EXPORTS = ["lh_eval_draw_batch", "lh_eval_draw_batch_device", "lh_naive_sequences", "lh_draws_resolve",
                   "lh_draws_rows_read", "lh_draws_candidates_read", "lh_draws_reset", "lh_collect_profile_read"]
EXPORTS += COLLECT_EXPORTS
# K7 (the lineage of a seed sequence, the lineage store)
LINEAGE_EXPORTS = ["lh_lineage_batch", "lh_lineage_collect_device", "lh_lineage_resolve", "lh_lineage_rows_read",
                   "lh_lineage_store_read", "lh_lineage_reset", "lh_lineage_profile_read"]
EXPORTS += LINEAGE_EXPORTS
LINEAGE_PAD_HASH = 0  # LH_LINEAGE_PAD_HASH
# the chain: evaluation, naive draw, D ancestral draws and lineage hashes in one pass
LINEAGE_EVAL_EXPORTS = ["lh_eval_lineage_batch", "lh_eval_lineage_batch_device", "lh_lineage_eval_profile_read"]
EXPORTS += LINEAGE_EVAL_EXPORTS
# K8 (the most probable state path, candidate paths)
VITERBI_EXPORTS = ["lh_eval_viterbi_batch", "lh_eval_viterbi_batch_device", "lh_viterbi_forward_batch",
                   "lh_family_set_candidate_paths", "lh_viterbi_profile_read"]
EXPORTS += VITERBI_EXPORTS
# K9 (exact posterior distributions of the naive sequence's codons)
CODON_EXPORTS = ["lh_family_set_codons", "lh_codon_layout", "lh_eval_codons_batch", "lh_eval_codons_batch_device",
                 "lh_codon_profile_read"]
EXPORTS += CODON_EXPORTS
# K10 (exact posteriors of the recombination events: deletion and insertion lengths)
EVENTS_EXPORTS = ["lh_events_layout", "lh_eval_events_batch", "lh_eval_events_batch_device", "lh_events_forward_batch",
                  "lh_events_profile_read"]
EXPORTS += EVENTS_EXPORTS
# K11 (exact ancestral-state marginals along a seed's lineage)
ANCESTRAL_EXPORTS = ["lh_asr_marginals_batch", "lh_asr_marginals_batch_device", "lh_eval_ancestral_batch",
                     "lh_eval_ancestral_batch_device", "lh_ancestral_profile_read"]
EXPORTS += ANCESTRAL_EXPORTS
# K12 (exact substitution posteriors along the edges of a seed's lineage)
EDGES_EXPORTS = ["lh_asr_edges_batch", "lh_asr_edges_batch_device", "lh_eval_edges_batch", "lh_eval_edges_batch_device",
                 "lh_edges_profile_read"]
EXPORTS += EDGES_EXPORTS
# K13 (exact posterior probabilities of candidate ancestral sequences)
ANCESTRAL_PROBS_EXPORTS = ["lh_family_set_ancestral_candidates", "lh_ancestral_candidates_info",
                           "lh_eval_ancestral_candidates_batch", "lh_eval_ancestral_candidates_batch_device",
                           "lh_ancestral_candidates_profile_read", "lh_eval_ancestral_candidates_at_batch",
                           "lh_eval_ancestral_candidates_at_batch_device"]
EXPORTS += ANCESTRAL_PROBS_EXPORTS
NODE_PARENT, NODE_MRCA = 0, 1  # lh_eval_ancestral_candidates_batch's `node`
# K14 (exact codon marginals of a node of a seed's lineage)
NODE_CODONS_EXPORTS = ["lh_eval_node_codons_batch", "lh_eval_node_codons_batch_device", "lh_asr_node_codons_batch",
                       "lh_asr_node_codons_batch_device", "lh_node_codon_classes", "lh_node_codons_profile_read",
                       "lh_eval_node_codons_at_batch", "lh_eval_node_codons_at_batch_device", "lh_asr_node_codons_at_batch",
                       "lh_asr_node_codons_at_batch_device"]
EXPORTS += NODE_CODONS_EXPORTS
# K15 (exact amino-acid replacement posteriors along the edges of a seed's lineage)
CODON_EDGES_EXPORTS = ["lh_eval_codon_edges_batch", "lh_eval_codon_edges_batch_device", "lh_asr_codon_edges_batch",
                       "lh_asr_codon_edges_batch_device", "lh_codon_edge_symbols", "lh_codon_edges_profile_read"]
EXPORTS += CODON_EDGES_EXPORTS
AA_SYMBOLS = "ACDEFGHIKLMNPQRSTVWY*"  # the 21 symbols of aa_counts, in lh_codon_edge_symbols' numbering


class _CodonOutputs(C.Structure):
    _fields_ = [("log_offset", c_f64p), ("loglik", c_f64p), ("windows", c_f64p), ("genes", c_f64p),
                ("weighted_windows", c_f64p), ("weighted_genes", c_f64p), ("weight_stats", c_f64p)]


class _CodonOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in ("log_offset", "loglik", "windows", "genes", "weighted_windows",
                                          "weighted_genes", "weight_stats")]


class _EventsOutputs(C.Structure):
    _fields_ = [("log_offset", c_f64p), ("loglik", c_f64p), ("events", c_f64p), ("genes", c_f64p),
                ("weighted_events", c_f64p), ("weighted_genes", c_f64p), ("weight_stats", c_f64p)]


class _EventsOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in ("log_offset", "loglik", "events", "genes", "weighted_events", "weighted_genes",
                                          "weight_stats")]


class _ViterbiOutputs(C.Structure):
    _fields_ = [("log_offset", c_f64p), ("loglik", c_f64p), ("states", c_i32p), ("log_path", c_f64p),
                ("weight_stats", c_f64p)]


class _ViterbiOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in ("log_offset", "loglik", "states", "log_path", "weight_stats")]


_ANCESTRAL_MEMBERS = ("log_offset", "loglik", "site_base", "marg", "rate_post", "weighted_sum", "weighted_rate",
                      "weight_stats")


class _AncestralOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _ANCESTRAL_MEMBERS]


class _AncestralOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _ANCESTRAL_MEMBERS]


_EDGES_MEMBERS = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
_EVAL_EDGES_MEMBERS = ("log_offset", "loglik", "site_base", "edge", "naive_edge", "chain_counts", "seed_edge", "edge_load",
                       "rate_post", "weighted_counts", "weighted_seed_edge", "weighted_naive_edge", "weight_stats")


class _EdgesOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _EDGES_MEMBERS]


class _EdgesOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _EDGES_MEMBERS]


class _EvalEdgesOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _EVAL_EDGES_MEMBERS]


class _EvalEdgesOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _EVAL_EDGES_MEMBERS]


_ANCESTRAL_PROBS_MEMBERS = ("log_offset", "loglik", "cond", "log_cand", "weighted_sum", "weight_stats")


class _AncestralProbsOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _ANCESTRAL_PROBS_MEMBERS]


class _AncestralProbsOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _ANCESTRAL_PROBS_MEMBERS]


_NODE_CODONS_MEMBERS = ("log_offset", "loglik", "codons", "change", "weighted_codons", "weighted_change", "weight_stats")


class _NodeCodonsOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _NODE_CODONS_MEMBERS]


class _NodeCodonsOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _NODE_CODONS_MEMBERS]


_CODON_EDGES_MEMBERS = ("log_offset", "loglik", "codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load",
                        "weighted_codon_counts", "weighted_aa_counts", "weighted_seed_change", "weight_stats")
_CODON_EDGES_TABLES = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")


class _CodonEdgesOutputs(C.Structure):
    _fields_ = [(k, c_f64p) for k in _CODON_EDGES_MEMBERS]


class _CodonEdgesOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in _CODON_EDGES_MEMBERS]


def _codon_edges_shapes(n, nc, P):
    return dict(codon_counts=(n, nc, 4), aa_counts=(n, nc, 21, 21), seed_change=(n, nc, 3), edge_change=(n, P + 1, nc, 3),
                edge_load=(n, P + 1, 2))


class _SamplerJunction(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_left", C.c_int32), ("n_right", C.c_int32), ("n_states", C.c_int32),
                ("left_rows", c_i32p), ("left_dense", c_i32p), ("left_lo", c_f64p), ("left_trans", c_f64p),
                ("enter_lo", c_f64p), ("right_dense", c_i32p), ("right_first", c_i32p), ("gene_prob", c_f64p),
                ("nti_landing_in", c_f64p), ("nti_transition", c_f64p), ("nti_landing_out", c_f64p),
                ("landing_in", c_f64p), ("right_trans", c_f64p), ("exit_nlo", c_f64p), ("exit_trans", c_f64p),
                ("exit_li", c_f64p), ("prod", c_f64p)]


class _SamplerDesc(C.Structure):
    _fields_ = [("vd", _SamplerJunction), ("dj", _SamplerJunction)]


class _PosteriorOutputs(C.Structure):
    _fields_ = [("log_offset", c_f64p), ("loglik", c_f64p), ("posterior", c_f64p), ("weighted_sum", c_f64p),
                ("weight_stats", c_f64p)]


class _CandidateOutputs(C.Structure):
    _fields_ = [("log_offset", c_f64p), ("loglik", c_f64p), ("log_cand", c_f64p), ("weighted_sum", c_f64p),
                ("weight_stats", c_f64p)]


class _LineageEvalOutputs(C.Structure):
    _fields_ = [("loglik", c_f64p), ("rates", c_f64p), ("states", c_i32p), ("naive", c_u8p),
                ("naive_hash", C.POINTER(C.c_uint64)), ("nt_hash", C.POINTER(C.c_uint64)),
                ("aa_hash", C.POINTER(C.c_uint64))]


class _LineageEvalOutputsDevice(C.Structure):  # the same members as device addresses
    _fields_ = [(k, C.c_void_p) for k in ("loglik", "rates", "states", "naive", "naive_hash", "nt_hash", "aa_hash")]


def library_path():
    # LH_LIB_DIR: timing experiments load a variant build from its own directory (tools/build_variant.sh) instead of
    # overwriting the product library in place
    return os.path.join(os.environ.get("LH_LIB_DIR") or os.path.join(_HERE, "lib"), "liblinearham_hip.so")


# what every lh_*_batch (host pointers) / lh_*_batch_device (device addresses) entry point begins with: the handle, n,
# n_tips, max_depth, ops, brlen, er, pi, alpha or rates, num_rates
_HOST_TREE = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_f64p, c_f64p, c_f64p, c_f64p, C.c_int32]
_DEV_TREE = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32]
_PROFILE_READ = [C.c_void_p, c_f64p, C.POINTER(C.c_int64)]


class HipLibrary:
    def __init__(self, path=None):
        path = path or library_path()
        if not os.path.exists(path):
            raise RuntimeError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (there is no CPU fallback)" % path)
        self.lib = lib = C.CDLL(path)
        c_u32p, c_u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        lib.lh_last_error.restype = C.c_char_p
        lib.lh_device_count.restype = C.c_int
        lib.lh_family_create.argtypes = [C.POINTER(_FamilyDesc), C.POINTER(C.c_void_p)]
        lib.lh_family_destroy.argtypes = [C.c_void_p]
        lib.lh_family_destroy.restype = None
        lib.lh_forward_size.argtypes = [C.c_void_p]
        lib.lh_forward_size.restype = C.c_int64
        lib.lh_scaler_size.argtypes = [C.c_void_p]
        lib.lh_scaler_size.restype = C.c_int64
        lib.lh_family_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.lh_family_info.restype = C.c_int
        lib.lh_family_consensus_sets.argtypes = [C.c_void_p]
        lib.lh_family_consensus_sets.restype = C.c_int
        lib.lh_family_prune_form.argtypes = [C.c_void_p]
        lib.lh_family_prune_form.restype = C.c_char_p
        lib.lh_family_forward_form.argtypes = [C.c_void_p]
        lib.lh_family_forward_form.restype = C.c_char_p
        if hasattr(lib, "lh_family_forward_dj_samples"):  # (absent from earlier builds loaded through LH_LIB_DIR)
            lib.lh_family_forward_dj_samples.argtypes = [C.c_void_p]
            lib.lh_family_forward_dj_samples.restype = C.c_int
        if hasattr(lib, "lh_family_forward_dj_waves"):  # (likewise)
            lib.lh_family_forward_dj_waves.argtypes = [C.c_void_p]
            lib.lh_family_forward_dj_waves.restype = C.c_int
        lib.lh_schedule_tree.argtypes = [C.c_int32, c_i32p, C.c_int32, c_i32p, c_i32p]
        lib.lh_eval_batch.argtypes = _HOST_TREE + [c_f64p, C.POINTER(_EvalOutputs)]
        lib.lh_eval_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.POINTER(_EvalOutputs), C.c_void_p]
        lib.lh_forward_batch.argtypes = [C.c_void_p, C.c_int32, c_f64p, c_f64p, C.POINTER(_EvalOutputs)]
        lib.lh_asr_batch.argtypes = _HOST_TREE + [c_u8p, C.c_uint64, C.c_uint64, c_u8p, c_u8p]
        lib.lh_asr_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3
        lib.lh_asr_profile_read.argtypes = _PROFILE_READ
        lib.lh_profile_enable.argtypes = [C.c_void_p, C.c_int]
        lib.lh_family_set_extended_range.argtypes = [C.c_void_p, C.c_int]
        lib.lh_profile_read.argtypes = [C.c_void_p, c_f64p, c_f64p, c_f64p, C.POINTER(C.c_int64)]
        if hasattr(lib, "lh_eval_sample_batch_device"):
            lib.lh_eval_sample_batch_device.argtypes = _DEV_TREE + [C.c_void_p] * 5
            lib.lh_sample_words.argtypes = [C.c_void_p]
            lib.lh_sample_states.argtypes = [C.c_void_p]
        if hasattr(lib, "lh_sample_forward_batch"):
            lib.lh_sample_forward_batch.argtypes = [C.c_void_p, C.c_int32, c_f64p, c_u32p, c_f64p, c_i32p,
                                                    C.POINTER(_EvalOutputs)]
            lib.lh_posterior_forward_batch.argtypes = [C.c_void_p, C.c_int32, c_f64p, c_f64p, c_f64p]
        if hasattr(lib, "lh_eval_posterior_batch"):
            lib.lh_eval_posterior_batch.argtypes = _HOST_TREE + [C.POINTER(_PosteriorOutputs)]
            lib.lh_eval_posterior_batch_device.argtypes = _DEV_TREE + [C.POINTER(_PosteriorOutputs), C.c_void_p]
            lib.lh_posterior_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_family_set_candidates"):
            lib.lh_family_set_candidates.argtypes = [C.c_void_p, C.c_int32, c_u8p, c_f64p]
            lib.lh_eval_candidates_batch.argtypes = _HOST_TREE + [C.POINTER(_CandidateOutputs)]
            lib.lh_eval_candidates_batch_device.argtypes = _DEV_TREE + [C.POINTER(_CandidateOutputs), C.c_void_p]
            lib.lh_candidates_profile_read.argtypes = _PROFILE_READ
            lib.lh_candidates_info.argtypes = [C.c_void_p, c_i32p, c_i32p]
            lib.lh_candidates_layout.argtypes = [C.c_void_p, c_i32p, c_i32p, c_i32p]
        if hasattr(lib, "lh_naive_sequences"):
            lib.lh_eval_draw_batch.argtypes = _HOST_TREE + [c_u32p, c_f64p, c_u64p, c_i32p]
            lib.lh_eval_draw_batch_device.argtypes = _DEV_TREE + [C.c_void_p] * 5
            lib.lh_naive_sequences.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_u8p, c_u64p]
            lib.lh_draws_resolve.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_i32p, c_i32p]
            lib.lh_draws_rows_read.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_u8p]
            lib.lh_draws_candidates_read.argtypes = [C.c_void_p, c_i32p, c_u8p]
            lib.lh_draws_reset.argtypes = [C.c_void_p]
            lib.lh_collect_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_lineage_batch"):
            lib.lh_lineage_batch.argtypes = _HOST_TREE + [c_u8p, C.c_uint64, C.c_uint64, c_i32p, C.c_int32, c_u64p, c_u64p]
            lib.lh_lineage_collect_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.lh_lineage_resolve.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_i32p, c_i32p]
            lib.lh_lineage_rows_read.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_u8p]
            lib.lh_lineage_store_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_i32p, c_u8p]
            lib.lh_lineage_reset.argtypes = [C.c_void_p]
            lib.lh_lineage_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_eval_lineage_batch"):
            lib.lh_eval_lineage_batch.argtypes = _HOST_TREE + [c_u32p, C.c_uint64, C.c_uint64, C.c_int32, c_i32p, C.c_int32,
                                                               C.POINTER(_LineageEvalOutputs)]
            lib.lh_eval_lineage_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(_LineageEvalOutputsDevice),
                C.c_void_p]
            lib.lh_lineage_eval_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_eval_viterbi_batch"):
            lib.lh_family_set_sampler.argtypes = [C.c_void_p, C.POINTER(_SamplerDesc)]
            lib.lh_eval_viterbi_batch.argtypes = _HOST_TREE + [C.POINTER(_ViterbiOutputs)]
            lib.lh_eval_viterbi_batch_device.argtypes = _DEV_TREE + [C.POINTER(_ViterbiOutputsDevice), C.c_void_p]
            lib.lh_viterbi_forward_batch.argtypes = [C.c_void_p, C.c_int32, c_f64p, c_f64p, c_i32p]
            lib.lh_family_set_candidate_paths.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_f64p]
            lib.lh_viterbi_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_family_set_codons"):
            lib.lh_family_set_codons.argtypes = [C.c_void_p, C.c_int32]
            lib.lh_codon_layout.argtypes = [C.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p]
            lib.lh_eval_codons_batch.argtypes = _HOST_TREE + [C.POINTER(_CodonOutputs)]
            lib.lh_eval_codons_batch_device.argtypes = _DEV_TREE + [C.POINTER(_CodonOutputsDevice), C.c_void_p]
            lib.lh_codon_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_events_layout"):
            c_i64p = C.POINTER(C.c_int64)
            lib.lh_events_layout.argtypes = [C.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p, c_i64p, c_i64p, c_i64p, c_i64p,
                                             c_i32p]
            lib.lh_eval_events_batch.argtypes = _HOST_TREE + [C.POINTER(_EventsOutputs)]
            lib.lh_eval_events_batch_device.argtypes = _DEV_TREE + [C.POINTER(_EventsOutputsDevice), C.c_void_p]
            lib.lh_events_forward_batch.argtypes = [C.c_void_p, C.c_int32, c_f64p, c_f64p, c_f64p]
            lib.lh_events_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_asr_marginals_batch"):
            lib.lh_asr_marginals_batch.argtypes = _HOST_TREE + [c_f64p, c_i32p, C.c_int32, c_f64p, c_f64p]
            lib.lh_asr_marginals_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3
            lib.lh_eval_ancestral_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, C.POINTER(_AncestralOutputs)]
            lib.lh_eval_ancestral_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_int32,
                                                                       C.POINTER(_AncestralOutputsDevice), C.c_void_p]
            lib.lh_ancestral_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_asr_edges_batch"):
            lib.lh_asr_edges_batch.argtypes = _HOST_TREE + [c_f64p, c_i32p, C.c_int32, C.c_int32, C.POINTER(_EdgesOutputs)]
            lib.lh_asr_edges_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                                  C.POINTER(_EdgesOutputsDevice), C.c_void_p]
            lib.lh_eval_edges_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, C.c_int32, C.POINTER(_EvalEdgesOutputs)]
            lib.lh_eval_edges_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_int32, C.c_int32,
                                                                   C.POINTER(_EvalEdgesOutputsDevice), C.c_void_p]
            lib.lh_edges_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_family_set_ancestral_candidates"):
            lib.lh_family_set_ancestral_candidates.argtypes = [C.c_void_p, C.c_int32, c_u8p]
            lib.lh_ancestral_candidates_info.argtypes = [C.c_void_p, c_i32p, c_i32p]
            lib.lh_eval_ancestral_candidates_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, C.c_int32,
                                                                            C.POINTER(_AncestralProbsOutputs)]
            lib.lh_eval_ancestral_candidates_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_AncestralProbsOutputsDevice), C.c_void_p]
            lib.lh_ancestral_candidates_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_eval_ancestral_candidates_at_batch"):  # (the slot array in the place of `node`)
            lib.lh_eval_ancestral_candidates_at_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, c_i32p,
                                                                               C.POINTER(_AncestralProbsOutputs)]
            lib.lh_eval_ancestral_candidates_at_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(_AncestralProbsOutputsDevice), C.c_void_p]
            lib.lh_eval_node_codons_at_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, c_i32p, C.POINTER(_NodeCodonsOutputs)]
            lib.lh_eval_node_codons_at_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(_NodeCodonsOutputsDevice), C.c_void_p]
            lib.lh_asr_node_codons_at_batch.argtypes = _HOST_TREE + [c_f64p, c_i32p, C.c_int32, c_i32p, c_f64p, c_f64p]
            lib.lh_asr_node_codons_at_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + \
                [C.c_void_p] * 3
        if hasattr(lib, "lh_eval_node_codons_batch"):
            lib.lh_eval_node_codons_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, C.c_int32,
                                                                   C.POINTER(_NodeCodonsOutputs)]
            lib.lh_eval_node_codons_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_NodeCodonsOutputsDevice), C.c_void_p]
            lib.lh_asr_node_codons_batch.argtypes = _HOST_TREE + [c_f64p, c_i32p, C.c_int32, C.c_int32, c_f64p, c_f64p]
            lib.lh_asr_node_codons_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + \
                [C.c_void_p] * 3
            lib.lh_node_codon_classes.argtypes = [c_u8p]
            lib.lh_node_codons_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_eval_codon_edges_batch"):
            lib.lh_eval_codon_edges_batch.argtypes = _HOST_TREE + [c_i32p, C.c_int32, C.c_int32,
                                                                   C.POINTER(_CodonEdgesOutputs)]
            lib.lh_eval_codon_edges_batch_device.argtypes = _DEV_TREE + [
                C.c_void_p, C.c_int32, C.c_int32, C.POINTER(_CodonEdgesOutputsDevice), C.c_void_p]
            lib.lh_asr_codon_edges_batch.argtypes = _HOST_TREE + [c_f64p, c_i32p, C.c_int32, C.c_int32] + [c_f64p] * 6
            lib.lh_asr_codon_edges_batch_device.argtypes = _DEV_TREE + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + \
                [C.c_void_p] * 7
            lib.lh_codon_edge_symbols.argtypes = [c_u8p]
            lib.lh_codon_edges_profile_read.argtypes = _PROFILE_READ
        if hasattr(lib, "lh_set_device"):      # (absent from round-2 builds loaded through LH_LIB_DIR for comparisons)
            lib.lh_set_device.argtypes = [C.c_int32]
            lib.lh_family_status.argtypes = [C.c_void_p]

    def error(self):
        return self.lib.lh_last_error().decode()

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("linearham_hip: " + self.error())

    def device_count(self):
        return self.lib.lh_device_count()

    def _profile_read(self, name, family, n_ms=1):
        """lh_<name>_profile_read: (the n_ms kernel times in ms ..., launch groups) since the last read."""
        ms, k = (C.c_double * n_ms)(), C.c_int64()
        self.check(getattr(self.lib, name)(_handle(family), ms, C.byref(k)))
        return tuple(ms) + (k.value,)

    def eval_posterior_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, log_offset=None,
                             want=("loglik", "posterior", "weighted_sum", "weight_stats")):
        """K0-K2 + K5 on a family handle (a raw lh_family* or a Family) that has sampler tables.  Returns a dict with the
        members of `want`: loglik [n], posterior [n, forward_size], weighted_sum [forward_size], weight_stats [3]
        (max lw, sum w, sum w^2 with lw = loglik - log_offset)."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        fs = self.lib.lh_forward_size(h)
        res, outs = _outputs(_PosteriorOutputs, want, log_offset, loglik=(n,), posterior=(n, fs), weighted_sum=(fs,),
                             weight_stats=(3,))
        self.check(self.lib.lh_eval_posterior_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, C.byref(outs)))
        return res

    def eval_ancestral_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, log_offset=None,
                             want=("loglik", "site_base", "marg", "rate_post", "weighted_sum", "weighted_rate",
                                   "weight_stats")):
        """K0-K2 + K5 + K11 on a family handle that has sampler tables; path [n][P] (seed_path rows, -1 padding).  Returns a
        dict with the members of `want`: loglik [n], site_base [n, L, 5], marg [n, P, L, 4], rate_post [n, L, R],
        weighted_sum [2, L, 4] (the seed's parent, the MRCA), weighted_rate [L, R], weight_stats [3]."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        path = _i32(path)
        assert path.ndim == 2 and path.shape[0] == n
        P, R = path.shape[1], num_rates
        _, L = self.candidates_info(h)
        res, outs = _outputs(_AncestralOutputs, want, log_offset, loglik=(n,), site_base=(n, L, 5), marg=(n, P, L, 4),
                             rate_post=(n, L, R), weighted_sum=(2, L, 4), weighted_rate=(L, R), weight_stats=(3,))
        self.check(self.lib.lh_eval_ancestral_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates,
                                                    _ptr(path, c_i32p), P, C.byref(outs)))
        return res

    def eval_ancestral_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                                    num_rates, path_ptr, path_len, outs, stream=0):
        """lh_eval_ancestral_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _AncestralOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_ancestral_batch_device(_handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr,
                                                           pi_ptr, alpha_ptr, num_rates, path_ptr, path_len, C.byref(o),
                                                           stream))

    def ancestral_profile_read(self, family):
        """(k11a_ms, k11b_ms, reduce_ms, launch groups) of K11 since the last read."""
        return self._profile_read("lh_ancestral_profile_read", family, 3)

    def ancestral_candidates_info(self, family):
        """(ancestral candidates registered on the handle, sites each has): lh_ancestral_candidates_info."""
        k, L = C.c_int32(), C.c_int32()
        self.check(self.lib.lh_ancestral_candidates_info(_handle(family), C.byref(k), C.byref(L)))
        return k.value, L.value

    def set_ancestral_candidates(self, family, seqs):
        """K13: registers candidate ancestral sequences seqs [K][L] on a family handle: A,C,G,T = 0..3, 4 = the site is
        left open.  The naive candidates of set_candidates stay registered."""
        h = _handle(family)
        seqs = np.asarray(seqs)
        if seqs.ndim != 2 or seqs.dtype.kind not in "iu":
            raise ValueError("lh_family_set_ancestral_candidates: candidates must be an integer [K][L] array")
        L = self.ancestral_candidates_info(h)[1]
        if seqs.shape[1] != L:
            raise ValueError("lh_family_set_ancestral_candidates: candidates have %d sites, the family's alignment %d"
                             % (seqs.shape[1], L))
        if seqs.size and (seqs.min() < 0 or seqs.max() > 255):
            raise ValueError("lh_family_set_ancestral_candidates: bases must be bytes")
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        self.check(self.lib.lh_family_set_ancestral_candidates(h, seqs.shape[0], seqs.ctypes.data_as(c_u8p)))

    def eval_ancestral_candidates_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, node,
                                        log_offset=None, want=("loglik", "cond", "log_cand", "weighted_sum",
                                                               "weight_stats")):
        """K0-K2 + K5 + K13 on a family handle that has sampler tables and ancestral candidates; path [n][P] (seed_path
        rows, -1 padding), node NODE_PARENT or NODE_MRCA.  Returns a dict with the members of `want`: loglik [n], cond
        [n, L, 5, 4] (P(x_node = c | column, naive base b)), log_cand [n, K], weighted_sum [K], weight_stats [3]."""
        return self._eval_ancestral_candidates("lh_eval_ancestral_candidates_batch", family, n_tips, max_depth, ops, brlen,
                                               er, pi, alpha, num_rates, path, node, log_offset, want)

    def eval_ancestral_candidates_at_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, slot,
                                           log_offset=None, want=("loglik", "cond", "log_cand", "weighted_sum",
                                                                  "weight_stats")):
        """eval_ancestral_candidates_batch at a node per row: slot [n], for every sample the entry of its own path the
        tables are formed at (clade_slot gives it for the common ancestor of the seed and other tips)."""
        return self._eval_ancestral_candidates("lh_eval_ancestral_candidates_at_batch", family, n_tips, max_depth, ops,
                                               brlen, er, pi, alpha, num_rates, path, _slots(slot), log_offset, want)

    def _eval_ancestral_candidates(self, entry, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, node,
                                   log_offset, want):
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        path = _i32(path)
        assert path.ndim == 2 and path.shape[0] == n
        K, L = self.ancestral_candidates_info(h)
        res, outs = _outputs(_AncestralProbsOutputs, want, log_offset, loglik=(n,), cond=(n, L, 5, 4), log_cand=(n, K),
                             weighted_sum=(K,), weight_stats=(3,))
        self.check(getattr(self.lib, entry)(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, _ptr(path, c_i32p),
                                            path.shape[1], _node_arg(node, n), C.byref(outs)))
        return res

    def eval_ancestral_candidates_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr,
                                               alpha_ptr, num_rates, path_ptr, path_len, node, outs, stream=0):
        """lh_eval_ancestral_candidates_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _AncestralProbsOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_ancestral_candidates_batch_device(
            _handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, path_ptr,
            path_len, node, C.byref(o), stream))

    def eval_ancestral_candidates_at_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr,
                                                  alpha_ptr, num_rates, path_ptr, path_len, slot_ptr, outs, stream=0):
        """lh_eval_ancestral_candidates_at_batch_device on device addresses (slot_ptr: int32 [n])."""
        o = _AncestralProbsOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_ancestral_candidates_at_batch_device(
            _handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, path_ptr,
            path_len, slot_ptr, C.byref(o), stream))

    def ancestral_candidates_profile_read(self, family):
        """(tables ms, pair emissions and sweeps ms, reduction ms, launch groups) of K13 since the last read."""
        return self._profile_read("lh_ancestral_candidates_profile_read", family, 3)

    def eval_node_codons_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, node,
                               log_offset=None, want=("loglik", "codons", "change", "weighted_codons", "weighted_change",
                                                      "weight_stats")):
        """K0-K2 + K9 + K13's tables + K14 on a family handle after set_codons; path [n][P] (seed_path rows, -1 padding),
        node NODE_PARENT or NODE_MRCA.  Returns a dict with the members of `want`: loglik [n], codons [n, C, 64] (the node's
        triple 16 x1 + 4 x2 + x3 over A,C,G,T), change [n, C, 4] (identical, synonymous, replacement, naive triple with an
        N), weighted_codons [C, 64], weighted_change [C, 4], weight_stats [3]."""
        return self._eval_node_codons("lh_eval_node_codons_batch", family, n_tips, max_depth, ops, brlen, er, pi, alpha,
                                      num_rates, path, node, log_offset, want)

    def eval_node_codons_at_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, slot,
                                  log_offset=None, want=("loglik", "codons", "change", "weighted_codons", "weighted_change",
                                                         "weight_stats")):
        """eval_node_codons_batch at a node per row: slot [n] as eval_ancestral_candidates_at_batch takes it."""
        return self._eval_node_codons("lh_eval_node_codons_at_batch", family, n_tips, max_depth, ops, brlen, er, pi, alpha,
                                      num_rates, path, _slots(slot), log_offset, want)

    def _eval_node_codons(self, entry, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, node,
                          log_offset, want):
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        path = _i32(path)
        assert path.ndim == 2 and path.shape[0] == n
        nc = C.c_int32()
        self.check(self.lib.lh_codon_layout(h, C.byref(nc), None, None, None))
        nc = nc.value
        res, outs = _outputs(_NodeCodonsOutputs, want, log_offset, loglik=(n,), codons=(n, nc, 64), change=(n, nc, 4),
                             weighted_codons=(nc, 64), weighted_change=(nc, 4), weight_stats=(3,))
        self.check(getattr(self.lib, entry)(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, _ptr(path, c_i32p),
                                            path.shape[1], _node_arg(node, n), C.byref(outs)))
        return res

    def eval_node_codons_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                                      num_rates, path_ptr, path_len, node, outs, stream=0):
        """lh_eval_node_codons_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _NodeCodonsOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_node_codons_batch_device(
            _handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, path_ptr,
            path_len, node, C.byref(o), stream))

    def eval_node_codons_at_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                                         num_rates, path_ptr, path_len, slot_ptr, outs, stream=0):
        """lh_eval_node_codons_at_batch_device on device addresses (slot_ptr: int32 [n])."""
        o = _NodeCodonsOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_node_codons_at_batch_device(
            _handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, path_ptr,
            path_len, slot_ptr, C.byref(o), stream))

    def node_codons_profile_read(self, family):
        """(K9 + tables ms, contraction ms, reduction ms, launch groups) of K14 since the last read."""
        return self._profile_read("lh_node_codons_profile_read", family, 3)

    def node_codon_classes(self):
        """[125, 64] uint8: the class (0 identical, 1 synonymous, 2 replacement, 3 naive triple with an N) of every (naive
        triple, node triple) pair as the device's compile-time table has it."""
        out = np.zeros((125, 64), dtype=np.uint8)
        self.check(self.lib.lh_node_codon_classes(out.ctypes.data_as(c_u8p)))
        return out

    def eval_codon_edges_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, seed_tip,
                               log_offset=None, want=("loglik",) + _CODON_EDGES_TABLES):
        """K0-K2 + K9 + K15 on a family handle after set_codons; path [n][P] (seed_path rows, -1 padding) of tip seed_tip.
        Returns a dict with the members of `want`: loglik [n], codon_counts [n, C, 4] (expected lineage edges on which the
        codon stays, changes silently, changes by replacement; naive triple with an N), aa_counts [n, C, 21, 21] (from the
        upper end's symbol to the lower end's, AA_SYMBOLS), seed_change [n, C, 3], edge_change [n, P + 1, C, 3] (entry P the
        naive edge), edge_load [n, P + 1, 2], weighted_codon_counts [C, 4], weighted_aa_counts [C, 21, 21],
        weighted_seed_change [C, 3], weight_stats [3]."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        path = _i32(path)
        assert path.ndim == 2 and path.shape[0] == n
        nc = C.c_int32()
        self.check(self.lib.lh_codon_layout(h, C.byref(nc), None, None, None))
        nc = nc.value
        res, outs = _outputs(_CodonEdgesOutputs, want, log_offset, loglik=(n,), weighted_codon_counts=(nc, 4),
                             weighted_aa_counts=(nc, 21, 21), weighted_seed_change=(nc, 3), weight_stats=(3,),
                             **_codon_edges_shapes(n, nc, path.shape[1]))
        self.check(self.lib.lh_eval_codon_edges_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates,
                                                      _ptr(path, c_i32p), path.shape[1], seed_tip, C.byref(outs)))
        return res

    def eval_codon_edges_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                                      num_rates, path_ptr, path_len, seed_tip, outs, stream=0):
        """lh_eval_codon_edges_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _CodonEdgesOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_codon_edges_batch_device(
            _handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, path_ptr,
            path_len, seed_tip, C.byref(o), stream))

    def codon_edges_profile_read(self, family):
        """(K9 + tables ms, contraction ms, reduction ms, launch groups) of K15 since the last read."""
        return self._profile_read("lh_codon_edges_profile_read", family, 3)

    def codon_edge_symbols(self):
        """[64] uint8: the symbol (index into AA_SYMBOLS) of every triple 16 x1 + 4 x2 + x3 as the device's compile-time
        map has it."""
        out = np.zeros(64, dtype=np.uint8)
        self.check(self.lib.lh_codon_edge_symbols(out.ctypes.data_as(c_u8p)))
        return out

    def eval_edges_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, path, seed_tip,
                         log_offset=None, want=("loglik", "chain_counts", "seed_edge", "naive_edge", "edge_load")):
        """K0-K2 + K5 + K12 on a family handle that has sampler tables; path [n][P] (seed_path rows, -1 padding) of tip
        `seed_tip`.  Returns a dict with the members of `want`: loglik [n], site_base [n, L, 5], edge [n, P, L, 4, 4],
        naive_edge [n, L, 5, 4], chain_counts [n, L, 4, 4], seed_edge [n, L, 4, 4], edge_load [n, P+1], rate_post [n, L, R],
        weighted_counts [L, 4, 4], weighted_seed_edge [L, 4, 4], weighted_naive_edge [L, 5, 4], weight_stats [3].  Tables are
        indexed [ancestor state][descendant state]; without "edge" the lean kernel runs."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        path = _i32(path)
        assert path.ndim == 2 and path.shape[0] == n
        P, R = path.shape[1], num_rates
        _, L = self.candidates_info(h)
        res, outs = _outputs(_EvalEdgesOutputs, want, log_offset, loglik=(n,), site_base=(n, L, 5), edge=(n, P, L, 4, 4),
                             naive_edge=(n, L, 5, 4), chain_counts=(n, L, 4, 4), seed_edge=(n, L, 4, 4), edge_load=(n, P + 1),
                             rate_post=(n, L, R), weighted_counts=(L, 4, 4), weighted_seed_edge=(L, 4, 4),
                             weighted_naive_edge=(L, 5, 4), weight_stats=(3,))
        self.check(self.lib.lh_eval_edges_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, _ptr(path, c_i32p), P,
                                                int(seed_tip), C.byref(outs)))
        return res

    def eval_edges_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates,
                                path_ptr, path_len, seed_tip, outs, stream=0):
        """lh_eval_edges_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _EvalEdgesOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_edges_batch_device(_handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr,
                                                       alpha_ptr, num_rates, path_ptr, path_len, int(seed_tip), C.byref(o),
                                                       stream))

    def edges_profile_read(self, family):
        """(k11a_ms, k12b_ms, reduce_ms, launch groups) of K12 since the last read."""
        return self._profile_read("lh_edges_profile_read", family, 3)

    def posterior_profile_read(self, family):
        return self._profile_read("lh_posterior_profile_read", family)

    def set_codons(self, family, frame=0):
        """Fixes the reading frame of K9 on a family handle that has sampler tables and returns its layout:
        dict(frame, n_codons, window_codon [n_window], n_genes)."""
        h = _handle(family)
        self.check(self.lib.lh_family_set_codons(h, frame))
        return self.codon_layout(h, frame)

    def codon_layout(self, family, frame):
        """The layout of the handle's window tables; `frame` is the one set_codons fixed (the C ABI does not report it)."""
        h = _handle(family)
        nc, nw, ng = C.c_int32(), C.c_int32(), C.c_int32()
        self.check(self.lib.lh_codon_layout(h, C.byref(nc), C.byref(nw), None, C.byref(ng)))
        wc = np.zeros(max(nw.value, 1), dtype=np.int32)
        self.check(self.lib.lh_codon_layout(h, None, None, wc.ctypes.data_as(c_i32p), None))
        return dict(frame=frame, n_codons=nc.value, window_codon=wc[:nw.value].tolist(), n_genes=ng.value)

    def eval_codons_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, log_offset=None,
                          want=("loglik", "windows", "genes", "weighted_windows", "weighted_genes", "weight_stats")):
        """K0-K2 + K9 on a family handle after set_codons.  Returns a dict with the members of `want`: loglik [n],
        windows [n, n_window, 125], genes [n, n_genes], weighted_windows [n_window, 125], weighted_genes [n_genes],
        weight_stats [3] (max lw, sum w, sum w^2 with lw = loglik - log_offset)."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        nw, ng = C.c_int32(), C.c_int32()
        self.check(self.lib.lh_codon_layout(h, None, C.byref(nw), None, C.byref(ng)))
        res, outs = _outputs(_CodonOutputs, want, log_offset, loglik=(n,), windows=(n, nw.value, 125), genes=(n, ng.value),
                             weighted_windows=(nw.value, 125), weighted_genes=(ng.value,), weight_stats=(3,))
        self.check(self.lib.lh_eval_codons_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, C.byref(outs)))
        return res

    def codon_profile_read(self, family):
        return self._profile_read("lh_codon_profile_read", family)

    def events_layout(self, family):
        """The layout of K10's flat row on a family handle that has sampler tables: dict(size, n_genes, junctions =
        [dict(rows, n_left, n_right, exit, enter, span)]), the last three the offsets of exit [n_left][rows + 1],
        enter [n_right][rows + 1] and span [rows + 1][rows + 1] in the row."""
        h = _handle(family)
        nj, ng, size = C.c_int32(), C.c_int32(), C.c_int64()
        i32 = [(C.c_int32 * 2)() for _ in range(3)]
        i64 = [(C.c_int64 * 2)() for _ in range(3)]
        self.check(self.lib.lh_events_layout(h, C.byref(nj), *i32, *i64, C.byref(size), C.byref(ng)))
        keys = ("rows", "n_left", "n_right", "exit", "enter", "span")
        return dict(size=size.value, n_genes=ng.value,
                    junctions=[dict(zip(keys, [int(a[j]) for a in i32 + i64])) for j in range(nj.value)])

    def eval_events_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, log_offset=None,
                          want=("loglik", "events", "genes", "weighted_events", "weighted_genes", "weight_stats")):
        """K0-K2 + K5 + K10 on a family handle that has sampler tables.  Returns a dict with the members of `want`:
        loglik [n], events [n, size], genes [n, n_genes], weighted_events [size], weighted_genes [n_genes],
        weight_stats [3] (max lw, sum w, sum w^2 with lw = loglik - log_offset).  split_events() cuts a row up."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        lay = self.events_layout(h)
        ne, ng = lay["size"], lay["n_genes"]
        res, outs = _outputs(_EventsOutputs, want, log_offset, loglik=(n,), events=(n, ne), genes=(n, ng),
                             weighted_events=(ne,), weighted_genes=(ng,), weight_stats=(3,))
        self.check(self.lib.lh_eval_events_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, C.byref(outs)))
        return res

    def events_forward_batch(self, family, em):
        """K2 + K5 + K10 on caller emissions em [n][C]: (loglik [n], events [n, size])."""
        h = _handle(family)
        em = _f64(em)
        n = em.shape[0]
        ll = np.zeros(n)
        ev = np.zeros((n, self.events_layout(h)["size"]))
        self.check(self.lib.lh_events_forward_batch(h, n, em.ctypes.data_as(c_f64p), ll.ctypes.data_as(c_f64p),
                                                    ev.ctypes.data_as(c_f64p)))
        return ll, ev

    def events_profile_read(self, family):
        """(ms of K5's pass on the copy, ms of K10 and its reduction, calls) since the last read."""
        return self._profile_read("lh_events_profile_read", family, 2)

    def candidates_info(self, family):
        """(candidates registered on the handle, sites every candidate has): lh_candidates_info."""
        k, L = C.c_int32(), C.c_int32()
        self.check(self.lib.lh_candidates_info(_handle(family), C.byref(k), C.byref(L)))
        return k.value, L.value

    def candidates_layout(self, family):
        """(variable sites V, log-emission u-columns n_lem, of which the variable sites' n_vlem) of the registered
        candidate tables: lh_candidates_layout."""
        v, a, b = C.c_int32(), C.c_int32(), C.c_int32()
        self.check(self.lib.lh_candidates_layout(_handle(family), C.byref(v), C.byref(a), C.byref(b)))
        return v.value, a.value, b.value

    def set_candidates(self, family, seqs, n_sites=None):
        """K6a: registers candidate naive sequences seqs [K][L] (A,C,G,T,N = 0..4) on a family handle (a raw lh_family* or
        a Family) and returns log P_HMM(s_k) [K] (-inf: no state path produces the candidate).  L must be the family's
        alignment length (n_sites, if given, must be too)."""
        h = _handle(family)
        seqs = np.asarray(seqs)
        if seqs.ndim != 2 or seqs.shape[0] < 1:
            raise ValueError("lh_family_set_candidates: candidates must be a non-empty [K][L] array")
        if seqs.dtype.kind not in "iu" or seqs.min() < 0 or seqs.max() > 4:
            raise ValueError("lh_family_set_candidates: bases must be integers 0..4 (A,C,G,T,N)")
        for want in (lambda: n_sites, lambda: self.candidates_info(h)[1]):
            L = want()
            if L is not None and seqs.shape[1] != L:
                raise ValueError("lh_family_set_candidates: candidates have %d sites, the family's alignment %d"
                                 % (seqs.shape[1], L))
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        out = np.zeros(seqs.shape[0])
        self.check(self.lib.lh_family_set_candidates(h, seqs.shape[0], seqs.ctypes.data_as(c_u8p),
                                                     out.ctypes.data_as(c_f64p)))
        return out

    def eval_candidates_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, n_candidates=None,
                              log_offset=None, want=("loglik", "log_cand", "weighted_sum", "weight_stats")):
        """K0-K2 + K6b on a handle with candidates (set_candidates).  Returns a dict with the members of `want`:
        loglik [n], log_cand [n, K] (log P(s_k | data, t_i)), weighted_sum [K], weight_stats [3], K = the candidates
        registered on the handle (n_candidates, if given, must equal it)."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        K, _ = self.candidates_info(h)
        if n_candidates is not None and n_candidates != K:
            raise ValueError("lh_eval_candidates_batch: %d candidates expected, the handle has %d" % (n_candidates, K))
        if K == 0:
            raise RuntimeError("linearham_hip: lh_eval_candidates_batch: lh_family_set_candidates has not been called")
        if n < 1 or not _n_rows(n, arrays, log_offset):
            raise ValueError("lh_eval_candidates_batch: the per-row arrays must all have n rows")
        res, outs = _outputs(_CandidateOutputs, want, log_offset, loglik=(n,), log_cand=(n, K), weighted_sum=(K,),
                             weight_stats=(3,))
        self.check(self.lib.lh_eval_candidates_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates,
                                                     C.byref(outs)))
        return res

    def candidates_profile_read(self, family):
        """(K6a ms, K6b ms, evaluation calls) since the last read."""
        return self._profile_read("lh_candidates_profile_read", family, 2)

    # ---- K8: the most probable state path, candidate paths ----
    def sample_states(self, family):
        """ints per sample of a state path in K4's layout (lh_sample_states; 0 without sampler tables)."""
        return int(self.lib.lh_sample_states(_handle(family)))

    def eval_viterbi_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, log_offset=None,
                           want=("loglik", "states", "log_path")):
        """K0-K2 + K8 on a handle with sampler tables.  Returns a dict with the members of `want`: loglik [n], states
        [n, lh_sample_states] (the most probable state path in K4's layout; -1 where there is none), log_path [n]
        (log P(data, path | tree)), weight_stats [3]."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        if not _n_rows(n, arrays, log_offset):
            raise ValueError("lh_eval_viterbi_batch: the per-row arrays must all have n rows")
        res, outs = _outputs(_ViterbiOutputs, want, log_offset, loglik=(n,), states=((n, self.sample_states(h)), np.int32),
                             log_path=(n,), weight_stats=(3,))
        self.check(self.lib.lh_eval_viterbi_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, C.byref(outs)))
        return res

    def eval_viterbi_batch_device(self, family, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                                  num_rates, outs, stream=0):
        """lh_eval_viterbi_batch_device on device addresses; outs: dict of the output members' addresses."""
        o = _ViterbiOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.check(self.lib.lh_eval_viterbi_batch_device(_handle(family), n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr,
                                                         pi_ptr, alpha_ptr, num_rates, C.byref(o), stream))

    def viterbi_forward_batch(self, family, em):
        """K2a + K8 on caller emissions em [n][C]: (log_path [n], states [n, lh_sample_states])."""
        h = _handle(family)
        em = _f64(em)
        n = em.shape[0]
        lp = np.zeros(n)
        st = np.zeros((n, self.sample_states(h)), dtype=np.int32)
        self.check(self.lib.lh_viterbi_forward_batch(h, n, em.ctypes.data_as(c_f64p), lp.ctypes.data_as(c_f64p),
                                                     st.ctypes.data_as(c_i32p)))
        return lp, st

    def sample_forward_batch(self, family, em, words, want=()):
        """K2 + K4 on caller emissions em [n][C] and engine words [n][lh_sample_words]: (loglik [n], states
        [n, lh_sample_states], dict with the members of `want`: forward [n, forward_size], scaler_counts [n, scaler_size] --
        the arrays K4 drew from)."""
        h = _handle(family)
        em = _f64(em)
        n = em.shape[0]
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if words.shape != (n, int(self.lib.lh_sample_words(h))):
            raise ValueError("lh_sample_forward_batch: words must be [n][lh_sample_words]")
        ll = np.zeros(n)
        st = np.zeros((n, self.sample_states(h)), dtype=np.int32)
        res, outs = _outputs(_EvalOutputs, [w for w in want if w in ("forward", "scaler_counts")],
                             forward=(n, self.lib.lh_forward_size(h)),
                             scaler_counts=((n, self.lib.lh_scaler_size(h)), np.int32))
        self.check(self.lib.lh_sample_forward_batch(h, n, em.ctypes.data_as(c_f64p),
                                                    words.ctypes.data_as(C.POINTER(C.c_uint32)), ll.ctypes.data_as(c_f64p),
                                                    st.ctypes.data_as(c_i32p), C.byref(outs)))
        return ll, st, res

    def posterior_forward_batch(self, family, em):
        """K2 + K5 on caller emissions em [n][C]: (loglik [n], posterior [n, forward_size])."""
        h = _handle(family)
        em = _f64(em)
        n = em.shape[0]
        ll = np.zeros(n)
        post = np.zeros((n, self.lib.lh_forward_size(h)))
        self.check(self.lib.lh_posterior_forward_batch(h, n, em.ctypes.data_as(c_f64p), ll.ctypes.data_as(c_f64p),
                                                       post.ctypes.data_as(c_f64p)))
        return ll, post

    def set_candidate_paths(self, family, states):
        """Registers state paths states [K][lh_sample_states] as the handle's candidates (their naive sequences, with
        the paths' HMM priors) and returns log P_HMM(a_k) [K]; eval_candidates_batch then scores the paths."""
        h = _handle(family)
        states = np.ascontiguousarray(states, dtype=np.int32)
        if states.ndim != 2 or states.shape[0] < 1 or states.shape[1] != self.sample_states(h):
            raise ValueError("lh_family_set_candidate_paths: paths must be a non-empty [K][lh_sample_states] array")
        out = np.zeros(states.shape[0])
        self.check(self.lib.lh_family_set_candidate_paths(h, states.shape[0], states.ctypes.data_as(c_i32p),
                                                          out.ctypes.data_as(c_f64p)))
        return out

    def viterbi_profile_read(self, family):
        """(K8 ms, launch groups) since the last read."""
        return self._profile_read("lh_viterbi_profile_read", family)

    # ---- K6c: naive sequences of sampled states and the candidate store ----
    def naive_sequences(self, family, states):
        """K6c on states [n][lh_sample_states()]: (seqs [n][L] uint8, A,C,G,T,N = 0..4; hash [n] uint64)."""
        h = _handle(family)
        states = np.ascontiguousarray(states, dtype=np.int32)
        n = states.shape[0]
        _, L = self.candidates_info(h)
        seqs = np.zeros((n, L), dtype=np.uint8)
        hsh = np.zeros(n, dtype=np.uint64)
        self.check(self.lib.lh_naive_sequences(h, n, states.ctypes.data_as(c_i32p), seqs.ctypes.data_as(c_u8p),
                                               hsh.ctypes.data_as(C.POINTER(C.c_uint64))))
        return seqs, hsh

    def eval_draw_batch(self, family, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, words, want_states=False):
        """lh_eval_draw_batch: (loglik [n], hash [n], states [n][S] or None); the sequences stay on the handle."""
        h = _handle(family)
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        ll = np.zeros(n)
        hsh = np.zeros(n, dtype=np.uint64)
        st = np.zeros((n, self.lib.lh_sample_states(h)), dtype=np.int32) if want_states else None
        self.check(self.lib.lh_eval_draw_batch(h, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates,
                                               _ptr(words, C.POINTER(C.c_uint32)), _ptr(ll),
                                               _ptr(hsh, C.POINTER(C.c_uint64)), _ptr(st, c_i32p)))
        return ll, hsh, st

    def draws_resolve(self, family, cand):
        """lh_draws_resolve: the rows of the last batch whose bytes differ from their candidate's."""
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        rows = np.zeros(max(len(cand), 1), dtype=np.int32)
        nm = C.c_int32()
        self.check(self.lib.lh_draws_resolve(_handle(family), len(cand), cand.ctypes.data_as(c_i32p), C.byref(nm),
                                             rows.ctypes.data_as(c_i32p)))
        return rows[:nm.value].copy()

    def draws_rows_read(self, family, rows):
        h = _handle(family)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        _, L = self.candidates_info(h)
        out = np.zeros((len(rows), L), dtype=np.uint8)
        self.check(self.lib.lh_draws_rows_read(h, len(rows), rows.ctypes.data_as(c_i32p), out.ctypes.data_as(c_u8p)))
        return out

    def draws_candidates_read(self, family):
        """The candidate store: [K][L] uint8."""
        h = _handle(family)
        k = C.c_int32()
        self.check(self.lib.lh_draws_candidates_read(h, C.byref(k), None))
        _, L = self.candidates_info(h)
        out = np.zeros((k.value, L), dtype=np.uint8)
        self.check(self.lib.lh_draws_candidates_read(h, C.byref(k), out.ctypes.data_as(c_u8p)))
        return out

    def draws_reset(self, family):
        self.check(self.lib.lh_draws_reset(_handle(family)))

    def collect_profile_read(self, family):
        """(K6c ms, launches) since the last read."""
        return self._profile_read("lh_collect_profile_read", family)

    def schedule_tree(self, n_tips, children, root):
        """children: int32 [(T-2)*2]; returns (ops [T-2,4] int32, max_depth)."""
        children = np.ascontiguousarray(children, dtype=np.int32).ravel()
        ops = np.zeros((max(n_tips - 2, 0), 4), dtype=np.int32)
        depth = C.c_int32(0)
        self.check(self.lib.lh_schedule_tree(n_tips, children.ctypes.data_as(c_i32p), root,
                                             ops.ctypes.data_as(c_i32p), C.byref(depth)))
        return ops, depth.value


_LIB = None


def load_library():
    global _LIB
    if _LIB is None:
        _LIB = HipLibrary()
    return _LIB


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _handle(family):
    """The lh_family* of a Family, or the raw handle itself."""
    return family.handle if isinstance(family, Family) else family


def _ptr(a, t=c_f64p):
    return a.ctypes.data_as(t) if a is not None else None


def _tree_args(ops, brlen, er, pi, alpha):
    """The per-row inputs of a batch of trees (alpha: or rates) as the C ABI reads them: (n, the five arrays)."""
    ops = _i32(ops)
    return ops.shape[0], (ops, _f64(brlen), _f64(er), _f64(pi), _f64(alpha))


def _tree_ptrs(arrays):
    return [_ptr(arrays[0], c_i32p)] + [_ptr(a) for a in arrays[1:]]


def _n_rows(n, arrays, log_offset):
    """Whether ops is [n][T-2][4] and every other per-row array has n rows."""
    return arrays[0].ndim == 3 and all(a.shape[0] == n for a in arrays[1:]) and \
        (log_offset is None or np.asarray(log_offset).shape == (n,))


class _Slots:
    """The int32 [n] slot array of an `_at` entry point (the wrappers pass it where `node` goes)."""

    def __init__(self, a):
        self.a = _i32(a)
        assert self.a.ndim == 1


def _slots(slot):
    return _Slots(slot)


def _node_arg(node, n):
    """What an entry point takes in the place of `node`: the integer, or the pointer to a _Slots array of n entries."""
    if isinstance(node, _Slots):
        assert node.a.shape[0] == n
        return _ptr(node.a, c_i32p)
    return node


def clade_slot(n_tips, children, root, seed_tip, with_tips):
    """(path, slot) of the most recent common ancestor of a seed and other tips: host.clade_slot."""
    from . import host
    return host.clade_slot(n_tips, children, root, seed_tip, with_tips)


def seed_path(n_tips, children, root, seed_tip):
    """The `path` row of a tip: host.seed_path (the host library's walk, shared with the lineage pipelines)."""
    from . import host
    return host.seed_path(n_tips, children, root, seed_tip)


def pad_paths(paths):
    """[n][P] int32 from path rows of different lengths, -1 after each row's last entry."""
    P = max(len(p) for p in paths)
    out = np.full((len(paths), P), -1, dtype=np.int32)
    for i, p in enumerate(paths):
        out[i, :len(p)] = p
    return out


def split_events(layout, row):
    """[(exit, enter, span)] per junction: views of one flat K10 row under HipLibrary.events_layout's layout."""
    row = np.asarray(row)
    out = []
    for j in layout["junctions"]:
        W1 = j["rows"] + 1
        out.append((row[j["exit"]:j["exit"] + j["n_left"] * W1].reshape(j["n_left"], W1),
                    row[j["enter"]:j["enter"] + j["n_right"] * W1].reshape(j["n_right"], W1),
                    row[j["span"]:j["span"] + W1 * W1].reshape(W1, W1)))
    return out


def _outputs(struct, want, log_offset=None, **shapes):
    """The outputs of an evaluation: (res, outs) with res[k] a zeroed array of shapes[k] -- a shape, or (shape, dtype) --
    for every k of `want`, and `outs` the filled output struct: its members point at res and at log_offset (if it has
    one), the others stay null."""
    res = {}
    for k, v in shapes.items():
        if k in want:
            shape, dtype = v if isinstance(v[0], tuple) else (v, np.float64)
            res[k] = np.zeros(shape, dtype=dtype)
    outs = struct()
    outs.arrays = dict(res, log_offset=None if log_offset is None else _f64(log_offset))  # (keeps log_offset alive)
    for k, t in struct._fields_:
        if outs.arrays.get(k) is not None:
            setattr(outs, k, _ptr(outs.arrays[k], t))
    return res, outs


class Segments:
    def __init__(self, offsets, xmsa_inds):
        self.offsets = _i32(offsets)
        self.xmsa_inds = _i32(xmsa_inds)

    def c(self):
        return _Segments(len(self.offsets) - 1, self.offsets.ctypes.data_as(c_i32p),
                         self.xmsa_inds.ctypes.data_as(c_i32p))


class JunctionTables:
    F64 = ["enter_trans", "enter_lo", "left_trans", "left_lo", "right_gp_nli", "right_ntt", "right_nlo",
           "right_trans", "right_gp_li", "exit_nlo", "exit_trans", "exit_gp_li"]
    I32 = ["left_xmsa", "right_xmsa", "nti_xmsa"]

    def __init__(self, n_rows, n_left, n_right, **arrays):
        self.n_rows, self.n_left, self.n_right = n_rows, n_left, n_right
        for k in self.F64:
            setattr(self, k, _f64(arrays[k]))
        for k in self.I32:
            setattr(self, k, _i32(arrays[k]))

    def c(self):
        j = _Junction()
        j.n_rows, j.n_left, j.n_right = self.n_rows, self.n_left, self.n_right
        for k in self.F64:
            setattr(j, k, getattr(self, k).ctypes.data_as(c_f64p))
        for k in self.I32:
            setattr(j, k, getattr(self, k).ctypes.data_as(c_i32p))
        return j


class SamplerJunction:
    """Host-side arrays of lh_sampler_junction (keeps the numpy buffers alive)."""
    F64 = ["left_lo", "left_trans", "enter_lo", "gene_prob", "nti_landing_in", "nti_transition", "nti_landing_out",
           "landing_in", "right_trans", "exit_nlo", "exit_trans", "exit_li", "prod"]
    I32 = ["left_rows", "left_dense", "right_dense", "right_first"]

    def __init__(self, n_rows, n_left, n_right, n_states, **arrays):
        self.n_rows, self.n_left, self.n_right, self.n_states = n_rows, n_left, n_right, n_states
        for k in self.F64:
            setattr(self, k, _f64(arrays[k]))
        for k in self.I32:
            setattr(self, k, _i32(arrays[k]))

    def c(self):
        j = _SamplerJunction()
        j.n_rows, j.n_left, j.n_right, j.n_states = self.n_rows, self.n_left, self.n_right, self.n_states
        for k in self.F64:
            setattr(j, k, getattr(self, k).ctypes.data_as(c_f64p))
        for k in self.I32:
            setattr(j, k, getattr(self, k).ctypes.data_as(c_i32p))
        return j


class FamilyDesc:
    """Host-side arrays of lh_family_desc (keeps the numpy buffers alive)."""

    def __init__(self, has_d, msa, xmsa_site, xmsa_naive_base, vpadding, vgerm, dgerm, jgerm, jpadding,
                 vgerm_gene_prob, vpadding_transition, vgerm_trans_prod, jpadding_transition, vd, dj,
                 n_xmsa=None):
        self.has_d = int(has_d)
        self.msa = np.ascontiguousarray(msa, dtype=np.uint8)
        self.xmsa_site = _i32(xmsa_site)
        self.xmsa_naive_base = np.ascontiguousarray(xmsa_naive_base, dtype=np.uint8)
        self.n_xmsa = int(n_xmsa if n_xmsa is not None else len(self.xmsa_site))
        self.vpadding, self.vgerm, self.dgerm, self.jgerm, self.jpadding = vpadding, vgerm, dgerm, jgerm, jpadding
        self.vgerm_gene_prob = _f64(vgerm_gene_prob)
        self.vpadding_transition = _f64(vpadding_transition)
        self.vgerm_trans_prod = _f64(vgerm_trans_prod)
        self.jpadding_transition = _f64(jpadding_transition)
        self.vd, self.dj = vd, dj

    def c(self):
        d = _FamilyDesc()
        d.abi_version = 1
        d.has_d = self.has_d
        d.n_seqs = self.msa.shape[0] if self.msa.ndim == 2 else 0
        d.n_sites = self.msa.shape[1] if self.msa.ndim == 2 else 0
        d.msa = self.msa.ctypes.data_as(c_u8p)
        d.n_xmsa = self.n_xmsa
        d.xmsa_site = self.xmsa_site.ctypes.data_as(c_i32p)
        d.xmsa_naive_base = self.xmsa_naive_base.ctypes.data_as(c_u8p)
        d.vpadding, d.vgerm, d.jgerm, d.jpadding = (self.vpadding.c(), self.vgerm.c(), self.jgerm.c(),
                                                    self.jpadding.c())
        if self.dgerm is not None:
            d.dgerm = self.dgerm.c()
        d.vgerm_gene_prob = self.vgerm_gene_prob.ctypes.data_as(c_f64p)
        d.vpadding_transition = self.vpadding_transition.ctypes.data_as(c_f64p)
        d.vgerm_trans_prod = self.vgerm_trans_prod.ctypes.data_as(c_f64p)
        d.jpadding_transition = self.jpadding_transition.ctypes.data_as(c_f64p)
        d.vd = self.vd.c()
        if self.dj is not None:
            d.dj = self.dj.c()
        return d


class Family:
    """Owning wrapper of an lh_family handle."""

    def __init__(self, desc, lib=None):
        self.hip = lib or load_library()
        self.desc = desc
        h = C.c_void_p()
        cdesc = desc.c()
        self.hip.check(self.hip.lib.lh_family_create(C.byref(cdesc), C.byref(h)))
        self.handle = h
        self.forward_size = self.hip.lib.lh_forward_size(h)
        self.scaler_size = self.hip.lib.lh_scaler_size(h)
        self.n_xmsa = desc.n_xmsa
        self.consensus_sets = self.hip.lib.lh_family_consensus_sets(h)

    @classmethod
    def borrow(cls, handle, lib=None):
        """A wrapper of a handle somebody else owns (host.PhyloHMM's family, which has the sampler tables): the same
        methods, close() leaves the handle alone."""
        self = cls.__new__(cls)
        self.hip = lib or load_library()
        self.desc = None
        self.handle = C.c_void_p(handle) if isinstance(handle, int) else handle
        self.owned = False
        self.forward_size = self.hip.lib.lh_forward_size(self.handle)
        self.scaler_size = self.hip.lib.lh_scaler_size(self.handle)
        return self

    def close(self):
        if self.handle:
            if getattr(self, "owned", True):
                self.hip.lib.lh_family_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _outs(self, n, R, want):
        shapes = dict(rates=(n, R), forward=(n, self.forward_size), scaler_counts=((n, self.scaler_size), np.int32))
        if "xmsa_emission" in want:  # (a borrowed handle knows n_xmsa only if its owner has set it)
            shapes["xmsa_emission"] = (n, self.n_xmsa)
        res, outs = _outputs(_EvalOutputs, want, **shapes)
        return outs, res

    def eval_batch(self, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, want=()):
        _, arrays = _tree_args(ops, brlen, er, pi, alpha)
        ops, brlen, er, pi, alpha = arrays
        n = alpha.shape[0]
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4)
        ll = np.zeros(n)
        outs, res = self._outs(n, num_rates, want)
        self.hip.check(self.hip.lib.lh_eval_batch(self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates,
                                                  _ptr(ll), C.byref(outs)))
        return ll, res

    def eval_batch_device(self, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr,
                          num_rates, loglik_ptr, stream=0):
        self.hip.check(self.hip.lib.lh_eval_batch_device(
            self.handle, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates,
            loglik_ptr, None, stream))

    def info(self):
        """(distinct alignment columns, distinct (naive base, column) pairs in use): lh_family_info."""
        a, b = C.c_int32(), C.c_int32()
        self.hip.check(self.hip.lib.lh_family_info(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def k1_form(self):
        """The pruning-kernel form of the handle's last evaluation (diagnostic, lh_family_prune_form)."""
        return self.hip.lib.lh_family_prune_form(self.handle).decode()

    def k2_form(self):
        """The K2 kernels of the handle's last forward sweep (diagnostic, lh_family_forward_form)."""
        return self.hip.lib.lh_family_forward_form(self.handle).decode()

    def k2_dj_samples(self):
        """Samples per wave of the last forward sweep's D-J kernel: 4 or 2 in the pair form, else 0
        (diagnostic, lh_family_forward_dj_samples)."""
        return int(self.hip.lib.lh_family_forward_dj_samples(self.handle))

    def k2_dj_waves(self):
        """Waves per workgroup of the last forward sweep's D-J kernel: 4, 8 or 16 with four samples per wave, the
        two-sample kernel's own otherwise, 0 outside the pair form (diagnostic, lh_family_forward_dj_waves)."""
        return int(self.hip.lib.lh_family_forward_dj_waves(self.handle))

    def status(self):
        """Synchronise the device and raise if a launch since the last call met a malformed (device-resident) schedule."""
        self.hip.check(self.hip.lib.lh_family_status(self.handle))

    def forward_batch(self, em, want=()):
        em = _f64(em)
        n = em.shape[0]
        assert em.shape == (n, self.n_xmsa)
        ll = np.zeros(n)
        outs, res = self._outs(n, 1, [w for w in want if w in ("forward", "scaler_counts")])
        self.hip.check(self.hip.lib.lh_forward_batch(self.handle, n, em.ctypes.data_as(c_f64p),
                                                     ll.ctypes.data_as(c_f64p), C.byref(outs)))
        return ll, res

    def asr_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive, seed, first_sample=0):
        """lh_asr_batch: returns (anc [n][T-2][L] uint8, rate_choice [n][L] uint8)."""
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive = np.ascontiguousarray(naive, dtype=np.uint8)
        n, L = naive.shape
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n
        anc = np.zeros((n, n_tips - 2, L), dtype=np.uint8)
        choice = np.zeros((n, L), dtype=np.uint8)
        self.hip.check(self.hip.lib.lh_asr_batch(self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), rates.shape[1],
                                                 _ptr(naive, c_u8p), seed, first_sample, _ptr(anc, c_u8p),
                                                 _ptr(choice, c_u8p)))
        return anc, choice

    # ---- K11: exact ancestral-state marginals along a lineage ----
    def asr_marginals_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive_prob, path,
                            want=("marg", "rate_post")):
        """lh_asr_marginals_batch: lh_asr_batch's trees and rates, naive_prob [n][L][5] and path [n][P] (seed_path rows,
        -1 padding); returns (marg [n][P][L][4], rate_post [n][L][R]), None for what `want` leaves out."""
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive_prob = _f64(naive_prob)
        path = _i32(path)
        n, L = naive_prob.shape[:2]
        assert naive_prob.shape == (n, L, 5) and path.ndim == 2 and path.shape[0] == n
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n
        P, R = path.shape[1], rates.shape[1]
        marg = np.zeros((n, P, L, 4)) if "marg" in want else None
        rate_post = np.zeros((n, L, R)) if "rate_post" in want else None
        self.hip.check(self.hip.lib.lh_asr_marginals_batch(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), R, _ptr(naive_prob), _ptr(path, c_i32p), P,
            _ptr(marg), _ptr(rate_post)))
        return marg, rate_post

    def asr_marginals_batch_device(self, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates,
                                   naive_prob_ptr, path_ptr, path_len, marg_ptr, rate_post_ptr, stream=0):
        """lh_asr_marginals_batch_device on device addresses, enqueued on `stream`."""
        self.hip.check(self.hip.lib.lh_asr_marginals_batch_device(
            self.handle, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates, naive_prob_ptr,
            path_ptr, path_len, marg_ptr, rate_post_ptr, stream))

    def ancestral_profile_read(self):
        """({k11a_ms, k11b_ms, reduce_ms}, launch groups) of K11 since the last read."""
        r = self.hip._profile_read("lh_ancestral_profile_read", self.handle, 3)
        return dict(zip(("k11a_ms", "k11b_ms", "reduce_ms"), r[:3])), r[3]

    # ---- K14: exact codon marginals of a node of a lineage ----
    def asr_node_codons_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive_codons, path, node,
                              want=("codons", "change")):
        """lh_asr_node_codons_batch: asr_marginals_batch's trees and rates, the caller's naive codon posteriors
        naive_codons [n][C][125] (C = n_codons of set_codons' frame) and path [n][P]; returns (codons [n][C][64], change
        [n][C][4]), None for what `want` leaves out."""
        return self._asr_node_codons("lh_asr_node_codons_batch", n_tips, max_depth, ops, brlen, er, pi, rates, naive_codons,
                                     path, node, want)

    def asr_node_codons_at_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive_codons, path, slot,
                                 want=("codons", "change")):
        """asr_node_codons_batch at a node per row: slot [n], for every sample the entry of its own path."""
        return self._asr_node_codons("lh_asr_node_codons_at_batch", n_tips, max_depth, ops, brlen, er, pi, rates,
                                     naive_codons, path, _slots(slot), want)

    def asr_node_codons_at_batch_device(self, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates,
                                        naive_codons_ptr, path_ptr, path_len, slot_ptr, codons_ptr, change_ptr, stream=0):
        """lh_asr_node_codons_at_batch_device on device addresses (slot_ptr: int32 [n]; codons_ptr / change_ptr may be 0)."""
        self.hip.check(self.hip.lib.lh_asr_node_codons_at_batch_device(
            self.handle, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates, naive_codons_ptr,
            path_ptr, path_len, slot_ptr, codons_ptr or None, change_ptr or None, stream))

    def _asr_node_codons(self, entry, n_tips, max_depth, ops, brlen, er, pi, rates, naive_codons, path, node, want):
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive_codons = _f64(naive_codons)
        path = _i32(path)
        n, nc = naive_codons.shape[:2]
        assert naive_codons.shape == (n, nc, 125) and path.ndim == 2 and path.shape[0] == n
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n
        have = C.c_int32()
        self.hip.check(self.hip.lib.lh_codon_layout(self.handle, C.byref(have), None, None, None))
        if have.value != nc:
            raise ValueError("lh_asr_node_codons_batch: naive_codons has %d codons, the handle's frame %d" % (nc, have.value))
        codons = np.zeros((n, nc, 64)) if "codons" in want else None
        change = np.zeros((n, nc, 4)) if "change" in want else None
        self.hip.check(getattr(self.hip.lib, entry)(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), rates.shape[1], _ptr(naive_codons), _ptr(path, c_i32p),
            path.shape[1], _node_arg(node, n), _ptr(codons), _ptr(change)))
        return codons, change

    # ---- K15: exact amino-acid replacement posteriors along the edges of a lineage ----
    def asr_codon_edges_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive_codons, path, seed_tip,
                              want=_CODON_EDGES_TABLES, n_sites=None):
        """lh_asr_codon_edges_batch: asr_node_codons_batch's trees, rates and naive codon posteriors naive_codons
        [n][C][125], path [n][P] of tip seed_tip; returns a dict with the members of `want` among codon_counts, aa_counts,
        seed_change, edge_change, edge_load (eval_codon_edges_batch's shapes) and cond_edge [n][P][L][5][4][4] (which needs
        n_sites = L)."""
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive_codons = _f64(naive_codons)
        path = _i32(path)
        n, nc = naive_codons.shape[:2]
        assert naive_codons.shape == (n, nc, 125) and path.ndim == 2 and path.shape[0] == n
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n
        have = C.c_int32()
        self.hip.check(self.hip.lib.lh_codon_layout(self.handle, C.byref(have), None, None, None))
        if have.value != nc:
            raise ValueError("lh_asr_codon_edges_batch: naive_codons has %d codons, the handle's frame %d" % (nc, have.value))
        P = path.shape[1]
        shapes = _codon_edges_shapes(n, nc, P)
        assert "cond_edge" not in want or n_sites
        shapes["cond_edge"] = (n, P, n_sites or 0, 5, 4, 4)
        res = {k: (np.zeros(shapes[k]) if k in want else None) for k in _CODON_EDGES_TABLES + ("cond_edge",)}
        self.hip.check(self.hip.lib.lh_asr_codon_edges_batch(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), rates.shape[1], _ptr(naive_codons), _ptr(path, c_i32p),
            P, seed_tip, *[_ptr(res[k]) for k in _CODON_EDGES_TABLES + ("cond_edge",)]))
        return {k: v for k, v in res.items() if v is not None}

    # ---- K12: exact substitution posteriors along the edges of a lineage ----
    def asr_edges_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive_prob, path, seed_tip,
                        want=_EDGES_MEMBERS):
        """lh_asr_edges_batch: asr_marginals_batch's inputs and the seed's tip id (a child of every row's path[0]); returns
        a dict with the members of `want`: edge [n][P][L][4][4], naive_edge [n][L][5][4], chain_counts [n][L][4][4],
        edge_load [n][P+1], rate_post [n][L][R], tables indexed [ancestor state][descendant state].  Without "edge" the
        lean kernel runs."""
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive_prob = _f64(naive_prob)
        path = _i32(path)
        n, L = naive_prob.shape[:2]
        assert naive_prob.shape == (n, L, 5) and path.ndim == 2 and path.shape[0] == n
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n
        P, R = path.shape[1], rates.shape[1]
        res, outs = _outputs(_EdgesOutputs, want, edge=(n, P, L, 4, 4), naive_edge=(n, L, 5, 4), chain_counts=(n, L, 4, 4),
                             edge_load=(n, P + 1), rate_post=(n, L, R))
        self.hip.check(self.hip.lib.lh_asr_edges_batch(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), R, _ptr(naive_prob), _ptr(path, c_i32p), P, int(seed_tip),
            C.byref(outs)))
        return res

    def asr_edges_batch_device(self, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates,
                               naive_prob_ptr, path_ptr, path_len, seed_tip, outs, stream=0):
        """lh_asr_edges_batch_device on device addresses, enqueued on `stream`; outs: dict of the members' addresses."""
        o = _EdgesOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.hip.check(self.hip.lib.lh_asr_edges_batch_device(
            self.handle, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, rates_ptr, num_rates, naive_prob_ptr,
            path_ptr, path_len, int(seed_tip), C.byref(o), stream))

    def edges_profile_read(self):
        """({k11a_ms, k12b_ms, reduce_ms}, launch groups) of K12 since the last read."""
        r = self.hip._profile_read("lh_edges_profile_read", self.handle, 3)
        return dict(zip(("k11a_ms", "k12b_ms", "reduce_ms"), r[:3])), r[3]

    # ---- K7: the lineage of a seed sequence and the lineage store ----
    def lineage_batch(self, n_tips, max_depth, ops, brlen, er, pi, rates, naive, seed, path, first_sample=0):
        """lh_lineage_batch: lh_asr_batch's inputs and path [n][P] (inner nodes seed's parent .. root, -1 padding);
        returns (nt_hash, aa_hash), each [n][P+1] uint64, slot P = the naive sequence.  The sampled states stay on the
        handle for lineage_resolve / lineage_rows_read."""
        _, arrays = _tree_args(ops, brlen, er, pi, rates)
        ops, brlen, er, pi, rates = arrays
        naive = np.ascontiguousarray(naive, dtype=np.uint8)
        path = _i32(path)
        n, L = naive.shape
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and rates.shape[0] == n and path.shape[0] == n
        P = path.shape[1]
        nt = np.zeros((n, P + 1), dtype=np.uint64)
        aa = np.zeros((n, P + 1), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        self.hip.check(self.hip.lib.lh_lineage_batch(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), rates.shape[1], _ptr(naive, c_u8p), seed, first_sample,
            _ptr(path, c_i32p), P, _ptr(nt, u64), _ptr(aa, u64)))
        self._lineage_sites = L
        return nt, aa

    def eval_lineage_batch(self, n_tips, max_depth, ops, brlen, er, pi, alpha, num_rates, words, seed, path, draws=1,
                           first_sample=0):
        """lh_eval_lineage_batch (the chain K0-K2, K4, K6c, K3 with `draws` ancestral draws per row, K7): a dict of
        loglik [n], rates [n][R], states [n][S], naive [n][L] uint8, naive_hash [n], nt_hash and aa_hash [n][draws][P+1]
        uint64.  The batch becomes the handle's last lineage batch: flat slot ((i * draws) + d) * (P + 1) + s."""
        n, arrays = _tree_args(ops, brlen, er, pi, alpha)
        ops, brlen, er, pi, alpha = arrays
        words = np.ascontiguousarray(words, dtype=np.uint32)
        path = _i32(path)
        assert ops.shape == (n, n_tips - 2, 4) and brlen.shape == (n, 2 * n_tips - 2)
        assert er.shape == (n, 6) and pi.shape == (n, 4) and alpha.shape == (n,) and path.shape[0] == n
        P = path.shape[1]
        lib = self.hip.lib
        _, L = self.hip.candidates_info(self.handle)
        d = max(int(draws), 0)
        shapes = dict(loglik=(n,), rates=(n, num_rates), states=((n, lib.lh_sample_states(self.handle)), np.int32),
                      naive=((n, L), np.uint8), naive_hash=((n,), np.uint64), nt_hash=((n, d, P + 1), np.uint64),
                      aa_hash=((n, d, P + 1), np.uint64))
        res, outs = _outputs(_LineageEvalOutputs, shapes, **shapes)
        self.hip.check(lib.lh_eval_lineage_batch(
            self.handle, n, n_tips, max_depth, *_tree_ptrs(arrays), num_rates, _ptr(words, C.POINTER(C.c_uint32)), seed,
            first_sample, draws, _ptr(path, c_i32p), P, C.byref(outs)))
        self._lineage_sites = L
        return res

    def eval_lineage_batch_device(self, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates,
                                  words_ptr, seed, first_sample, draws, path_ptr, path_len, outs, stream=0):
        """lh_eval_lineage_batch_device on device addresses; outs: dict of the output members' addresses (loglik,
        nt_hash, aa_hash required)."""
        o = _LineageEvalOutputsDevice(**{k: int(v) for k, v in outs.items() if v})
        self.hip.check(self.hip.lib.lh_eval_lineage_batch_device(
            self.handle, n, n_tips, max_depth, ops_ptr, brlen_ptr, er_ptr, pi_ptr, alpha_ptr, num_rates, words_ptr, seed,
            first_sample, draws, path_ptr, path_len, C.byref(o), stream))
        _, self._lineage_sites = self.hip.candidates_info(self.handle)

    def lineage_eval_profile_read(self):
        """({k0_ms, k1_ms, k2_k4_k6c_ms, k3_ms, k7_ms}, launch groups) of the chain since the last read."""
        r = self.hip._profile_read("lh_lineage_eval_profile_read", self.handle, 5)
        return dict(zip(("k0_ms", "k1_ms", "k2_k4_k6c_ms", "k3_ms", "k7_ms"), r[:5])), r[5]

    def lineage_collect_device(self, n, n_tips, anc_ptr, naive_ptr, path_ptr, path_len, nt_hash_ptr, aa_hash_ptr,
                               stream=0):
        """lh_lineage_collect_device: K7 alone on device pointers, enqueued on `stream`."""
        self.hip.check(self.hip.lib.lh_lineage_collect_device(self.handle, n, n_tips, anc_ptr, naive_ptr, path_ptr,
                                                              path_len, nt_hash_ptr, aa_hash_ptr, stream))

    def lineage_resolve(self, ids):
        """lh_lineage_resolve on ids [n][P+1] (or flat): the flat slots whose bases differ from their id's."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        slots = np.zeros(max(len(ids), 1), dtype=np.int32)
        nm = C.c_int32()
        self.hip.check(self.hip.lib.lh_lineage_resolve(self.handle, len(ids), ids.ctypes.data_as(c_i32p), C.byref(nm),
                                                       slots.ctypes.data_as(c_i32p)))
        return slots[:nm.value].copy()

    def lineage_rows_read(self, slots, n_sites=None):
        """The bases [len(slots)][L] of flat slots of the last lineage batch."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        out = np.zeros((len(slots), n_sites or self._lineage_sites), dtype=np.uint8)
        self.hip.check(self.hip.lib.lh_lineage_rows_read(self.handle, len(slots), slots.ctypes.data_as(c_i32p),
                                                         out.ctypes.data_as(c_u8p)))
        return out

    def lineage_store_read(self, first=0, count=None, n_sites=None):
        """The lineage store's sequences first .. first+count-1 (default: all): [count][L] uint8."""
        k = C.c_int32()
        self.hip.check(self.hip.lib.lh_lineage_store_read(self.handle, 0, 0, C.byref(k), None))
        count = k.value - first if count is None else count
        out = np.zeros((count, n_sites or self._lineage_sites), dtype=np.uint8)
        self.hip.check(self.hip.lib.lh_lineage_store_read(self.handle, first, count, C.byref(k),
                                                          out.ctypes.data_as(c_u8p)))
        return out

    def lineage_reset(self):
        self.hip.check(self.hip.lib.lh_lineage_reset(self.handle))

    def lineage_profile_read(self):
        """(K7 ms, launches) since the last read."""
        return self.hip._profile_read("lh_lineage_profile_read", self.handle)

    def set_extended_range(self, on=True):
        self.hip.check(self.hip.lib.lh_family_set_extended_range(self.handle, int(on)))

    def set_sampler(self, vd, dj=None):
        """lh_family_set_sampler from SamplerJunction tables (dj: igh only)."""
        d = _SamplerDesc()
        d.vd = vd.c()
        if dj is not None:
            d.dj = dj.c()
        self.hip.check(self.hip.lib.lh_family_set_sampler(self.handle, C.byref(d)))

    def viterbi_forward_batch(self, em):
        """(log_path [n], states [n][S]) of caller emissions em [n][C] (set_sampler first)."""
        assert _f64(em).shape[1] == self.n_xmsa
        return self.hip.viterbi_forward_batch(self.handle, em)

    def sample_forward_batch(self, em, words, want=()):
        """(loglik [n], states [n][S], dict of `want`) of caller emissions em [n][C] and engine words (set_sampler first)."""
        assert _f64(em).shape[1] == self.n_xmsa
        return self.hip.sample_forward_batch(self.handle, em, words, want)

    def posterior_forward_batch(self, em):
        """(loglik [n], posterior [n][forward_size]) of caller emissions em [n][C] (set_sampler first)."""
        assert _f64(em).shape[1] == self.n_xmsa
        return self.hip.posterior_forward_batch(self.handle, em)

    def profile_enable(self, on=True):
        self.hip.check(self.hip.lib.lh_profile_enable(self.handle, int(on)))

    def profile_read(self):
        a, b, c, k = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self.hip.check(self.hip.lib.lh_profile_read(self.handle, C.byref(a), C.byref(b), C.byref(c),
                                                    C.byref(k)))
        return {"model_ms": a.value, "prune_ms": b.value, "forward_ms": c.value, "launch_groups": k.value}
