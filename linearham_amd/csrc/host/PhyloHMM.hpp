// PhyloHMM of the MI355X-native linearham host (class surface of src/PhyloHMM.hpp:23-126).
// Per tree sample the reference builds a libpll partition, prunes every xMSA column, fills the
// emission matrices and runs the forward algorithm on one CPU core; here all of that is ONE batched
// call into the HIP library (lh_eval_batch) and this class only prepares inputs / unpacks outputs.
#ifndef LINEARHAM_PHYLOHMM_
#define LINEARHAM_PHYLOHMM_

#include <array>
#include <fstream>
#include <map>
#include <ostream>
#include <tuple>
#include <memory>
#include <string>
#include <vector>

#include "HMM.hpp"
#include "newick.hpp"

namespace linearham {

struct LineageNode;  // --node as text (NaiveProbs.hpp)

class PhyloHMM : public HMM {
 private:
  MatrixXi xmsa_;
  std::vector<std::string> xmsa_labels_, xmsa_seqs_;
  int xmsa_naive_ind_ = 0;
  VectorXd xmsa_emission_;
  VectorXi vpadding_xmsa_inds_, vgerm_xmsa_inds_, dgerm_xmsa_inds_, jgerm_xmsa_inds_, jpadding_xmsa_inds_;
  MatrixXi vd_junction_xmsa_inds_, dj_junction_xmsa_inds_;
  std::vector<int32_t> xmsa_site_;       // MSA site of each xMSA column
  std::vector<uint8_t> xmsa_base_;       // naive base of each xMSA column

  int iteration_ = 0;
  double rb_loglikelihood_ = 0, prior_ = 0, alpha_ = 1.0;
  std::vector<double> er_, pi_, sr_;
  TreeArrays tree_;
  bool have_tree_ = false;
  int num_rates_ = 1;
  double lh_loglikelihood_ = 0, logweight_ = 0;
  std::string naive_sequence_;
  const std::string* pending_newick_ = nullptr;  // RunPipeline: this row's tree, already exported

  // raw device outputs of the pending evaluation (unpacked by RunForwardAlgorithm)
  std::vector<double> pending_forward_;
  std::vector<int32_t> pending_scalers_;
  double pending_loglik_ = 0;

  void InitializeXmsaStructs();
  void CreateFamily();
  void RunForwardAlgorithm() override;
  void WriteOutputHeaders(std::ofstream& outfile) const;
  void WriteOutputLine(std::ofstream& outfile) const;
  void FormatOutputLine(std::string& line, int iteration, double rb_loglikelihood, double prior, double alpha,
                        const double* er, const double* pi, const std::string& tree, const double* sr, int num_rates,
                        double lh_loglikelihood, const RowSampler& sample) const;
  struct TsvTable;
  struct TableBatch;

 public:
  PhyloHMM(const std::string& yaml_path, int cluster_ind, const std::string& hmm_param_dir, int seed);

  const MatrixXi& xmsa() const { return xmsa_; }
  const std::vector<std::string>& xmsa_labels() const { return xmsa_labels_; }
  const std::vector<std::string>& xmsa_seqs() const { return xmsa_seqs_; }
  int xmsa_naive_ind() const { return xmsa_naive_ind_; }
  const VectorXd& xmsa_emission() const { return xmsa_emission_; }
  const VectorXi& vpadding_xmsa_inds() const { return vpadding_xmsa_inds_; }
  const VectorXi& vgerm_xmsa_inds() const { return vgerm_xmsa_inds_; }
  const MatrixXi& vd_junction_xmsa_inds() const { return vd_junction_xmsa_inds_; }
  const VectorXi& dgerm_xmsa_inds() const { return dgerm_xmsa_inds_; }
  const MatrixXi& dj_junction_xmsa_inds() const { return dj_junction_xmsa_inds_; }
  const VectorXi& jgerm_xmsa_inds() const { return jgerm_xmsa_inds_; }
  const VectorXi& jpadding_xmsa_inds() const { return jpadding_xmsa_inds_; }
  int iteration() const { return iteration_; }
  double rb_loglikelihood() const { return rb_loglikelihood_; }
  double prior() const { return prior_; }
  double alpha() const { return alpha_; }
  const std::vector<double>& er() const { return er_; }
  const std::vector<double>& pi() const { return pi_; }
  const TreeArrays& tree() const { return tree_; }
  /// Discrete-Gamma category rates; computed on the device, valid after InitializePhyloEmission().
  const std::vector<double>& sr() const { return sr_; }
  double lh_loglikelihood() const { return lh_loglikelihood_; }
  double logweight() const { return logweight_; }
  const std::string& naive_sequence() const { return naive_sequence_; }

  void InitializePhyloParameters(const std::string& newick_path, const std::vector<double>& er,
                                 const std::vector<double>& pi, double alpha, int num_rates);
  /// Same with the Newick text given directly (RunPipeline rows).
  void InitializePhyloParametersFromString(const std::string& newick, const std::vector<double>& er,
                                           const std::vector<double>& pi, double alpha, int num_rates);
  void InitializePhyloEmission();
  void RunPipeline(const std::string& input_path, const std::string& output_path, int num_rates);
  /// Test entry: the state draws of SampleNaiveSequence for the current tree and parameters with the engine's
  /// outputs GIVEN (n_words >= RawDrawsPerSample(), at most 624), once by the device sampler (lh_eval_sample_batch)
  /// and once by the host sampler (HMM::SampleRow on a std::mt19937 whose state is set so that it returns exactly these
  /// words).  States as lh_eval_sample_batch lays them out.
  // Exact posterior state marginals of the current tree (K5, lh_eval_posterior_batch), in the compact layout of
  // lh_eval_outputs.forward; NaN if the log-likelihood is not finite.  Needs the device sampler tables.
  std::vector<double> NaivePosterior(double* loglik);
  /// What the compact posteriors mean: per alignment site the distribution of the naive base over A, C, G, T, N, and
  /// the posterior of every V / D / J gene (region letter, gene name as the pipeline's VGene / DGene / JGene spell it).
  struct NaiveMarginalsResult {
    std::vector<std::array<double, 5>> site_base;
    std::vector<std::tuple<char, std::string, double>> genes;
  };
  NaiveMarginalsResult MapPosterior(const double* post) const;
  /// After InitializePhyloEmission: the exact marginals of the current tree (K5).
  NaiveMarginalsResult NaiveMarginals();
  /// Importance-weighted marginals over a RevBayes table: the first floor(burnin_frac * rows) rows are dropped
  /// (scripts/run_bootstrap_asr_ess.R:23), each row is weighted by exp(LHLogLikelihood - RBLogLikelihood), batches of at
  /// most 49 152 rows are combined in file order.  Writes <prefix>.sites.tsv, .genes.tsv and .summary.tsv.
  void RunMarginalsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                            double burnin_frac);
  /// Exact log P(s | data, tree) of every candidate naive sequence (ACGTN strings of the alignment's length) for the
  /// current tree (K6: lh_family_set_candidates + lh_eval_candidates_batch); -inf for a sequence no state path writes.
  /// After InitializePhyloParameters.  log_prior (optional) receives log P_HMM(s).
  std::vector<double> CandidatePosterior(const std::vector<std::string>& seqs, double* loglik,
                                         std::vector<double>* log_prior = nullptr);
  /// Exact posterior probabilities of naive sequences over a RevBayes table, with RunMarginalsPipeline's burn-in and
  /// weights.  The candidates are the distinct naive sequences drawn for the used rows (pass 1: K0-K2 + K4 + K6c on the
  /// same std::mt19937 stream as RunPipeline), the `max_candidates` most drawn of them, or the sequences of
  /// `candidates_path` when it is not empty; pass 2 scores them exactly (K6).  Writes <prefix>.naive.tsv, .aa.fasta,
  /// .dnamap and .summary.tsv.
  void RunNaiveProbsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                             double burnin_frac, const std::string& candidates_path, int max_candidates = 65536);
  /// The most probable annotation of the current tree (K8, lh_eval_viterbi_batch), spelled out as ApplySampledStates
  /// spells a draw: after InitializePhyloParameters.  *log_path = log P(data, annotation's state path | tree), *loglik the
  /// tree's log-likelihood (either may be null); their difference is the path's posterior given the tree.  Throws if the
  /// log-likelihood is not finite or no path has positive probability.
  RowSampler ViterbiAnnotation(double* log_path, double* loglik);
  /// The annotation columns of an output line (WriteOutputHeaders from NaiveSequence on), tab-separated, no line end.
  std::string AnnotationHeader() const;
  void AppendAnnotationColumns(std::string& line, const RowSampler& sample) const;
  /// Exact posterior probabilities of annotations (state paths) over a RevBayes table, with RunNaiveProbsPipeline's
  /// burn-in, weights, skipped-row accounting and one-device rule.  Pass 1 runs K8 on every used row and interns the rows'
  /// most probable paths; pass 2 registers the `max_candidates` paths of largest MAP weight (ties: the first row seen) and
  /// scores them exactly on every row (lh_family_set_candidate_paths + K6b); the rows' scores are added up on the host in
  /// row order, so the files do not depend on LH_PIPELINE_BATCH.  Writes <prefix>.annotations.tsv (one line per distinct
  /// annotation, paths that format alike collapsed), .best.tsv, .rows.tsv and .summary.tsv.
  void RunAnnotationsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                              double burnin_frac, int max_candidates = 65536);
  /// The exact posterior distribution of every codon of the naive sequence in reading frame `frame` (K9,
  /// lh_eval_codons_batch): codon c covers sites frame + 3c .. frame + 3c + 2; its 125 entries are indexed
  /// 25 b1 + 5 b2 + b3 over A, C, G, T, N.
  struct CodonMarginalsResult {
    int frame = 0;
    std::vector<std::array<double, 125>> codons;
  };
  /// The full table from what the device writes -- the window codons' distributions and the V | D | J gene posteriors:
  /// a codon inside one germline region gets every gene's three bases there (N where the gene writes none) with the
  /// gene's posterior.
  CodonMarginalsResult ExpandCodons(int frame, const std::vector<int32_t>& window_codon, const double* windows,
                                    const double* genes) const;
  /// After InitializePhyloParameters: the codon table of the current tree.
  CodonMarginalsResult NaiveCodonMarginals(int frame);
  /// The importance-weighted codon table over a RevBayes table, with RunMarginalsPipeline's reader, burn-in and weights.
  /// The rows' tables are added up on the host in row order, every row rescaled to the running largest log weight, so the
  /// files do not depend on LH_PIPELINE_BATCH.  Writes <prefix>.codons.tsv, .aa.tsv and .summary.tsv.
  void RunCodonMarginalsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                 double burnin_frac, int frame);
  /// codon, first_site, bases, probability: the entries above 0, numbers as ReprDouble prints them
  static void WriteCodonTable(std::ostream& o, const CodonMarginalsResult& m);
  /// codon, aa, probability: the codon table folded with TranslateDna's table (its N-codon rule included)
  static void WriteAminoAcidTable(std::ostream& o, const CodonMarginalsResult& m);
  /// The exact posteriors of the recombination events (K10, lh_eval_events_batch) in the units of the annotation columns.
  /// deletions: P(column = length, gene) for V5pDel, V3pDel, D5pDel, D3pDel, J5pDel, J3pDel (light chains: no D columns),
  /// the gene-summed rows under gene "*"; insertions: P(length) per junction ("VD", "DJ"; light chains "VJ"); spans:
  /// P(rows the left gene occupies, first row of the right gene) per junction.  Entries above 0 only.
  struct EventsResult {
    struct Deletion {
      std::string column, gene;
      int length;
      double p;
    };
    struct Insertion {
      std::string junction;
      int length;
      double p;
    };
    struct Span {
      std::string junction;
      int left_rows, right_first;
      double p;
    };
    std::vector<Deletion> deletions;
    std::vector<Insertion> insertions;
    std::vector<Span> spans;
  };
  /// The length of K10's flat row for this family (lh_events_layout's, derived from the state space alone) and the
  /// number of gene posteriors nV + nD + nJ.
  std::size_t EventsSize() const;
  std::size_t EventsGenes() const;
  /// Maps one flat row (per junction exit | enter | span) and the V | D | J gene posteriors to the columns' units.  The
  /// deletion length comes from the members the sampler reads (SampleJunctionStates / SampleGermlineState): the junction
  /// state's `del` on row a - 1 or row b, the germline region's right_del for a = 0 and left_del for b = W; V5pDel and
  /// J3pDel are functions of the gene alone and are folded from the gene posteriors.  No device is needed.
  EventsResult MapEvents(const double* events, const double* genes) const;
  /// After InitializePhyloParameters: the tables of the current tree.
  EventsResult RearrangementEvents();
  /// The importance-weighted tables over a RevBayes table, with RunMarginalsPipeline's reader, burn-in, weights and Kish
  /// ESS.  The rows' tables are added up on the host in row order, so the files do not depend on LH_PIPELINE_BATCH.
  /// Writes <prefix>.deletions.tsv, .insertions.tsv, .spans.tsv and .summary.tsv.
  void RunEventsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates, double burnin_frac);
  /// column, gene, length, probability / junction, length, probability / junction, left_rows, right_first, probability;
  /// numbers printed with %.17g
  static void WriteDeletionTable(std::ostream& o, const EventsResult& m);
  static void WriteInsertionTable(std::ostream& o, const EventsResult& m);
  static void WriteSpanTable(std::ostream& o, const EventsResult& m);
  /// K11: exact ancestral-state marginals along the lineage of the tip `seed_seq` (lh_eval_ancestral_batch).  Per lineage
  /// slot -- slot 0 the seed's parent, the last one the MRCA (naive's neighbour) -- the node, its table [L][4] over
  /// A, C, G, T, marginalised over the rate category and over the naive base, and the rate posterior [L][R].
  struct AncestralMarginalsResult {
    std::vector<int32_t> nodes;     // [P] the lineage: inner nodes in lh_schedule_tree's numbering
    std::vector<double> marg;       // [P][L][4]
    std::vector<double> rate_post;  // [L][R]
    int n_sites = 0, num_rates = 0;
    double loglik = 0.0;
  };
  /// After InitializePhyloParameters: the tables of the current tree.
  AncestralMarginalsResult AncestralMarginals(const std::string& seed_seq);
  /// The importance-weighted tables of the seed's parent and of the MRCA -- the two slots that mean the same in every
  /// tree -- and of the rate posteriors over a RevBayes table, with RunMarginalsPipeline's reader, burn-in, weights
  /// exp(LHLogLikelihood - Likelihood), Kish ESS and one-device rule.  The rows' tables are added up on the host in row
  /// order, so the files do not depend on LH_PIPELINE_BATCH.  Writes <prefix>.parent.tsv and .mrca.tsv (site, four
  /// probabilities, the arg-max base), .rates.tsv, .rows.tsv (row, weight, chain_length) and .summary.tsv.
  void RunAncestralMarginalsPipeline(const std::string& input_path, const std::string& seed_seq,
                                     const std::string& output_prefix, int num_rates, double burnin_frac);
  /// K12: exact substitution posteriors along the edges of the lineage of the tip `seed_seq` (lh_eval_edges_batch).  Tables
  /// are indexed [ancestor state][descendant state], naive the oldest node.
  struct LineageSubstitutionsResult {
    struct Edge {
      int32_t upper = 0, lower = 0;  // nodes in lh_schedule_tree's numbering (0 = naive, tips 1 .. T-1)
      double brlen = 0.0;            // of the lower node's branch (the naive edge: naive's)
      double load = 0.0;             // the expected number of sites whose two ends differ
    };
    std::vector<int32_t> nodes;        // [P] the lineage: slot 0 the seed's parent, the last one the MRCA
    std::vector<Edge> edges;           // [P+1]: [s] the edge below slot s ([0] ends at the seed tip), [P] naive -> MRCA
    std::vector<double> edge;          // [P][L][4][4]
    std::vector<double> naive_edge;    // [L][5][4]
    std::vector<double> chain_counts;  // [L][4][4] expected number of lineage edges on which the site goes from a to c
    int n_sites = 0;
    double loglik = 0.0;
  };
  /// After InitializePhyloParameters: the tables of the current tree.
  LineageSubstitutionsResult LineageSubstitutions(const std::string& seed_seq);
  /// The importance-weighted chain_counts, seed-edge and naive-edge tables -- the three that mean the same in every tree --
  /// over a RevBayes table, with RunAncestralMarginalsPipeline's reader, burn-in, weights, Kish ESS and one-device rule.
  /// Only the per-row reductions come back from the device (the lean kernel runs); they are added up on the host in row
  /// order, so the files do not depend on LH_PIPELINE_BATCH.  Writes <prefix>.substitutions.tsv (site, the 16 weighted
  /// counts, their off-diagonal sum), .seed_edge.tsv, .naive_edge.tsv, .rows.tsv (row, weight, chain_length, the row's
  /// expected number of differing edge ends over all sites) and .summary.tsv.
  void RunLineageSubstitutionsPipeline(const std::string& input_path, const std::string& seed_seq,
                                       const std::string& output_prefix, int num_rates, double burnin_frac);
  /// K13: exact posterior probabilities of whole candidate sequences at a node of the lineage of the tip `seed_seq`
  /// (lh_eval_ancestral_candidates_batch): node 0 = the seed's parent, 1 = the MRCA; candidates of the alignment's length
  /// over ACGTN, N leaving the site open.
  struct AncestralCandidateResult {
    std::vector<double> log_cand;  // [K] log P(X_node = x_k | data, tree)
    int32_t node = 0;              // the node in lh_schedule_tree's numbering
    double loglik = 0.0;
  };
  /// After InitializePhyloParameters: the candidates' log probabilities under the current tree.
  /// `with` not empty: the node is the most recent common ancestor of the seed and the sequences named there
  /// (lh_eval_ancestral_candidates_at_batch at CladeSlot's slot) and `node` is not looked at; a name that is no sequence
  /// of the family, the seed itself and 'naive' are refused before any device work.
  AncestralCandidateResult AncestralCandidatePosterior(const std::string& seed_seq, int node,
                                                       const std::vector<std::string>& candidates,
                                                       const std::vector<std::string>& with = {});
  /// The importance-weighted probabilities of the candidates of `candidates_path` (ReadNamedCandidateFile) over a RevBayes
  /// table, with RunAncestralMarginalsPipeline's reader, burn-in, weights, Kish ESS and one-device rule.  The node and the
  /// candidate file are checked first, before any device work.  The rows' probabilities are added up on the host in row
  /// order, so the files do not depend on LH_PIPELINE_BATCH.  Writes <prefix>.probs.tsv (name, sequence, probability,
  /// ranked), .rows.tsv (row, weight, chain_length) and .summary.tsv (rows used and skipped, Kish ESS, the candidates,
  /// those without an open site and the posterior mass these cover).
  void RunAncestralProbsPipeline(const std::string& input_path, const std::string& seed_seq, int node,
                                 const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                 double burnin_frac);
  /// The same with the node as --node's text (ParseLineageNodeText).  For 'mrca-with:<names>' the node is the most recent
  /// common ancestor of the seed and the named sequences, at a slot of its own in every row: .rows.tsv gains the column
  /// `slot` and .summary.tsv the lines node, slot_min and slot_max.  For 'parent' and 'mrca' the files are the int form's.
  void RunAncestralProbsPipeline(const std::string& input_path, const std::string& seed_seq, const std::string& node_text,
                                 const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                 double burnin_frac);
  /// K14: exact codon marginals of a node of the lineage of the tip `seed_seq` (lh_eval_node_codons_batch): node 0 = the
  /// seed's parent, 1 = the MRCA; codon c covers the sites frame + 3 c ...  A node triple is indexed 16 x1 + 4 x2 + x3 over
  /// ACGT; change = the probabilities that the node's codon is identical to the naive one, a synonymous change of it, an
  /// amino-acid replacement, or undetermined (the naive triple holds an N).
  struct NodeCodonsResult {
    int frame = 0;
    int32_t node = 0;  // the node in lh_schedule_tree's numbering (-1: a weighted mean over trees)
    double loglik = 0.0;
    std::vector<std::array<double, 64>> codons;
    std::vector<std::array<double, 4>> change;
  };
  /// After InitializePhyloParameters: the tables of the current tree.  The node and the frame are checked first.
  /// `with` not empty: as AncestralCandidatePosterior's (lh_eval_node_codons_at_batch).
  NodeCodonsResult NodeCodonMarginals(const std::string& seed_seq, int node, int frame,
                                      const std::vector<std::string>& with = {});
  /// The importance-weighted tables over a RevBayes table, with RunAncestralMarginalsPipeline's reader, burn-in, weights,
  /// Kish ESS and one-device rule.  What needs no device (the node, the frame, the burn-in, the seed) is refused before the
  /// family is created.  The rows' tables are added up on the host in row order, so the files do not depend on
  /// LH_PIPELINE_BATCH.  Writes <prefix>.codons.tsv (codon, first site, node triple, probability), .aa.tsv (codon, amino
  /// acid, probability), .changes.tsv (codon, identical, synonymous, replacement, undetermined), .rows.tsv (row, weight,
  /// chain_length) and .summary.tsv (with frame, node, expected_synonymous and expected_replacement, the column sums of
  /// the changes table).
  void RunNodeCodonsPipeline(const std::string& input_path, const std::string& seed_seq, int node,
                             const std::string& output_prefix, int num_rates, double burnin_frac, int frame);
  /// The same with the node as --node's text, as RunAncestralProbsPipeline's text form: for 'mrca-with:<names>' .rows.tsv
  /// gains `slot`, .summary.tsv's node line holds the text and slot_min and slot_max follow it.
  void RunNodeCodonsPipeline(const std::string& input_path, const std::string& seed_seq, const std::string& node_text,
                             const std::string& output_prefix, int num_rates, double burnin_frac, int frame);
  /// numbers printed with %.17g; entries of probability 0 are left out of the first two
  static void WriteNodeCodonTable(std::ostream& o, const NodeCodonsResult& m);
  static void WriteNodeAminoAcidTable(std::ostream& o, const NodeCodonsResult& m);
  static void WriteChangeTable(std::ostream& o, const NodeCodonsResult& m);
  /// K15: exact amino-acid replacement posteriors along the edges of the lineage of the tip `seed_seq`
  /// (lh_eval_codon_edges_batch); codon c covers the sites frame + 3 c ...  The lineage has nodes.size() + 1 edges: slot s
  /// from nodes[s] to nodes[s - 1] (slot 0: to the seed), the last entry the naive edge.  Amino acids are indexed by their
  /// place in kAaSymbols, the stop codons a symbol of their own.
  static constexpr const char* kAaSymbols = "ACDEFGHIKLMNPQRSTVWY*";
  struct LineageReplacementsResult {
    int frame = 0;
    double loglik = 0.0;
    std::vector<int32_t> nodes;                          // the chain, the seed's parent first (empty: a weighted mean)
    std::vector<std::array<double, 4>> codon_counts;     // expected edges: unchanged, synonymous, replacement; naive triple with an N
    std::vector<std::array<double, 441>> aa_counts;      // [from][to] expected edges
    std::vector<std::array<double, 3>> seed_change;      // the edge into the seed alone
    std::vector<double> edge_change;                     // [nodes.size() + 1][n_codons][3]
    std::vector<std::array<double, 2>> edge_load;        // per edge: expected codons changing silently / by replacement
  };
  /// After InitializePhyloParameters: the tables of the current tree.  The frame is checked first.
  LineageReplacementsResult LineageReplacements(const std::string& seed_seq, int frame);
  /// The importance-weighted tables over a RevBayes table, with RunLineageSubstitutionsPipeline's reader, burn-in, weights,
  /// Kish ESS and one-device rule.  The seed, the frame and the burn-in are refused before the family is created.  The rows'
  /// tables are added up on the host in row order, so the files do not depend on LH_PIPELINE_BATCH.  Writes
  /// <prefix>.replacements.tsv (codon, first site, from, to, expected edges: the non-zero off-diagonal cells),
  /// .codon_changes.tsv (codon, unchanged, synonymous, replacement, undetermined), .seed_edge.tsv (codon, unchanged,
  /// synonymous, replacement), .rows.tsv (row, weight, chain_length, expected_synonymous, expected_replacement) and
  /// .summary.tsv (with frame, expected_synonymous and expected_replacement, the column sums of the codon changes).
  void RunLineageReplacementsPipeline(const std::string& input_path, const std::string& seed_seq, const std::string& output_prefix,
                                      int num_rates, double burnin_frac, int frame);
  /// numbers printed with %.17g; the first leaves out the diagonal and the cells that are 0
  static void WriteReplacementTable(std::ostream& o, const LineageReplacementsResult& m);
  static void WriteCodonChangeTable(std::ostream& o, const LineageReplacementsResult& m);
  static void WriteSeedChangeTable(std::ostream& o, const LineageReplacementsResult& m);
  /// site, then one column per cell named <ancestor base><descendant base> (n_rows x 4 cells, rows over ACGTN), and with
  /// `with_sum` the off-diagonal sum of the first four rows; numbers printed with %.17g
  static void WritePairTable(std::ostream& o, const double* table, std::size_t n_sites, int n_rows, bool with_sum);
  /// site, A, C, G, T, map_base / site, rate0 ..; numbers printed with %.17g
  static void WriteNodeTable(std::ostream& o, const double* table, std::size_t n_sites);
  static void WriteRateTable(std::ostream& o, const double* rate_post, std::size_t n_sites, int num_rates);
  /// The tip (1 .. T-1) of a sequence of the clonal family; throws for 'naive' and for names the family does not hold.
  int SeedTip(const std::string& seed_seq) const;
  static void WriteSiteTable(std::ostream& o, const NaiveMarginalsResult& m);
  static void WriteGeneTable(std::ostream& o, const NaiveMarginalsResult& m);
  void SampleStatesWithWords(const uint32_t* words, int n_words, std::vector<int32_t>& device_states,
                             std::vector<int32_t>& host_states);

  /// The per-tree body of scripts/run_bootstrap_asr_ess.R:48-104 for every row of a RunPipeline output table
  /// (columns er[1..6], pi[1..4], tree, sr[1..R], NaiveSequence): per alignment site a rate category is drawn
  /// with the column likelihoods on the rate-scaled trees, then the inner-node states are drawn jointly given
  /// the tips (K3, lh_asr_batch).  Writes one Newick string per row, rooted on the naive branch as
  /// ape::root(tree, "naive", resolve.root = TRUE) does, every node annotated [&ancestral="<L bases>"] (tips:
  /// their observed sequence).  Random numbers: Philox stream `seed`, sample number = row number.
  void RunAsr(const std::string& input_path, const std::string& output_path, uint64_t seed);
  /// The lineage tables of the tip `seed_seq` (scripts/tabulate_lineage_probs.py) straight from a RunPipeline table:
  /// RunAsr's input, parsing, batches and draws (Philox stream `seed`, sample number = row number), but the sampled
  /// states stay on the device.  Per batch K3 + K7 (lh_lineage_batch) hand back two hashes per lineage node; the host
  /// assigns sequence ids by hash, lh_lineage_resolve settles every assignment by the bases themselves, and only the
  /// bases of sequences first seen are read back.  Writes <prefix>.fasta, .dnamap, .nodes.tsv, .edges.tsv and
  /// .summary.tsv (Lineage.hpp): what TabulateLineageTrees makes of RunAsr's output for the same table and seed.
  /// LH_LINEAGE_BATCH=n sets the rows per batch (default 1 024, RunAsr's).
  void RunLineagePipeline(const std::string& input_path, const std::string& seed_seq, const std::string& output_prefix,
                          uint64_t seed);
  /// Importance-weighted lineage tables straight from the RevBayes table, in one pass: RunNaiveProbsPipeline's burn-in
  /// (the first floor(burnin_frac * rows) rows), weights (lw_i = LHLogLikelihood_i - Likelihood_i, w_i = exp(lw_i - max lw),
  /// rows with a non-finite lw skipped and counted) and one-device rule; per row the naive sequence `--pipeline --seed s`
  /// prints for it (the same std::mt19937 words) and `draws_per_row` (1 .. 64) ancestral draws on K0a's full-precision
  /// rates (Philox stream `seed`, sample number = table row, draw d in the upper 32 bits: lh_eval_lineage_batch).  Every
  /// (row, draw) is one tree of weight w_i, counted in (row, draw) order after the last batch (the id lists wait until
  /// the largest log-weight is known: the result does not depend on LH_LINEAGE_BATCH; more than 1 GiB of them is
  /// refused).  Writes the five lineage files -- counts are weighted sums, fractions sum / (draws x sum w), the summary
  /// gains rows_used, rows_skipped_nonfinite, draws_per_row and kish_ess -- and <prefix>.rows.tsv (row, lh_loglik,
  /// log_weight, weight, naive_id, path_len per row after the burn-in).
  void RunWeightedLineagePipeline(const std::string& input_path, const std::string& seed_seq,
                                  const std::string& output_prefix, int num_rates, double burnin_frac, int draws_per_row,
                                  uint64_t seed);
  /// One annotated tree (RunAsr's output line) from the sampled states anc[(T-2)][L] of a row.
  std::string AnnotatedNewick(const TreeArrays& tree, const std::string& naive_sequence, const uint8_t* anc) const;

  /// Batched log-likelihoods of many tree samples (the GPU-native entry point RunPipeline uses).
  /// Rows are (newick, er[6], pi[4], alpha).  Returns HMM::LogLikelihood() per row.
  struct TreeSample {
    std::string newick;
    std::vector<double> er, pi;
    double alpha;
  };
  std::vector<double> LogLikelihoodBatch(const std::vector<TreeSample>& samples, int num_rates);

  /// Flattened device inputs of a batch (used by LogLikelihoodBatch and by the benchmark harness).
  struct DeviceBatch {
    int n = 0, n_tips = 0, max_depth = 0;
    std::vector<int32_t> ops;
    std::vector<double> brlen, er, pi, alpha;
  };
  /// `trees` / `exported` (optional): the parsed trees and their re-exported Newick strings, produced by the
  /// same worker threads (RunPipeline needs both per row and would otherwise redo them one by one).
  DeviceBatch FlattenBatch(const std::vector<TreeSample>& samples, std::vector<TreeArrays>* trees = nullptr,
                           std::vector<std::string>* exported = nullptr) const;
  /// The whole RevBayes table `path` as device inputs (rows parsed and scheduled by worker threads).
  DeviceBatch FlattenTsv(const std::string& path, int* n_rows) const;
  /// Only the table rows `row_ids[0..n)` (any order, repeats allowed), in that order.
  DeviceBatch FlattenTsvRows(const std::string& path, const int64_t* row_ids, int n, int* n_rows) const;
  lh_family* family() {
    CreateFamily();
    return family_;
  }
  /// Opt-in extended-range arithmetic of the device path (lh_family_set_extended_range): finite log-likelihoods
  /// where the reference's equalisation overflows or its exp underflows; off by default.
  void SetExtendedRange(bool on);
  /// The HIP devices RunPipeline uses (before the first evaluation): one family handle and one host thread per
  /// entry, table row i evaluated and sampled on devices[i mod N], output in file order -- the split of
  /// src/PhyloHMM.cpp:414-442's loop over one node's GPUs.  The same device may be listed more than once (two
  /// handles on one GPU).  Single-row members (LogLikelihood, SampleNaiveSequence ...) use devices[0].
  void SetDevices(const std::vector<int>& devices);
  int n_xmsa() const { return xmsa_.cols(); }

 private:
  TableBatch FlattenTable(const TsvTable& table, std::size_t r0, std::size_t r1, bool with_export, bool with_scalars,
                          const std::string& path, bool with_children = false) const;
  /// What the pipelines over a RevBayes table refuse before any file is opened, in this order: more than one device
  /// ("the <what> pipeline ..."), the burn-in fraction, the seed sequence (returns its tip; 0 without one), then a
  /// family without sampler tables ("needed by the <kernel> kernel").
  int BeginPipeline(const std::string& what, const std::string& kernel, double burnin_frac, const std::string* seed_seq = nullptr);
  struct WeightedRows;
  template <class Batch>
  WeightedRows SumWeightedRows(const std::string& what, const TsvTable& table, const std::string& input_path, std::size_t first,
                               std::size_t batch_rows, std::size_t width, bool with_children, Batch&& batch) const;
  struct SeedLineage;
  SeedLineage OpenSeedLineage(const std::string& seed_seq);
  struct SeedChains;
  SeedChains SeedChainsOf(const TableBatch& tb, std::size_t off, int seed_tip, const std::string& seed_seq, int32_t* path_len) const;
  static void WriteSeedRows(std::ostream& rows, std::size_t first, const WeightedRows& w, const std::vector<int32_t>& path_len,
                            const char* extra_name = nullptr, const std::vector<double>* extra = nullptr);
  /// The tips of the sequences `with` names, to join the seed (tip seed_tip) with: no device is touched.  Throws, naming
  /// the name, for 'naive', the seed itself and a name that is no sequence of the family.
  std::vector<int32_t> WithTips(int seed_tip, const std::vector<std::string>& with) const;
  /// slot[m] of a batch of table rows (CladeSlot under every row's own tree); nothing is done for an empty `with_tips`
  std::vector<int32_t> CladeSlotsOf(const TableBatch& tb, int seed_tip, const std::vector<int32_t>& with_tips) const;
  void RunAncestralProbsPipelineAt(const std::string& input_path, const std::string& seed_seq, const LineageNode& node,
                                   const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                   double burnin_frac);
  void RunNodeCodonsPipelineAt(const std::string& input_path, const std::string& seed_seq, const LineageNode& node,
                               const std::string& output_prefix, int num_rates, double burnin_frac, int frame);
  struct AsrRow;
  /// The rows of a RunPipeline table as RunAsr and RunLineagePipeline read them; *num_rates = the sr[] columns.
  std::vector<AsrRow> ReadAsrRows(const std::string& input_path, int* num_rates) const;
  /// lh_asr_batch's rates [m][R] and naive [m][L] of rows off .. off+m-1, and their tree samples.
  void EncodeAsrRows(const std::vector<AsrRow>& rows, std::size_t off, std::size_t m, int num_rates,
                     std::vector<TreeSample>* samples, std::vector<double>* rates, std::vector<uint8_t>* naive) const;
};

typedef std::shared_ptr<PhyloHMM> PhyloHMMPtr;

void StoreGermlinePaddingXmsaIndices(const std::vector<int>& naive_bases, const std::vector<int>& site_inds,
                                     std::map<std::pair<int, int>, int>& xmsa_ids, VectorXi& xmsa_inds);
void StoreJunctionXmsaIndices(const std::vector<int>& naive_bases, const std::vector<int>& site_inds,
                              std::pair<int, int> left_flexbounds, std::pair<int, int> right_flexbounds,
                              std::map<std::pair<int, int>, int>& xmsa_ids, MatrixXi& xmsa_inds);
void StoreXmsaIndex(std::pair<int, int> id, std::map<std::pair<int, int>, int>& xmsa_ids, int& xmsa_ind);

}  // namespace linearham

#endif  // LINEARHAM_PHYLOHMM_
