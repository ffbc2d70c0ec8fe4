// Ancestral lineage tables of a seed sequence (scripts/tabulate_lineage_probs.py:95-144): which amino-acid sequences
// stood on the path from the naive sequence to the seed, in how many trees, and which followed which.  Pure host code.
#ifndef LINEARHAM_LINEAGE_
#define LINEARHAM_LINEAGE_

#include <cstdint>
#include <map>
#include <ostream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace linearham {

/// The finished tables.  Nodes are in node_c.most_common() order (descending count, ties by first appearance), edges
/// likewise; a count is the sum of the weights of the trees that count (whole numbers when every tree weighs 1, the
/// script's case), fractions are count / total, total = the sum of all trees' weights.
struct LineageTables {
  struct Node {
    std::string name, kind, aa;  // kind: seed / naive / intermediate
    double count = 0;
    std::vector<std::pair<double, std::string>> dna;  // node_dt[aa].most_common(): (count, nucleotide sequence)
  };
  struct Edge {
    int parent = 0, child = 0;  // indices into nodes; never equal
    double count = 0;
  };
  std::vector<Node> nodes;
  std::vector<Edge> edges;
  int64_t num_trees = 0, distinct_nt = 0, distinct_aa = 0, longest_path = 0;
  double total = 0;       // sum of the trees' weights (= num_trees when none was given)
  bool weighted = false;  // some tree was added with a weight of its own: counts print as doubles
};

/// What the weighted entry points add to .summary.tsv.
struct LineageWeightSummary {
  int64_t rows_used = 0, rows_skipped_nonfinite = 0;
  int draws_per_row = 1;
  double kish_ess = 0;  // (sum w)^2 / sum w^2 over the used rows
};

/// The script's counting.  A tree is its lineage as a list of nucleotide sequences naive, root, ..., seed's parent,
/// seed (the script's reversed `l`); the rules, oddities included:
///  - node_c: each distinct translation of a tree counts once for that tree;
///  - node_dt: for every run of consecutive equal translations, each distinct nucleotide sequence of the run counts
///    once, so a translation that returns after a change counts its nucleotide sequences again;
///  - edge_c: consecutive pairs of translations; pairs with equal ends are never shown by the script and are left out;
///  - "first appearance" is list order inside a tree (the script iterates a frozenset there, which has no order).
class LineageTabulator {
 public:
  /// Registers a nucleotide sequence (translated once) and returns its id; equal sequences share an id.
  int AddSequence(const std::string& nt);
  /// One tree, as ids from AddSequence; `path_len` (inner nodes between seed and naive) feeds longest_path.  The tree
  /// counts `weight` wherever the script counts 1 (sums of ones are exact: the unweighted tables are the script's).
  void AddTree(const std::vector<int>& ids, int path_len, double weight = 1.0);
  void AddTree(const std::vector<std::string>& seqs, int path_len, double weight = 1.0);
  /// The tables' counts are to print as doubles even if every weight was 1 (the weighted entry points).
  void SetWeighted() { weighted_ = true; }
  /// Names as the script gives them: the seed's translation is `seed_name`; a translation that is some tree's naive
  /// translation is naive_<i>_<fraction> as tabulate_naive_probs.py:57-60 numbers them over these trees' naive
  /// sequences; every other is intermediate_<i>_<fraction>.  Throws if no tree was added or the seeds' translations
  /// differ (the script's assert len(seed_s) == 1).
  LineageTables Finish(const std::string& seed_name) const;

 private:
  struct Counted {  // a Counter: insertion-ordered keys with counts
    std::vector<int> keys;
    std::vector<double> counts;
    std::unordered_map<int, int> at;  // key -> position, kept once there are more than kLinear keys
    static constexpr std::size_t kLinear = 8;
    void Add(int key, double weight);
    std::vector<int> MostCommon() const;  // positions into keys
  };
  std::vector<std::string> nt_, aa_;
  std::vector<int> aa_of_nt_;
  std::unordered_map<std::string, int> nt_id_, aa_id_;
  Counted node_c_, naive_c_;
  std::vector<Counted> node_dt_;  // aa -> Counter of nt
  std::vector<std::pair<int, int>> edge_keys_;
  std::vector<double> edge_counts_;
  std::map<std::pair<int, int>, int> edge_at_;
  std::vector<int> seed_aa_;  // distinct seed translations
  int64_t num_trees_ = 0, longest_path_ = 0;
  double total_ = 0;
  bool weighted_ = false;
};

/// find_muts: "<orig><1-based position><mutated>" for every differing position, space-separated.
std::string FindMuts(const std::string& orig, const std::string& mutated);

/// <prefix>.fasta and .dnamap byte for byte as the script writes them; .nodes.tsv (name, kind, count, fraction),
/// .edges.tsv (parent, child, count, fraction, parent_fraction, mutations) and .summary.tsv (rows, distinct_nt,
/// distinct_aa, longest_path, hash_collisions_resolved; with `ws` also rows_used, rows_skipped_nonfinite, draws_per_row and
/// kish_ess, %.17g).  Fractions print as Python's str(float); counts as integers, or -- weighted tables -- as str(float).
void WriteLineageFasta(std::ostream& o, const LineageTables& t);
void WriteLineageDnaMap(std::ostream& o, const LineageTables& t);
void WriteLineageNodes(std::ostream& o, const LineageTables& t);
void WriteLineageEdges(std::ostream& o, const LineageTables& t);
void WriteLineageSummary(std::ostream& o, const LineageTables& t, int64_t collisions,
                         const LineageWeightSummary* ws = nullptr);
void WriteLineageFiles(const std::string& prefix, const LineageTables& t, int64_t collisions,
                       const LineageWeightSummary* ws = nullptr);

/// Importance weights of rows from their log-weights: w_i = exp(lw_i - max lw) over the finite lw_i, 0 for the others
/// (which `ws` counts as skipped); ws->kish_ess = (sum w)^2 / sum w^2.  Throws if no log-weight is finite.
std::vector<double> LineageWeights(const std::vector<double>& log_weights, LineageWeightSummary* ws);

/// The `path` row of a tip under a tree in the C ABI's rooted-at-naive arrays (children [(T-2)*2] of the inner nodes
/// T .. 2T-3, root = naive's neighbour): the inner nodes from the tip's parent up to the root, each the child of the next
/// (lh_lineage_batch's and lh_asr_marginals_batch's convention).  Empty if the tip does not hang below the root or is not
/// one of the tips 1 .. T-1.
std::vector<int32_t> SeedPath(const int32_t* children, int n_tips, int root, int seed_tip);

/// The seed's path (SeedPath) and the index on it of the first node that is an ancestor of every tip of `with_tips`: the
/// most recent common ancestor of the seed and those tips, which is the largest, over the tips, of the slot at which the
/// tip's own path joins the seed's.  That node means the same in every tree sample; its slot does not.  Throws
/// std::invalid_argument, naming the offender, for an empty list, tip 0 (naive: that node is the MRCA), a tip outside
/// 1 .. T-1, the seed itself, a repeated tip, and a seed or tip that does not hang below the root.
struct CladeSlotResult {
  std::vector<int32_t> path;
  int slot = 0;
};
CladeSlotResult CladeSlot(const int32_t* children, int n_tips, int root, int seed_tip, const std::vector<int32_t>& with_tips);

/// One line of PhyloHMM::RunAsr's output (annotated Newick): the [&ancestral="..."] strings on the way seed, its
/// ancestors up to the top node, then the tip `naive`, as seqs_of_tree collects them, reversed (naive first).
/// Throws when the tree has no tip `seed_seq` or `naive`, or a node on the way has no annotation.
std::vector<std::string> LineageOfAnnotatedTree(const std::string& newick, const std::string& seed_seq);

/// tabulate_lineage_probs.py for a file of RunAsr lines: needs no family and no device.  Writes the five files.
/// `weights_path` (optional): one log-weight per tree line (a table's LogWeight column); tree k then counts
/// exp(lw_k - max lw), lines whose log-weight is not finite are skipped and counted, and the summary gains the weighted
/// keys.  The two files must have the same number of lines.
void TabulateLineageTrees(const std::string& trees_path, const std::string& seed_seq, const std::string& prefix,
                          const std::string& weights_path = "");

}  // namespace linearham

#endif  // LINEARHAM_LINEAGE_
