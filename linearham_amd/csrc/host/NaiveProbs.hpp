// Tables of exact naive-sequence probabilities (PhyloHMM::CandidatePosterior, RunNaiveProbsPipeline): translation,
// number formatting, the candidate file and the writers of the output files.  Pure host code.
#ifndef LINEARHAM_NAIVEPROBS_
#define LINEARHAM_NAIVEPROBS_

#include <cstdint>
#include <ostream>
#include <string>
#include <vector>

namespace linearham {

/// Candidates in candidate order (first appearance among the draws, or file order) with their exact posterior
/// probability and log P_HMM(s); the sampled columns when the candidates came from draws.
struct NaiveProbsTable {
  std::vector<std::string> seqs;
  std::vector<double> prob, log_prior;
  bool sampled = false;
  std::vector<int64_t> count;
  std::vector<double> freq;
};

/// Standard genetic code, reading frame 0, truncated to a multiple of 3 (util_functions.translate).  Stop codons are
/// '*'.  A codon with N translates to the one symbol all of its resolutions give (stop included), otherwise to 'X':
/// TTN -> X (F/L), CTN -> L, TAN -> X (Y/*), TRN does not occur (the alphabet is ACGTN).
std::string TranslateDna(const std::string& dna);
/// Python's repr(float): the shortest digits that read back to the same double, fixed notation for exponents
/// -4 .. 15 ("0.0001", "1e-05", "0.5", "1.0", "1e+16"), "inf", "-inf", "nan".
std::string ReprDouble(double v);
/// A candidate file: FASTA (">" headers, sequence lines joined) or one sequence per line; blank lines ignored.  Every
/// sequence must have `n_sites` characters of ACGTN (lower case accepted), at most 65 536 distinct ones, no repeats,
/// and every FASTA header must be followed by sequence lines.  Throws with the line number otherwise, and for a file
/// without sequences.
std::vector<std::string> ReadCandidateFile(const std::string& path, int n_sites);
/// The same file with the candidates' names, by the same rules: a FASTA record's name is its header up to the first
/// blank, a plain line's is "candidate_<k>", k counting the sequences from 1.
struct NamedCandidates {
  std::vector<std::string> names, seqs;
};
NamedCandidates ReadNamedCandidateFile(const std::string& path, int n_sites);
/// Candidate ancestral sequences (PhyloHMM::AncestralCandidatePosterior, RunAncestralProbsPipeline) with their exact
/// posterior probability, in file order.  N leaves a site open.
struct AncestralProbsTable {
  std::vector<std::string> names, seqs;
  std::vector<double> prob;
};
/// <prefix>.probs.tsv: name, sequence, probability ("%.17g"), ranked as RankCandidates ranks.
void WriteAncestralProbsTable(std::ostream& o, const AncestralProbsTable& t);
/// The sum of the probabilities of the candidates without an open site: distinct ones cover at most 1.
double CoveredMass(const AncestralProbsTable& t);
/// --node's values: "parent" -> 0 (the seed's parent), "mrca" -> 1, "mrca-with:<name>[,<name>...]" -> 2 (the most recent
/// common ancestor of the seed and the named sequences); throws otherwise.
int ParseLineageNode(const std::string& name);
/// --node as text: the value above and, for "mrca-with:...", the names (none empty, none repeated; whether they are
/// sequences of the family is the caller's to say).  `text` is kept for the summary files.
struct LineageNode {
  int node = 0;
  std::vector<std::string> with;
  std::string text;
  bool at_clade() const { return node == 2; }
};
LineageNode ParseLineageNodeText(const std::string& text);
/// Candidate order sorted by probability, descending, ties by candidate order.
std::vector<std::size_t> RankCandidates(const NaiveProbsTable& t);
/// <prefix>.naive.tsv: rank, NaiveSequence, probability, log_prior[, sampled_count, sampled_frequency] ("%.17g";
/// the sampled columns hold NA when t.sampled is false).  with_sampled = false leaves the two columns out.
void WriteNaiveTable(std::ostream& o, const NaiveProbsTable& t, bool with_sampled = true);
/// <prefix>.aa.fasta: ">naive_<i>_<p>" and the translation, candidates grouped by translation, p = the group's summed
/// probability (ReprDouble), groups in descending p (ties: first appearance).
void WriteAaFasta(std::ostream& o, const NaiveProbsTable& t);
/// <prefix>.dnamap: the same headers, then one "<p>,<dna>" line per candidate of the group, descending.
void WriteDnaMap(std::ostream& o, const NaiveProbsTable& t);

}  // namespace linearham

#endif  // LINEARHAM_NAIVEPROBS_
