// `linearham` command line (same sub-commands and flag names as src/linearham.cpp:268-455 of the
// reference, without TCLAP): --compute-logl | --sample | --pipeline; plus --asr, the per-tree body of
// scripts/run_bootstrap_asr_ess.R:48-104 on a --pipeline output table, and --marginals / --marginals-pipeline, the exact
// posterior of the naive sequence (one tree / importance-weighted over a RevBayes table), and --naive-probs /
// --naive-probs-pipeline, exact posterior probabilities of naive sequences (tabulate_naive_probs.py's table), and
// --lineage-pipeline / --lineage-trees, the ancestral lineage tables of a seed sequence (tabulate_lineage_probs.py's), and
// --viterbi / --annotations-pipeline, the most probable annotation of one tree and the exact posterior probabilities of
// annotations over a RevBayes table (write_lh_annotations.py's counting, without the sampling), and --codon-marginals /
// --codon-marginals-pipeline, the exact codon and amino-acid distributions of the naive sequence (the logo
// tabulate_naive_probs.py draws from sampled sequences), and --events / --events-pipeline, the exact posteriors of the
// deletion and insertion lengths (the annotation's event columns).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "Lineage.hpp"
#include "NaiveProbs.hpp"
#include "PhyloHMM.hpp"

namespace {

struct Args {
  std::map<std::string, std::vector<std::string>> v;
  const std::string& one(const std::string& k) const {
    auto it = v.find(k);
    if (it == v.end() || it->second.empty()) throw std::invalid_argument("Required argument missing: " + k);
    if (it->second.size() > 1) throw std::invalid_argument("Argument already set! for arg --" + k);
    return it->second[0];
  }
  std::string opt(const std::string& k, const std::string& dflt) const {
    auto it = v.find(k);
    return (it == v.end() || it->second.empty()) ? dflt : it->second.back();
  }
  std::vector<double> multi(const std::string& k) const {
    auto it = v.find(k);
    if (it == v.end() || it->second.empty()) throw std::invalid_argument("Required argument missing: " + k);
    std::vector<double> out;
    for (const auto& s : it->second) out.push_back(std::stod(s));
    return out;
  }
};

Args Parse(int argc, char** argv, int first) {
  Args a;
  for (int i = first; i < argc; ++i) {
    std::string k = argv[i];
    if (k.rfind("--", 0) != 0) throw std::invalid_argument("Couldn't find match for argument " + k);
    k = k.substr(2);
    if (i + 1 >= argc) throw std::invalid_argument("Missing a value for this argument! --" + k);
    a.v[k].push_back(argv[++i]);
  }
  return a;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc < 2 || std::string(argv[1]) == "-h" || std::string(argv[1]) == "--help") {
      std::cout << "A Phylo-HMM implementation for B cell receptor sequence analysis.\n"
                   "USAGE: linearham {--compute-logl|--sample|--pipeline|--asr|--marginals|--marginals-pipeline|--naive-probs|--naive-probs-pipeline|--lineage-pipeline|--weighted-lineage-pipeline|--viterbi|--annotations-pipeline|--codon-marginals|--codon-marginals-pipeline|--events|--events-pipeline|--ancestral-marginals|--ancestral-marginals-pipeline|--lineage-substitutions|--lineage-substitutions-pipeline|--ancestral-probs|--ancestral-probs-pipeline|--node-codons|--node-codons-pipeline|--lineage-replacements|--lineage-replacements-pipeline} --yaml-path <string> "
                   "--cluster-ind <int> --hmm-param-dir <string> [--seed <int>] [--num-rates <int>] [--extended-range <0|1>] "
                   "[--devices <a,b,...>] ...\n"
                   "  --marginals: the arguments of --compute-logl; prints the per-site naive-base table and the gene table\n"
                   "  --marginals-pipeline --input-path <RevBayes table> --output-path <prefix> [--burnin-frac <f>]: writes\n"
                   "    <prefix>.sites.tsv, <prefix>.genes.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --naive-probs: the arguments of --compute-logl and --candidates-path <file>; prints the exact posterior\n"
                   "    probability of every candidate naive sequence for that tree\n"
                   "  --naive-probs-pipeline --input-path <RevBayes table> --output-path <prefix> [--burnin-frac <f>]\n"
                   "    [--candidates-path <file>] [--max-candidates <n>]: writes <prefix>.naive.tsv, <prefix>.aa.fasta,\n"
                   "    <prefix>.dnamap and <prefix>.summary.tsv (one device)\n"
                   "  --viterbi: the arguments of --compute-logl; prints the most probable annotation of that tree, the log joint\n"
                   "    probability of its state path, that path's log posterior and the tree's log-likelihood\n"
                   "  --annotations-pipeline --input-path <RevBayes table> --output-path <prefix> [--burnin-frac <f>]\n"
                   "    [--max-candidates <n>]: exact posterior probabilities of annotations; writes <prefix>.annotations.tsv,\n"
                   "    <prefix>.best.tsv, <prefix>.rows.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --codon-marginals [--frame <0|1|2>]: the arguments of --marginals; prints the codon table and the amino-acid\n"
                   "    table of the naive sequence for that tree\n"
                   "  --codon-marginals-pipeline --input-path <RevBayes table> --output-path <prefix> [--burnin-frac <f>]\n"
                   "    [--frame <0|1|2>]: writes <prefix>.codons.tsv, <prefix>.aa.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --events: the arguments of --marginals; prints the exact posteriors of the deletion lengths (column, gene,\n"
                   "    length), of the insertion lengths and of the junction spans for that tree\n"
                   "  --events-pipeline --input-path <RevBayes table> --output-path <prefix> [--burnin-frac <f>]: writes\n"
                   "    <prefix>.deletions.tsv, <prefix>.insertions.tsv, <prefix>.spans.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --ancestral-marginals --seed-seq <name>: the arguments of --marginals; prints, per node on the way from the\n"
                   "    sequence <name> to naive (slot 0 its parent, the last slot the MRCA), the exact per-site table of the node's\n"
                   "    base, then the per-site posterior of the rate category\n"
                   "  --ancestral-marginals-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    [--burnin-frac <f>]: writes <prefix>.parent.tsv, <prefix>.mrca.tsv, <prefix>.rates.tsv, <prefix>.rows.tsv\n"
                   "    and <prefix>.summary.tsv (one device)\n"
                   "  --lineage-substitutions --seed-seq <name>: the arguments of --marginals; prints the edges of the lineage from\n"
                   "    the sequence <name> up to naive (upper node, lower node, branch length, expected number of sites whose two\n"
                   "    ends differ), the per-site expected number of lineage edges on which the site goes from one base to another,\n"
                   "    then per edge the exact joint table of its two ends' bases ([ancestor][descendant]), the naive edge last\n"
                   "  --lineage-substitutions-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    [--burnin-frac <f>]: writes <prefix>.substitutions.tsv, <prefix>.seed_edge.tsv, <prefix>.naive_edge.tsv,\n"
                   "    <prefix>.rows.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --ancestral-probs --seed-seq <name> --node <parent|mrca|mrca-with:NAME[,NAME...]> --candidates <fasta>: the arguments of --marginals;\n"
                   "    prints the exact posterior probability of every candidate sequence at the parent of the sequence <name>\n"
                   "    or at its MRCA with naive (name, sequence, probability, ranked; N leaves a site open);\n"
                   "    --node mrca-with:NAME[,NAME...] selects the most recent common ancestor of <name> and the named sequences of\n"
                   "    the family instead, here and in the three commands below\n"
                   "  --ancestral-probs-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    --node <parent|mrca|mrca-with:NAME[,NAME...]> --candidates <fasta> [--burnin-frac <f>]: writes <prefix>.probs.tsv, <prefix>.rows.tsv\n"
                   "    and <prefix>.summary.tsv (one device)\n"
                   "  --node-codons --seed-seq <name> --node <parent|mrca|mrca-with:NAME[,NAME...]> [--frame <0|1|2>]: the arguments of --marginals; prints\n"
                   "    the exact codon table of the parent of the sequence <name> or of its MRCA with naive for that tree, its\n"
                   "    amino-acid table, and per codon the probabilities that it is identical to the naive codon, a synonymous\n"
                   "    change of it, a replacement, or undetermined (the naive codon holds an N)\n"
                   "  --node-codons-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    --node <parent|mrca|mrca-with:NAME[,NAME...]> [--frame <0|1|2>] [--burnin-frac <f>]: writes <prefix>.codons.tsv, <prefix>.aa.tsv,\n"
                   "    <prefix>.changes.tsv, <prefix>.rows.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --lineage-replacements --seed-seq <name> [--frame <0|1|2>]: the arguments of --marginals; prints per codon the\n"
                   "    expected number of lineage edges, naive to the sequence <name>, on which its amino acid goes from one residue\n"
                   "    to another, the codon's expected unchanged / synonymous / replacement edges, the same on the edge into the\n"
                   "    sequence alone, and per edge the expected number of codons changing silently and by replacement\n"
                   "  --lineage-replacements-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    [--frame <0|1|2>] [--burnin-frac <f>]: writes <prefix>.replacements.tsv, <prefix>.codon_changes.tsv,\n"
                   "    <prefix>.seed_edge.tsv, <prefix>.rows.tsv and <prefix>.summary.tsv (one device)\n"
                   "  --lineage-pipeline --input-path <--pipeline table> --output-path <prefix> --seed-seq <name> [--seed <int>]:\n"
                   "    the lineage tables of the sequence <name>: <prefix>.fasta, .dnamap, .nodes.tsv, .edges.tsv, .summary.tsv\n"
                   "       linearham --lineage-trees --input-path <--asr trees> --output-path <prefix> --seed-seq <name>\n"
                   "         [--weights-path <file>]\n"
                   "    the same tables from a file --asr wrote (no family, no device); --weights-path: one log-weight per tree\n"
                   "    line (the table's LogWeight column), tree k then counts exp(lw_k - max lw)\n"
                   "  --weighted-lineage-pipeline --input-path <RevBayes table> --output-path <prefix> --seed-seq <name>\n"
                   "    [--burnin-frac <f>] [--draws-per-row <1..64>] [--seed <int>]: the importance-weighted lineage tables in\n"
                   "    one pass (one device): rows after the burn-in weighted by exp(LHLogLikelihood - Likelihood), per row the\n"
                   "    naive sequence --pipeline --seed <int> prints and <draws-per-row> ancestral draws; writes the five lineage\n"
                   "    files (counts are weighted sums; the summary gains rows_used, rows_skipped_nonfinite, draws_per_row,\n"
                   "    kish_ess) and <prefix>.rows.tsv\n";
      return argc < 2 ? EXIT_FAILURE : EXIT_SUCCESS;
    }
    const auto t_main = std::chrono::steady_clock::now();
    const bool timing = linearham::host_options().pipeline_timing;
    auto since_start = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main).count(); };
    const std::string subcmd = argv[1];
    const Args a = Parse(argc, argv, 2);
    if (subcmd == "--lineage-trees") {
      linearham::TabulateLineageTrees(a.one("input-path"), a.one("seed-seq"), a.one("output-path"), a.opt("weights-path", ""));
      return EXIT_SUCCESS;
    }
    if (subcmd != "--compute-logl" && subcmd != "--sample" && subcmd != "--pipeline" && subcmd != "--asr" &&
        subcmd != "--marginals" && subcmd != "--marginals-pipeline" && subcmd != "--naive-probs" &&
        subcmd != "--naive-probs-pipeline" && subcmd != "--lineage-pipeline" && subcmd != "--weighted-lineage-pipeline" &&
        subcmd != "--viterbi" && subcmd != "--annotations-pipeline" && subcmd != "--codon-marginals" &&
        subcmd != "--codon-marginals-pipeline" && subcmd != "--events" && subcmd != "--events-pipeline" &&
        subcmd != "--ancestral-marginals" && subcmd != "--ancestral-marginals-pipeline" &&
        subcmd != "--lineage-substitutions" && subcmd != "--lineage-substitutions-pipeline" &&
        subcmd != "--ancestral-probs" && subcmd != "--ancestral-probs-pipeline" && subcmd != "--node-codons" &&
        subcmd != "--node-codons-pipeline" && subcmd != "--lineage-replacements" && subcmd != "--lineage-replacements-pipeline")
      throw std::invalid_argument("'" + subcmd + "' is not a valid subcommand.");
    const std::string yaml_path = a.one("yaml-path");
    const int cluster_ind = std::stoi(a.one("cluster-ind"));
    const std::string hmm_param_dir = a.one("hmm-param-dir");
    const int seed = std::stoi(a.opt("seed", "0"));
    const int num_rates = std::stoi(a.opt("num-rates", "1"));
    // not in the reference: --devices a,b,... -- the GPUs --pipeline deals the table's rows to (row i -> device i mod N);
    // every other subcommand evaluates on the first one
    std::vector<int> device_list;
    {
      const std::string devs = a.opt("devices", "");
      std::size_t pos = 0;
      while (!devs.empty() && pos <= devs.size()) {
        const std::size_t comma = std::min(devs.find(',', pos), devs.size());
        device_list.push_back(std::stoi(devs.substr(pos, comma - pos)));
        pos = comma + 1;
      }
      if (device_list.size() > 1 && (subcmd == "--marginals-pipeline" || subcmd == "--naive-probs-pipeline" ||
                                     subcmd == "--weighted-lineage-pipeline" || subcmd == "--annotations-pipeline" ||
                                     subcmd == "--codon-marginals-pipeline" || subcmd == "--events-pipeline" ||
                                     subcmd == "--ancestral-marginals-pipeline" || subcmd == "--lineage-substitutions-pipeline" ||
                                     subcmd == "--ancestral-probs-pipeline" || subcmd == "--node-codons-pipeline" ||
                                     subcmd == "--lineage-replacements-pipeline"))
        throw std::invalid_argument(subcmd + " runs on one device: --devices may list only one");
      if (device_list.size() > 1 && subcmd != "--pipeline")
        std::fprintf(stderr, "linearham: %s evaluates on one device; of --devices only device %d is used\n", subcmd.c_str(),
                     device_list[0]);
    }
    // the HIP runtime and the context of the device the run evaluates on come up on a side thread while the parameter
    // files are read
    const int first_device = device_list.empty() ? -1 : device_list[0];
    std::thread warmup([first_device] {
      if (first_device >= 0 && first_device < lh_device_count()) (void)lh_set_device(first_device);
      (void)lh_warmup();
    });
    struct Join {
      std::thread& t;
      ~Join() {
        if (t.joinable()) t.join();
      }
    } join_warmup{warmup};
    linearham::PhyloHMMPtr phylo_hmm_ptr =
        std::make_shared<linearham::PhyloHMM>(yaml_path, cluster_ind, hmm_param_dir, seed);
    warmup.join();
    if (timing) std::fprintf(stderr, "[main] family object + HIP context ready at %.3f s\n", since_start());
    if (!device_list.empty()) {
      if (subcmd != "--pipeline") device_list.resize(1);
      phylo_hmm_ptr->SetDevices(device_list);
    }
    // not in the reference: finite log-likelihoods where its scaling over/underflows (include/linearham_amd.h)
    if (std::stoi(a.opt("extended-range", "0")) != 0) phylo_hmm_ptr->SetExtendedRange(true);
    if (subcmd == "--pipeline") {
      phylo_hmm_ptr->RunPipeline(a.one("input-path"), a.one("output-path"), num_rates);
      if (timing) std::fprintf(stderr, "[main] RunPipeline returned at %.3f s\n", since_start());
      phylo_hmm_ptr.reset();
      if (timing) std::fprintf(stderr, "[main] family released at %.3f s\n", since_start());
      return EXIT_SUCCESS;
    }
    if (subcmd == "--marginals-pipeline") {
      phylo_hmm_ptr->RunMarginalsPipeline(a.one("input-path"), a.one("output-path"), num_rates,
                                          std::stod(a.opt("burnin-frac", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--codon-marginals-pipeline") {
      phylo_hmm_ptr->RunCodonMarginalsPipeline(a.one("input-path"), a.one("output-path"), num_rates,
                                               std::stod(a.opt("burnin-frac", "0")), std::stoi(a.opt("frame", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--events-pipeline") {
      phylo_hmm_ptr->RunEventsPipeline(a.one("input-path"), a.one("output-path"), num_rates, std::stod(a.opt("burnin-frac", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--ancestral-marginals-pipeline") {
      phylo_hmm_ptr->RunAncestralMarginalsPipeline(a.one("input-path"), a.one("seed-seq"), a.one("output-path"), num_rates,
                                                   std::stod(a.opt("burnin-frac", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--lineage-substitutions-pipeline") {
      phylo_hmm_ptr->RunLineageSubstitutionsPipeline(a.one("input-path"), a.one("seed-seq"), a.one("output-path"), num_rates,
                                                     std::stod(a.opt("burnin-frac", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--ancestral-probs-pipeline") {
      phylo_hmm_ptr->RunAncestralProbsPipeline(a.one("input-path"), a.one("seed-seq"), std::string(a.one("node")),
                                               a.one("candidates"), a.one("output-path"), num_rates,
                                               std::stod(a.opt("burnin-frac", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--node-codons-pipeline") {
      phylo_hmm_ptr->RunNodeCodonsPipeline(a.one("input-path"), a.one("seed-seq"), std::string(a.one("node")),
                                           a.one("output-path"), num_rates, std::stod(a.opt("burnin-frac", "0")),
                                           std::stoi(a.opt("frame", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--lineage-replacements-pipeline") {
      phylo_hmm_ptr->RunLineageReplacementsPipeline(a.one("input-path"), a.one("seed-seq"), a.one("output-path"), num_rates,
                                                    std::stod(a.opt("burnin-frac", "0")), std::stoi(a.opt("frame", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--naive-probs-pipeline") {
      phylo_hmm_ptr->RunNaiveProbsPipeline(a.one("input-path"), a.one("output-path"), num_rates,
                                           std::stod(a.opt("burnin-frac", "0")), a.opt("candidates-path", ""),
                                           std::stoi(a.opt("max-candidates", "65536")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--annotations-pipeline") {
      phylo_hmm_ptr->RunAnnotationsPipeline(a.one("input-path"), a.one("output-path"), num_rates,
                                            std::stod(a.opt("burnin-frac", "0")), std::stoi(a.opt("max-candidates", "65536")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--lineage-pipeline") {
      phylo_hmm_ptr->RunLineagePipeline(a.one("input-path"), a.one("seed-seq"), a.one("output-path"),
                                        (uint64_t)std::stoll(a.opt("seed", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--weighted-lineage-pipeline") {
      phylo_hmm_ptr->RunWeightedLineagePipeline(a.one("input-path"), a.one("seed-seq"), a.one("output-path"), num_rates,
                                                std::stod(a.opt("burnin-frac", "0")), std::stoi(a.opt("draws-per-row", "1")),
                                                (uint64_t)std::stoll(a.opt("seed", "0")));
      return EXIT_SUCCESS;
    }
    if (subcmd == "--asr") {
      phylo_hmm_ptr->RunAsr(a.one("input-path"), a.one("output-path"), (uint64_t)std::stoll(a.opt("seed", "0")));
      return EXIT_SUCCESS;
    }
    // --ancestral-probs: the node and the candidate file are refused before anything is evaluated
    linearham::LineageNode probs_node;
    linearham::AncestralProbsTable probs;
    if (subcmd == "--ancestral-probs") {
      probs_node = linearham::ParseLineageNodeText(a.one("node"));
      linearham::NamedCandidates c = linearham::ReadNamedCandidateFile(a.one("candidates"), (int)phylo_hmm_ptr->msa().cols());
      probs.names = std::move(c.names);
      probs.seqs = std::move(c.seqs);
    }
    // --node-codons: the node and the frame are refused before anything is evaluated
    linearham::LineageNode codons_node;
    int codons_frame = 0;
    if (subcmd == "--node-codons") {
      codons_node = linearham::ParseLineageNodeText(a.one("node"));
      codons_frame = std::stoi(a.opt("frame", "0"));
      if (codons_frame < 0 || codons_frame > 2) throw std::invalid_argument("--frame must be 0, 1 or 2");
    }
    // --lineage-replacements: the frame is refused before anything is evaluated
    int replacements_frame = 0;
    if (subcmd == "--lineage-replacements") {
      replacements_frame = std::stoi(a.opt("frame", "0"));
      if (replacements_frame < 0 || replacements_frame > 2) throw std::invalid_argument("--frame must be 0, 1 or 2");
    }
    phylo_hmm_ptr->InitializePhyloParameters(a.one("newick-path"), a.multi("er"), a.multi("pi"),
                                             std::stod(a.opt("alpha", "1.0")), num_rates);
    phylo_hmm_ptr->InitializePhyloEmission();
    if (subcmd == "--compute-logl") {
      std::cout << phylo_hmm_ptr->LogLikelihood() << std::endl;
    } else if (subcmd == "--naive-probs") {
      linearham::NaiveProbsTable t;
      t.seqs = linearham::ReadCandidateFile(a.one("candidates-path"), (int)phylo_hmm_ptr->msa().cols());
      double ll = 0;
      const std::vector<double> lc = phylo_hmm_ptr->CandidatePosterior(t.seqs, &ll, &t.log_prior);
      for (double x : lc) t.prob.push_back(std::exp(x));
      linearham::WriteNaiveTable(std::cout, t, false);
    } else if (subcmd == "--viterbi") {
      double lp = 0, ll = 0;
      const linearham::HMM::RowSampler s = phylo_hmm_ptr->ViterbiAnnotation(&lp, &ll);
      char buf[128];
      std::snprintf(buf, sizeof buf, "%.17g\t%.17g\t%.17g\t", lp, lp - ll, ll);
      std::string line = buf;
      phylo_hmm_ptr->AppendAnnotationColumns(line, s);
      std::cout << "log_path\tlog_path_posterior\tlh_loglik\t" << phylo_hmm_ptr->AnnotationHeader() << "\n" << line << "\n";
    } else if (subcmd == "--codon-marginals") {
      const linearham::PhyloHMM::CodonMarginalsResult m = phylo_hmm_ptr->NaiveCodonMarginals(std::stoi(a.opt("frame", "0")));
      linearham::PhyloHMM::WriteCodonTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteAminoAcidTable(std::cout, m);
    } else if (subcmd == "--events") {
      const linearham::PhyloHMM::EventsResult m = phylo_hmm_ptr->RearrangementEvents();
      linearham::PhyloHMM::WriteDeletionTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteInsertionTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteSpanTable(std::cout, m);
    } else if (subcmd == "--ancestral-marginals") {
      const linearham::PhyloHMM::AncestralMarginalsResult m = phylo_hmm_ptr->AncestralMarginals(a.one("seed-seq"));
      const std::size_t L = (std::size_t)m.n_sites;
      for (std::size_t s = 0; s < m.nodes.size(); ++s) {
        std::cout << "slot\t" << s << "\tnode\t" << m.nodes[s] << "\n";
        linearham::PhyloHMM::WriteNodeTable(std::cout, m.marg.data() + s * L * 4, L);
        std::cout << "\n";
      }
      linearham::PhyloHMM::WriteRateTable(std::cout, m.rate_post.data(), L, m.num_rates);
    } else if (subcmd == "--ancestral-probs") {
      for (double x : phylo_hmm_ptr->AncestralCandidatePosterior(a.one("seed-seq"), probs_node.node, probs.seqs, probs_node.with)
                          .log_cand)
        probs.prob.push_back(std::exp(x));
      linearham::WriteAncestralProbsTable(std::cout, probs);
    } else if (subcmd == "--node-codons") {
      const linearham::PhyloHMM::NodeCodonsResult m = phylo_hmm_ptr->NodeCodonMarginals(a.one("seed-seq"), codons_node.node, codons_frame,
                                                                                               codons_node.with);
      linearham::PhyloHMM::WriteNodeCodonTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteNodeAminoAcidTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteChangeTable(std::cout, m);
    } else if (subcmd == "--lineage-replacements") {
      const linearham::PhyloHMM::LineageReplacementsResult m = phylo_hmm_ptr->LineageReplacements(a.one("seed-seq"), replacements_frame);
      linearham::PhyloHMM::WriteReplacementTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteCodonChangeTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteSeedChangeTable(std::cout, m);
      std::cout << "\nedge\tupper\tlower\texpected_synonymous\texpected_replacement\n";
      const std::size_t P = m.nodes.size();
      for (std::size_t e = 0; e <= P; ++e)
        std::cout << e << '\t' << (e < P ? std::to_string(m.nodes[e]) : std::string("naive")) << '\t'
                  << (e == P ? std::to_string(m.nodes[P - 1]) : e == 0 ? a.one("seed-seq") : std::to_string(m.nodes[e - 1])) << '\t'
                  << linearham::Fmt17(m.edge_load[e][0]) << '\t' << linearham::Fmt17(m.edge_load[e][1]) << '\n';
    } else if (subcmd == "--lineage-substitutions") {
      const linearham::PhyloHMM::LineageSubstitutionsResult m = phylo_hmm_ptr->LineageSubstitutions(a.one("seed-seq"));
      const std::size_t L = (std::size_t)m.n_sites, P = m.nodes.size();
      char buf[96];
      std::cout << "edge\tupper\tlower\tbrlen\texpected_substitutions\n";
      for (std::size_t e = 0; e <= P; ++e) {
        std::snprintf(buf, sizeof buf, "%.17g\t%.17g", m.edges[e].brlen, m.edges[e].load);
        std::cout << e << '\t' << m.edges[e].upper << '\t' << m.edges[e].lower << '\t' << buf << "\n";
      }
      std::cout << "\n";
      linearham::PhyloHMM::WritePairTable(std::cout, m.chain_counts.data(), L, 4, true);
      for (std::size_t s = 0; s < P; ++s) {
        std::cout << "\nedge\t" << s << "\tupper\t" << m.edges[s].upper << "\tlower\t" << m.edges[s].lower << "\n";
        linearham::PhyloHMM::WritePairTable(std::cout, m.edge.data() + s * L * 16, L, 4, false);
      }
      std::cout << "\nedge\t" << P << "\tupper\t" << m.edges[P].upper << "\tlower\t" << m.edges[P].lower << "\n";
      linearham::PhyloHMM::WritePairTable(std::cout, m.naive_edge.data(), L, 5, false);
    } else if (subcmd == "--marginals") {
      const linearham::PhyloHMM::NaiveMarginalsResult m = phylo_hmm_ptr->NaiveMarginals();
      linearham::PhyloHMM::WriteSiteTable(std::cout, m);
      std::cout << "\n";
      linearham::PhyloHMM::WriteGeneTable(std::cout, m);
    } else {
      const int N = std::stoi(a.opt("N", "1"));
      for (int i = 0; i < N; i++) std::cout << phylo_hmm_ptr->SampleNaiveSequence() << std::endl;
    }
    return EXIT_SUCCESS;
  } catch (const std::exception& e) {
    std::cerr << "ERROR: " << e.what() << std::endl;
  }
  return EXIT_FAILURE;
}
