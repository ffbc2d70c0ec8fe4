// Constants, tiny dense containers and sequence helpers of the host side
// (mirrors src/utils.hpp / src/utils.cpp of the reference; Eigen is replaced by Matrix<T>).
#ifndef LINEARHAM_UTILS_
#define LINEARHAM_UTILS_

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "yaml_lite.hpp"

struct lh_family;

namespace linearham {

/// The linearham epsilon (src/utils.hpp:20).
const double EPS = 1e-6;
/// The linearham scale factor for dealing with numeric underflow (src/utils.hpp:22).
const double SCALE_FACTOR = std::pow(2, 256);
/// The linearham scale threshold (src/utils.hpp:24).
const double SCALE_THRESHOLD = 1.0 / SCALE_FACTOR;

/// Row-major dense matrix standing in for Eigen::MatrixXd / Eigen::MatrixXi.
template <typename T>
class Matrix {
 public:
  Matrix() = default;
  Matrix(int rows, int cols, T fill = T()) : rows_(rows), cols_(cols), d_((std::size_t)rows * cols, fill) {}
  void setConstant(int rows, int cols, T v) {
    rows_ = rows;
    cols_ = cols;
    d_.assign((std::size_t)rows * cols, v);
  }
  void setZero(int rows, int cols) { setConstant(rows, cols, T()); }
  int rows() const { return rows_; }
  int cols() const { return cols_; }
  std::size_t size() const { return d_.size(); }
  T& operator()(int r, int c) { return d_[(std::size_t)r * cols_ + c]; }
  const T& operator()(int r, int c) const { return d_[(std::size_t)r * cols_ + c]; }
  const T* data() const { return d_.data(); }
  T* data() { return d_.data(); }
  const T* row(int r) const { return d_.data() + (std::size_t)r * cols_; }
  T* row(int r) { return d_.data() + (std::size_t)r * cols_; }
  bool operator==(const Matrix& o) const { return rows_ == o.rows_ && cols_ == o.cols_ && d_ == o.d_; }

 private:
  int rows_ = 0, cols_ = 0;
  std::vector<T> d_;
};

typedef Matrix<double> MatrixXd;
typedef Matrix<int> MatrixXi;
typedef std::vector<double> VectorXd;
typedef std::vector<int> VectorXi;

std::pair<std::vector<std::string>, VectorXd> ParseStringProbMap(const yaml_lite::Node& node);
std::string GetAlphabet(const yaml_lite::Node& root);
int GetAlphabetIndex(const std::string& alphabet, char base);
bool MatchGermlineState(const std::string& state_name, const std::string& gname, int* index);
bool MatchNTIState(const std::string& state_name, const std::string& alphabet, char* base);
std::pair<int, int> FindGermlineStartEnd(const yaml_lite::Node& root, const std::string& gname);
VectorXi ConvertSeqToInts(const std::string& seq_str, const std::string& alphabet);
std::string ConvertIntsToSeq(const VectorXi& seq, const std::string& alphabet);
std::string FixGeneName(std::string name);
/// Bytes 0 .. alphabet.size() - 1 -> characters (the device's sequences; a larger byte reads as the last character, N).
std::string DecodeBases(const uint8_t* bytes, std::size_t n, const std::string& alphabet);

/// assert() of the reference is live in its release build (no -DNDEBUG, SConstruct:266); here format
/// violations throw so that a library user gets a message instead of an abort.
inline void Require(bool cond, const std::string& what) {
  if (!cond) throw std::runtime_error("linearham: requirement failed: " + what);
}

/// %.17g: enough digits for a double to read back as the same bits (the numbers of the pipelines' tables)
inline std::string Fmt17(double v) {
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}

/// The environment switches of the host library (test hooks; read once per process).
struct HostOptions {
  bool pipeline_timing = false;  // LH_PIPELINE_TIMING: stage times of RunPipeline / RunASR / main on stderr
  bool host_sampling = false;    // LH_HOST_SAMPLING: HMM::SampleRow on the host even where the device sampler could run
  int host_threads = 0;          // LH_HOST_THREADS=<n>: worker threads per host stage (0: from the affinity mask)
  int pipeline_batch = 0;        // LH_PIPELINE_BATCH=<n>: rows per batch of RunNaiveProbsPipeline (0: 49 152)
  int lineage_batch = 0;         // LH_LINEAGE_BATCH=<n>: rows per batch of RunLineagePipeline (0: 1 024, RunAsr's)
};
const HostOptions& host_options();

/// Wall-clock marks printed to stderr when LH_PIPELINE_TIMING is set (where the host side of a run spends its time).
struct StageTimer {
  bool on;
  double t0;
  static double Now();
  StageTimer();
  void Mark(const char* what);
};

/// Steady-clock readings and the seconds between two of them (the pipelines' stage times).
using SteadyTime = std::chrono::steady_clock::time_point;
inline SteadyTime SteadyNow() { return std::chrono::steady_clock::now(); }
inline double Seconds(SteadyTime a, SteadyTime b) { return std::chrono::duration<double>(b - a).count(); }

/// The running weighted combination of a table's batches.  A batch hands in wsum[j] = sum_i w_i x_ij and
/// st = (max log weight, sum w, sum w^2), its weights taken relative to its own maximum; the running sums are kept
/// relative to the running maximum.  A batch without a finite weight (st[0] not finite) adds nothing.
struct WeightedSums {
  std::vector<double> total;
  double mx = -INFINITY, s1 = 0.0, s2 = 0.0;
  explicit WeightedSums(std::size_t n) : total(n, 0.0) {}
  void Add(const double* wsum, const double* st) {
    if (!std::isfinite(st[0])) return;
    const double nm = std::max(mx, st[0]);
    const double fo = std::isfinite(mx) ? std::exp(mx - nm) : 0.0, fn = std::exp(st[0] - nm);
    for (std::size_t j = 0; j < total.size(); ++j) total[j] = total[j] * fo + wsum[j] * fn;
    s1 = s1 * fo + st[1] * fn;
    s2 = s2 * fo * fo + st[2] * fn * fn;
    mx = nm;
  }
  void Normalise() {  // total -> weighted means (s1 > 0: some row had a finite weight)
    for (double& v : total) v /= s1;
  }
  double KishEss() const { return s1 * s1 / s2; }
};

/// The host side of a device sequence store (lh_draws_* or lh_lineage_*, which share their signatures): ids for the slots
/// of the handle's last batch from their 64-bit hashes, verified by the device against the stored bytes, so that no hash
/// decides alone.  Two sequences that share a hash are told apart by their bytes.
class SeqInterner {
 public:
  using ResolveFn = int (*)(lh_family*, int32_t, const int32_t*, int32_t*, int32_t*);
  using RowsReadFn = int (*)(lh_family*, int32_t, const int32_t*, uint8_t*);
  /// L: bytes per sequence; who: the pipeline's name, for error texts
  SeqInterner(lh_family* family, ResolveFn resolve, RowsReadFn rows_read, int L, std::string who)
      : family_(family), resolve_(resolve), rows_read_(rows_read), L_(L), who_(std::move(who)) {}
  /// ids[x] = the store id of slot x < m of the last batch (hash[x]; -1 where take[x] is 0), in slot order.  Slots that
  /// differ from their id's bytes are read back and interned by their bytes; one more round must then find none.
  /// Returns how many ids are new: the store appended K() - that .. K() - 1.
  int32_t Assign(std::size_t m, const uint64_t* hash, const uint8_t* take, int32_t* ids);
  int32_t K() const { return K_; }
  int64_t collisions() const { return collisions_; }  // slots that went through the second round

 private:
  lh_family* family_;
  ResolveFn resolve_;
  RowsReadFn rows_read_;
  int L_;
  std::string who_;
  std::unordered_map<uint64_t, int32_t> by_hash_;   // hash -> store id of the first sequence seen with it
  std::unordered_map<std::string, int32_t> exact_;  // store ids made by resolving collisions, by their bytes
  int32_t K_ = 0;
  int64_t collisions_ = 0;
};

}  // namespace linearham

#endif  // LINEARHAM_UTILS_
