// similarity_glue.cpp -- Rcpp glue that replaces the BODIES of the reference's
// src/minHash.cpp (similarityMH, :119-188) and src/pairwiseSeqAlign.cpp
// (similarityNW, :331-365) with calls into libdynaalign_hip.so (include/dynaalign.h).
//
// Drop-in recipe: delete those two files from the reference's src/, add this
// file and the Makevars next to it and re-run Rcpp::compileAttributes().  The two exported
// signatures the reference already has (similarityMH, similarityNW) are kept verbatim, so their
// generated shims come out byte-identical; the two ADDED exports (similarityMH_edges,
// similarityNW_edges) get new shims in src/RcppExports.cpp + R/RcppExports.R and need
// `export(similarityMH_edges)` / `export(similarityNW_edges)` in NAMESPACE (roxygen writes them
// from the @export tags below); likewise the two-set exports similarityMH_cross / similarityNW_cross.
// Without compileAttributes() only the two original functions are callable.
//
// NOT compiled in the build container (R and Rcpp are absent there); it is the binding a
// maintainer adds.  Everything it calls is exercised through the same C ABI by
// dynaalign_amd/similarity.py and the test-suite.
#include <Rcpp.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "dynaalign.h"

using namespace Rcpp;

namespace {

// One pass over the STRSXP on the calling (main R) thread: bytes of every element back
// to back + offsets.  (The reference copies each element per use -- src/minHash.cpp:147 --
// from OpenMP worker threads, and src/pairwiseSeqAlign.cpp:341-343 once per pair.)
struct Packed {
  std::vector<uint8_t> residues;
  std::vector<int64_t> offsets;
  explicit Packed(const CharacterVector &x) : offsets(x.length() + 1, 0) {
    const R_xlen_t n = x.length();
    size_t total = 0;
    for (R_xlen_t i = 0; i < n; ++i) total += std::string(as<std::string>(x[i])).size();
    residues.reserve(total ? total : 1);
    for (R_xlen_t i = 0; i < n; ++i) {
      const std::string s = as<std::string>(x[i]);  // same conversion the reference uses
      residues.insert(residues.end(), s.begin(), s.end());
      offsets[i + 1] = (int64_t)residues.size();
    }
    if (residues.empty()) residues.push_back(0);
  }
};

void check(int rc) {
  if (rc != DA_OK) Rcpp::stop("%s", da_last_error());  // reference message texts come from the library
}

void set_dimnames(NumericMatrix &m) {  // src/minHash.cpp:181-185, src/pairwiseSeqAlign.cpp:356-362
  const R_xlen_t n = m.nrow();
  CharacterVector labels(n);
  for (R_xlen_t i = 0; i < n; ++i) labels[i] = std::to_string(i + 1);
  m.attr("dimnames") = List::create(labels, labels);
}

void set_dimnames_rect(NumericMatrix &m) {  // the two-set calls: rows "1".."m", columns "1".."n"
  CharacterVector rows(m.nrow()), cols(m.ncol());
  for (R_xlen_t i = 0; i < m.nrow(); ++i) rows[i] = std::to_string(i + 1);
  for (R_xlen_t j = 0; j < m.ncol(); ++j) cols[j] = std::to_string(j + 1);
  m.attr("dimnames") = List::create(rows, cols);
}

// Seed for HashFamily: the reference draws std::random_device{}() (src/minHash.cpp:73) and
// gives no way to fix it.  options(DynaAlign.seed = <int>) or DYNAALIGN_SEED=<int> make a
// run reproducible without touching the R-level signature.
uint32_t hash_seed() {
  Environment base = Environment::base_env();
  Function getOption = base["getOption"];
  SEXP opt = getOption("DynaAlign.seed");
  if (!Rf_isNull(opt)) {
    // reduce modulo 2^32 through a 64-bit integer: a direct double -> uint32_t cast of a negative or
    // > 2^32 value is undefined behaviour
    const double d = std::floor(as<double>(opt));
    if (!(std::fabs(d) < 9.0e15)) Rcpp::stop("options(DynaAlign.seed) must be a finite integer");
    return (uint32_t)((uint64_t)(int64_t)d & 0xffffffffu);
  }
  if (const char *e = std::getenv("DYNAALIGN_SEED")) return (uint32_t)(std::strtoull(e, nullptr, 10) & 0xffffffffu);
  return da_random_seed();
}

// options(DynaAlign.devices = c(0L, 1L, ...)) -- HIP device ordinals this ONE R process drives (a host thread per
// device inside the library) -- and options(DynaAlign.exchange = "rows" | "allgather" | "peercopy").  Unset: the
// current device, exactly as before.  DYNAALIGN_DEVICES=0,1,.. is the environment form.
struct DeviceOpts {
  std::vector<int32_t> devices;
  da_opts opts;
  bool set = false;
  DeviceOpts() {
    Environment base = Environment::base_env();
    Function getOption = base["getOption"];
    SEXP dv = getOption("DynaAlign.devices");
    if (!Rf_isNull(dv)) {
      IntegerVector v = as<IntegerVector>(dv);
      devices.assign(v.begin(), v.end());
      set = true;
    } else if (const char *e = std::getenv("DYNAALIGN_DEVICES")) {
      for (const char *p = e; *p;) {
        char *end = nullptr;
        const long d = std::strtol(p, &end, 10);
        if (end == p) break;
        devices.push_back((int32_t)d);
        p = (*end == ',') ? end + 1 : end;
      }
      set = !devices.empty();
    }
    int exchange = DA_EXCHANGE_ROWS;
    SEXP ex = getOption("DynaAlign.exchange");
    if (!Rf_isNull(ex)) {
      const std::string x = as<std::string>(ex);
      if (x == "rows") exchange = DA_EXCHANGE_ROWS;
      else if (x == "allgather") exchange = DA_EXCHANGE_ALLGATHER;
      else if (x == "peercopy") exchange = DA_EXCHANGE_PEERCOPY;
      else Rcpp::stop("options(DynaAlign.exchange) must be \"rows\", \"allgather\" or \"peercopy\"");
    }
    opts.struct_size = (uint32_t)sizeof(da_opts);
    opts.n_devices = (int32_t)devices.size();
    opts.devices = devices.empty() ? nullptr : devices.data();
    opts.exchange = exchange;
    opts.reserved = 0;
    opts.phase_ms = nullptr;
  }
  const da_opts *get() const { return set ? &opts : nullptr; }   // NULL = da_similarity_mh / _nw on the current device
};

// dim(v) <- c(rows, cols): an integer vector becomes R's integer matrix.  (A vector type without attr() -- the test-only Rcpp stand-in
// this file is also compiled against -- takes the overload below and stays a plain column-major vector.)
template <typename V>
auto set_dim(V &v, int rows, int cols, int) -> decltype(v.attr("dim"), void()) {
  IntegerVector d(2);
  d[0] = rows;
  d[1] = cols;
  v.attr("dim") = d;
}
template <typename V>
void set_dim(V &, int, int, long) {}

// the C ABI's row-major [m][top] results as R's list(index = m x top integer matrix, 1-based; similarity = m x top numeric matrix)
List topk_result(const std::vector<int32_t> &idx, const std::vector<double> &val, int64_t m, int top) {
  IntegerVector index(m * top);
  NumericMatrix similarity(m, top);
  for (int64_t i = 0; i < m; ++i)
    for (int t = 0; t < top; ++t) {
      index[i + (int64_t)t * m] = idx[(size_t)(i * top + t)] + 1;   // column-major, R is 1-based
      REAL(similarity)[i + (int64_t)t * m] = val[(size_t)(i * top + t)];
    }
  set_dim(index, (int)m, top, 0);
  return List::create(_["index"] = index, _["similarity"] = similarity);
}

struct EdgesHandle {   // da_edges_free on scope exit
  da_edges *h;
  explicit EdgesHandle(da_edges *p) : h(p) {}
  ~EdgesHandle() { da_edges_free(h); }
  EdgesHandle(const EdgesHandle &) = delete;
  EdgesHandle &operator=(const EdgesHandle &) = delete;
};

}  // namespace

//' @name similarityMH
//' @title Compute MinHash Similarity Matrix
//' @param sequences A character vector of input sequences
//' @param k The length of k-mers to use (default: 4)
//' @param n_hash Number of hash functions to use (default: 50)
//' @return A numeric matrix of pairwise similarities
//' @export
// [[Rcpp::export]]
NumericMatrix similarityMH(CharacterVector sequences, int k = 4, int n_hash = 50) {
  const Packed in(sequences);
  const int64_t n = sequences.length();
  // validation order and messages (src/minHash.cpp:121-131) are enforced by the library;
  // call it first with no output so that errors surface before the n*n allocation
  std::vector<uint32_t> seeds(n_hash > 0 ? n_hash : 1);
  if (n_hash > 0) check(da_hash_family_seeds(hash_seed(), n_hash, seeds.data()));
  if (n <= 0 || k <= 0 || n_hash <= 0) {
    check(da_similarity_mh(in.residues.data(), in.offsets.data(), n, k, n_hash, seeds.data(), nullptr));   // always an error here
  }
  NumericMatrix out(n, n);  // column-major; the result is symmetric, so layout does not matter
  const DeviceOpts dev;
  check(da_similarity_mh_opts(in.residues.data(), in.offsets.data(), n, k, n_hash, seeds.data(), REAL(out), dev.get()));
  set_dimnames(out);
  return out;
}

//' @name similarityNW
//' @title Sequence Alignment using Needleman-Wunsch Algorithm
//' @param sequences A character vector of input sequences
//' @param matrixName A substitution matrix for scoring alignments
//' @param gapOpen penalty for opening a gap
//' @param gapExt penalty for extending a gap
//' @return A numeric matrix of pairwise similarities
//' @export
// [[Rcpp::export]]
NumericMatrix similarityNW(CharacterVector sequences, std::string matrixName = "BLOSUM62",
                           int gapOpen = 10, int gapExt = 4) {
  const Packed in(sequences);
  const int64_t n = sequences.length();
  NumericMatrix out(n, n);
  const DeviceOpts dev;
  check(da_similarity_nw_opts(in.residues.data(), in.offsets.data(), n, matrixName.c_str(), gapOpen, gapExt,
                              n > 0 ? REAL(out) : nullptr, dev.get()));
  set_dimnames(out);
  return out;
}

//' @name similarityMH_edges
//' @title MinHash similarity + clusterbreak's quantile threshold, as an edge list
//' @description Non-breaking addition.  Equivalent to
//'   S <- similarityMH(sequences, k, n_hash); thr <- quantile(S[upper.tri(S)], thresh_p); S[S < thr] <- 0
//' (R/clusterbreak.R:217-221) but returns only the surviving upper-triangle entries, so a 100k-peptide set
//' never materialises its 80 GB matrix:  igraph::graph_from_data_frame(res$edges, directed = FALSE).
//' @export
// [[Rcpp::export]]
List similarityMH_edges(CharacterVector sequences, int k = 4, int n_hash = 50, double thresh_p = 0.8) {
  const Packed in(sequences);
  const int64_t n = sequences.length();
  std::vector<uint32_t> seeds(n_hash > 0 ? n_hash : 1);
  if (n_hash > 0) check(da_hash_family_seeds(hash_seed(), n_hash, seeds.data()));
  double thr = 0;
  int64_t m = 0;
  da_edges *h = nullptr;                  // one pass: the pipeline runs once, the edges wait in the handle
  check(da_similarity_mh_edges_begin(in.residues.data(), in.offsets.data(), n, k, n_hash, seeds.data(), thresh_p, &h, &thr, &m));
  const EdgesHandle guard(h);             // released even if the allocations below throw
  IntegerVector from(m), to(m);
  NumericVector weight(m);
  check(da_edges_fetch(h, m, INTEGER(from), INTEGER(to), REAL(weight)));
  for (int64_t e = 0; e < m; ++e) { from[e] += 1; to[e] += 1; }   // R is 1-based
  return List::create(_["threshold"] = thr,
                      _["edges"] = DataFrame::create(_["from"] = from, _["to"] = to, _["weight"] = weight));
}

//' @name similarityNW_edges
//' @title Needleman-Wunsch identity + clusterbreak's quantile threshold, as an edge list
//' @description The similarityNW counterpart of similarityMH_edges (sequences up to 127 residues, none empty).
//' @export
// [[Rcpp::export]]
List similarityNW_edges(CharacterVector sequences, std::string matrixName = "BLOSUM62", int gapOpen = 10,
                        int gapExt = 4, double thresh_p = 0.8) {
  const Packed in(sequences);
  const int64_t n = sequences.length();
  double thr = 0;
  int64_t m = 0;
  da_edges *h = nullptr;
  check(da_similarity_nw_edges_begin(in.residues.data(), in.offsets.data(), n, matrixName.c_str(), gapOpen, gapExt, thresh_p,
                                     &h, &thr, &m));
  const EdgesHandle guard(h);
  IntegerVector from(m), to(m);
  NumericVector weight(m);
  check(da_edges_fetch(h, m, INTEGER(from), INTEGER(to), REAL(weight)));
  for (int64_t e = 0; e < m; ++e) { from[e] += 1; to[e] += 1; }   // R is 1-based
  return List::create(_["threshold"] = thr,
                      _["edges"] = DataFrame::create(_["from"] = from, _["to"] = to, _["weight"] = weight));
}

//' @name similarityMH_cross
//' @title MinHash similarity of every sequence of x against every sequence of y
//' @description Non-breaking addition: the length(x) by length(y) matrix whose element (i, j) is the share of hash functions on which the
//' signatures of x[i] and y[j] agree -- the block [seq_along(x), length(x) + seq_along(y)] of similarityMH(c(x, y), k, n_hash) under the
//' same seeds.  No forced diagonal.
//' @export
// [[Rcpp::export]]
NumericMatrix similarityMH_cross(CharacterVector x, CharacterVector y, int k = 4, int n_hash = 50) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  std::vector<uint32_t> seeds(n_hash > 0 ? n_hash : 1);
  if (n_hash > 0) check(da_hash_family_seeds(hash_seed(), n_hash, seeds.data()));
  if (m <= 0 || n <= 0 || k <= 0 || n_hash <= 0)   // always an error here: raised before the m * n allocation
    check(da_similarity_mh_cross(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, k, n_hash, seeds.data(),
                                 nullptr, 1));
  NumericMatrix out(m, n);   // column-major: column_major = 1 fills it in place
  check(da_similarity_mh_cross(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, k, n_hash, seeds.data(),
                               REAL(out), 1));
  set_dimnames_rect(out);
  return out;
}

//' @name similarityNW_cross
//' @title Needleman-Wunsch identity of every sequence of x against every sequence of y
//' @description Non-breaking addition: element (i, j) is the identity of the alignment of x[i] (sequence1) with y[j] -- the block
//' [seq_along(x), length(x) + seq_along(y)] of similarityNW(c(x, y), ...).
//' @export
// [[Rcpp::export]]
NumericMatrix similarityNW_cross(CharacterVector x, CharacterVector y, std::string matrixName = "BLOSUM62", int gapOpen = 10,
                                 int gapExt = 4) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  NumericMatrix out(m, n);
  check(da_similarity_nw_cross(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, matrixName.c_str(), gapOpen,
                               gapExt, (m > 0 && n > 0) ? REAL(out) : nullptr, 1));
  set_dimnames_rect(out);
  return out;
}

//' @name similarityMH_cross_topk
//' @title For every sequence of x its top most similar sequences of y (MinHash), without the length(x) by length(y) matrix
//' @description Non-breaking addition.  With R <- similarityMH_cross(x, y, k, n_hash) under the same seeds, row i of index is
//' order(-R[i, ], seq_along(y))[1:top] -- similarity descending, position ascending among equals, zeros filling a row with fewer than top
//' positive entries -- and similarity[i, t] is R[i, index[i, t]].  top is clamped to length(y) and may be at most 1024.
//' @return list(index = integer matrix, similarity = numeric matrix), both length(x) by top
//' @export
// [[Rcpp::export]]
List similarityMH_cross_topk(CharacterVector x, CharacterVector y, int k = 4, int n_hash = 50, int top = 10) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  std::vector<uint32_t> seeds(n_hash > 0 ? n_hash : 1);
  if (n_hash > 0) check(da_hash_family_seeds(hash_seed(), n_hash, seeds.data()));
  if (n > 0 && top > n) top = (int)n;
  const size_t cnt = (size_t)(m > 0 ? m : 1) * (size_t)(top > 0 ? top : 1);
  std::vector<int32_t> idx(cnt);
  std::vector<double> val(cnt);
  check(da_similarity_mh_cross_topk(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, k, n_hash, seeds.data(),
                                    top, idx.data(), val.data()));
  return topk_result(idx, val, m, top);
}

//' @name similarityNW_cross_topk
//' @title For every sequence of x its top most similar sequences of y (Needleman-Wunsch identity, x[i] as sequence1)
//' @description Non-breaking addition, as similarityMH_cross_topk on similarityNW_cross(x, y, ...).  Equal similarities tie whatever their
//' (matches, length) -- 2/4 and 3/6 -- and are listed by position.  Sequences of 1 to 127 residues.
//' @return list(index = integer matrix, similarity = numeric matrix), both length(x) by top
//' @export
// [[Rcpp::export]]
List similarityNW_cross_topk(CharacterVector x, CharacterVector y, std::string matrixName = "BLOSUM62", int gapOpen = 10, int gapExt = 4,
                             int top = 10) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  if (n > 0 && top > n) top = (int)n;
  const size_t cnt = (size_t)(m > 0 ? m : 1) * (size_t)(top > 0 ? top : 1);
  std::vector<int32_t> idx(cnt);
  std::vector<double> val(cnt);
  check(da_similarity_nw_cross_topk(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, matrixName.c_str(),
                                    gapOpen, gapExt, top, idx.data(), val.data()));
  return topk_result(idx, val, m, top > 0 ? top : 0);
}

namespace {
// the handle of a *_cross_edges_begin call as list(threshold, i, j, weight), positions 1-based
List cross_edges_result(da_edges *h, double thr, int64_t cnt) {
  const EdgesHandle guard(h);             // released even if the allocations below throw
  IntegerVector i(cnt), j(cnt);
  NumericVector weight(cnt);
  check(da_edges_fetch(h, cnt, INTEGER(i), INTEGER(j), REAL(weight)));
  for (int64_t e = 0; e < cnt; ++e) { i[e] += 1; j[e] += 1; }   // R is 1-based
  return List::create(_["threshold"] = thr, _["i"] = i, _["j"] = j, _["weight"] = weight);
}
}  // namespace

//' @name similarityMH_cross_edges
//' @title The entries of similarityMH_cross(x, y, k, n_hash) that pass a threshold, as a sorted edge list
//' @description Non-breaking addition.  With R <- similarityMH_cross(x, y, k, n_hash) under the same seeds: every (i, j) with
//' R[i, j] >= threshold and R[i, j] > 0, sorted by (i, j), weight = R[i, j]; the length(x) by length(y) matrix is never built.  The threshold is
//' quantile(as.vector(R), thresh_p), or, with absolute = TRUE, thresh_p itself (a range query: every y within that similarity of each x).
//' @return list(threshold, i, j, weight), i and j 1-based
//' @export
// [[Rcpp::export]]
List similarityMH_cross_edges(CharacterVector x, CharacterVector y, int k = 4, int n_hash = 50, double thresh_p = 0.8,
                              bool absolute = false) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  std::vector<uint32_t> seeds(n_hash > 0 ? n_hash : 1);
  if (n_hash > 0) check(da_hash_family_seeds(hash_seed(), n_hash, seeds.data()));
  double thr = 0;
  int64_t cnt = 0;
  da_edges *h = nullptr;
  check(da_similarity_mh_cross_edges_begin(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, k, n_hash,
                                           seeds.data(), thresh_p, absolute ? 0 : 1, &h, &thr, &cnt));
  return cross_edges_result(h, thr, cnt);
}

//' @name similarityNW_cross_edges
//' @title The entries of similarityNW_cross(x, y, ...) that pass a threshold, as a sorted edge list
//' @description Non-breaking addition, as similarityMH_cross_edges on similarityNW_cross(x, y, ...) (x[i] is sequence1).  Sequences of 1 to 127
//' residues.
//' @return list(threshold, i, j, weight), i and j 1-based
//' @export
// [[Rcpp::export]]
List similarityNW_cross_edges(CharacterVector x, CharacterVector y, std::string matrixName = "BLOSUM62", int gapOpen = 10, int gapExt = 4,
                              double thresh_p = 0.8, bool absolute = false) {
  const Packed px(x), py(y);
  const int64_t m = x.length(), n = y.length();
  double thr = 0;
  int64_t cnt = 0;
  da_edges *h = nullptr;
  check(da_similarity_nw_cross_edges_begin(px.residues.data(), px.offsets.data(), m, py.residues.data(), py.offsets.data(), n, matrixName.c_str(),
                                           gapOpen, gapExt, thresh_p, absolute ? 0 : 1, &h, &thr, &cnt));
  return cross_edges_result(h, thr, cnt);
}
