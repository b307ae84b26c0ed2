// --rescore FILE.jplace: the placements of an existing jplace evaluated again at their own branch lengths under
// this run's tree, alignment and model.  The device call is epa_dev_score_at (Tiny_Tree::place with opt_branches ==
// false, src/tree/Tiny_Tree.cpp:186-204); the chunk loop around it reads the query file like simple_mpi (place.cpp)
// does -- same reader, same premasking -- and picks the sequences the jplace names.  With --rell N the same rows also
// get their RELL bootstrap support (epa_dev_rell_support) among the rows of their placement object; the object's index
// in the input file is its random stream, so the result does not depend on --chunk-size.  --rell-tests makes that one
// call epa_dev_rell_tests: expected likelihood weight and SH p-value from the same replicates; --au adds the AU test's
// p-value from multiscale replicates of the same streams (epa_dev_rell_au, the default scales); --kh adds the p-values of
// the KH, weighted KH and weighted SH tests from the replicates of --rell (epa_dev_rell_kh).  With --posterior the rows get
// their marginal likelihood (epa_dev_marginal_like: only edge_num comes from the row; Gauss-Legendre x Gauss-Laguerre
// rule, exponential pendant prior) and post_prob, its normalisation over the rows of the placement object.  With --edpl the
// rows get exp_dist, the LWR-weighted mean path distance from the row's attachment point to the rows of its object, and
// the object's edpl (epa_dev_edpl on the tree's topology, one call over the whole file once the LWRs are known).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>
#include <unordered_map>

#include "epa_host.hpp"

namespace epa {

Run_Stats rescore(const Tree& tree, const std::string& jplace_file, const std::string& query_file, const MSA_Info& msa_info,
                  const std::string& outdir, const Options& options, const std::string& invocation, int device) {
  using clk = std::chrono::steady_clock;
  // ---- everything that can be refused without a device
  if (tree.mapper())
    throw std::runtime_error{"--rescore: the reference tree is rooted and --preserve-rooting is on: the file's edge numbers "
                             "are the rooted tree's, which cannot be mapped back to the unrooted working tree in this "
                             "version; run with --preserve-rooting off"};
  std::vector<Jplace_PQuery> input = read_jplace(jplace_file);
  const size_t B = tree.num_branches();
  std::vector<double> blen;
  {
    epa_tree_desc d;
    Tree::Tree_Desc_Storage store;
    tree.fill_tree_desc(d, store);
    blen.swap(store.blen);
  }
  std::unordered_map<std::string, size_t> by_name;
  size_t n_rows = 0;
  for (size_t i = 0; i < input.size(); ++i) {
    Jplace_PQuery& pq = input[i];
    const std::string where = jplace_file + ": placement of '" + pq.name + "': ";
    if (!by_name.emplace(pq.name, i).second) throw std::runtime_error{where + "the name occurs in more than one placement object"};
    for (Jplace_Row& r : pq.rows) {
      if (r.edge_num >= B)
        throw std::runtime_error{where + "edge_num " + std::to_string(r.edge_num) + " is not a branch of the reference tree (" +
                                 std::to_string(B) + " branches)"};
      if (!std::isfinite(r.pendant_length) || r.pendant_length < 0.0)
        throw std::runtime_error{where + "pendant_length " + std::to_string(r.pendant_length) + " is negative or not finite"};
      if (!std::isfinite(r.distal_length) || r.distal_length < 0.0)
        throw std::runtime_error{where + "distal_length " + std::to_string(r.distal_length) + " is negative or not finite"};
      if (r.distal_length > blen[r.edge_num]) {
        if (r.distal_length > blen[r.edge_num] + kDistalSlack)
          throw std::runtime_error{where + "distal_length " + std::to_string(r.distal_length) + " lies beyond the length of edge " +
                                   std::to_string(r.edge_num) + " (" + std::to_string(blen[r.edge_num]) + ")"};
        r.distal_length = blen[r.edge_num];
      }
      ++n_rows;
    }
  }

  // the rule of --posterior: attachment uniform on the edge, pendant length exponential with mean mu
  std::vector<double> x_frac, x_logw, p_len, p_logw;
  if (options.posterior) {
    const uint32_t kx = options.posterior_kx, kp = options.posterior_kp;
    x_frac.resize(kx); x_logw.resize(kx); p_len.resize(kp); p_logw.resize(kp);
    if (epa_quadrature_legendre01(kx, x_frac.data(), x_logw.data()) != EPA_OK ||
        epa_quadrature_laguerre(kp, p_len.data(), p_logw.data()) != EPA_OK)
      throw std::runtime_error{"--posterior-nodes: the node counts must be 1 .. 64"};
    double mu = options.prior_mean;
    if (mu == 0.0) {   // default: the mean branch length of the reference tree
      for (const double l : blen) mu += l;
      mu /= (double)B;
    }
    if (!(std::isfinite(mu) && mu > 0.0))
      throw std::runtime_error{"--posterior: the mean branch length of the reference tree is not positive; give --prior-mean"};
    for (double& t : p_len) t *= mu;
    if (p_len[0] < 1e-4)
      std::cerr << "warning: --posterior: the smallest pendant node is " << p_len[0] << " (prior mean " << mu << "): below 1e-4 "
                   "the error of a log-likelihood grows like 1 / pendant and marginal_like is not covered by the 1e-6 bound; "
                   "a larger --prior-mean or fewer pendant nodes (--posterior-nodes) lift it" << std::endl;
  }

  // ---- device
  Run_Stats st;
  st.host_threads = configure_host_threads();
  st.chunk_path = "rescore";
  auto ts = clk::now();
  Device_Evaluator dev(tree, options, device);
  st.ref_tree_logl = dev.ref_tree_logl(0);
  st.seconds_setup = std::chrono::duration<double>(clk::now() - ts).count();
  if (dev.lookup_blocks()) { st.lookup_mode = "blocks"; st.lookup_block = dev.lookup_block(); }
  const auto t_loop = clk::now();

  Sample sample(input.size());
  std::vector<char> seen(input.size(), 0);
  const bool premask = options.premasking && msa_info.gap_count() > 0;
  Fasta_Stream reader(query_file);
  const size_t per_chunk = std::max<size_t>(1, options.chunk_size);
  st.device_chunk = per_chunk;
  size_t skipped = 0;
  for (;;) {
    ts = clk::now();
    MSA chunk;
    if (reader.read_next(chunk, per_chunk) == 0) break;
    st.seconds_read += std::chrono::duration<double>(clk::now() - ts).count();
    // the sequences of this chunk that the jplace names, in file order
    MSA named;
    std::vector<size_t> target;
    for (Sequence& s : chunk) {
      const auto it = by_name.find(s.header());
      if (it == by_name.end() || seen[it->second]) { ++skipped; continue; }
      seen[it->second] = 1;
      target.push_back(it->second);
      named.emplace_back(s.header(), premask ? subset_sequence(s.sequence(), msa_info.gap_mask()) : s.sequence());
    }
    if (named.empty()) continue;
    ts = clk::now();
    const Encoded_Chunk enc = encode_chunk(named, tree, options);
    st.seconds_encode += std::chrono::duration<double>(clk::now() - ts).count();
    std::vector<epa_pair> pairs;
    std::vector<double> pendant, distal;
    for (size_t q = 0; q < named.size(); ++q)
      for (const Jplace_Row& r : input[target[q]].rows) {
        pairs.push_back(epa_pair{r.edge_num, (uint32_t)q});
        pendant.push_back(r.pendant_length);
        distal.push_back(r.distal_length);
      }
    std::vector<double> lnl(pairs.size());
    ts = clk::now();
    epa_dev_set_query_layout(dev.ctx(), enc.stride);
    epa_dev_set_query_packing(dev.ctx(), enc.bits);
    auto check = [&](int rc) {
      if (rc != EPA_OK)
        throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
    };
    // the calls on the rows at their own lengths begin with the same ten arguments; `rest` is what follows them
    auto rows = [&](auto fn, auto... rest) {
      check(fn(dev.ctx(), pairs.data(), pendant.data(), distal.data(), nullptr, pairs.size(), enc.codes.data(),
               enc.win_begin.data(), enc.win_span.data(), (uint32_t)named.size(), rest...));
    };
    rows(epa_dev_score_at, lnl.data());
    std::vector<double> support, elw, p_sh, p_au, p_kh, p_wkh, p_wsh;
    if (options.rell_replicates) {
      const std::vector<uint64_t> stream_id(target.begin(), target.end());
      const uint32_t R = options.rell_replicates;
      const uint64_t seed = options.rell_seed;
      support.resize(pairs.size());
      if (options.rell_tests) { elw.resize(pairs.size()); p_sh.resize(pairs.size()); }
      if (options.rell_tests) rows(epa_dev_rell_tests, stream_id.data(), R, seed, support.data(), elw.data(), p_sh.data());
      else rows(epa_dev_rell_support, stream_id.data(), R, seed, support.data());
      if (options.au) {
        p_au.resize(pairs.size());
        rows(epa_dev_rell_au, stream_id.data(), R, seed, nullptr, 0, p_au.data(), nullptr, nullptr);
      }
      if (options.kh) {
        p_kh.resize(pairs.size()); p_wkh.resize(pairs.size()); p_wsh.resize(pairs.size());
        rows(epa_dev_rell_kh, stream_id.data(), R, seed, p_kh.data(), p_wkh.data(), p_wsh.data());
      }
    }
    std::vector<double> marginal;
    if (options.posterior) {
      marginal.resize(pairs.size());
      check(epa_dev_marginal_like(dev.ctx(), pairs.data(), pairs.size(), x_frac.data(), x_logw.data(), (uint32_t)x_frac.size(),
                                  p_len.data(), p_logw.data(), (uint32_t)p_len.size(), enc.codes.data(), enc.win_begin.data(),
                                  enc.win_span.data(), (uint32_t)named.size(), marginal.data(), nullptr));
    }
    st.seconds_place += std::chrono::duration<double>(clk::now() - ts).count();
    size_t k = 0;
    for (size_t q = 0; q < named.size(); ++q) {
      PQuery pq(target[q], named[q].header());
      for (const Jplace_Row& r : input[target[q]].rows) {
        pq.emplace_back(r.edge_num, lnl[k], r.pendant_length, r.distal_length);
        if (!support.empty()) pq[pq.size() - 1].rell_support(support[k]);
        if (!elw.empty()) { pq[pq.size() - 1].elw(elw[k]); pq[pq.size() - 1].p_sh(p_sh[k]); }
        if (!p_au.empty()) pq[pq.size() - 1].p_au(p_au[k]);
        if (!p_kh.empty()) { pq[pq.size() - 1].p_kh(p_kh[k]); pq[pq.size() - 1].p_wkh(p_wkh[k]); pq[pq.size() - 1].p_wsh(p_wsh[k]); }
        if (!marginal.empty()) pq[pq.size() - 1].marginal_like(marginal[k]);
        ++k;
      }
      sample[target[q]] = std::move(pq);
    }
    st.queries += named.size();
    st.pairs += pairs.size();
  }
  for (size_t i = 0; i < input.size(); ++i)
    if (!seen[i])
      throw std::runtime_error{"--rescore: sequence '" + input[i].name + "' of " + jplace_file + " does not occur in " + query_file};
  std::cout << "Rescored " << n_rows << " placements of " << st.queries << " sequences; " << skipped
            << " sequences of the query file are not named in " << jplace_file << " and were skipped." << std::endl;

  ts = clk::now();
  compute_and_set_lwr(sample);
  if (options.posterior)   // post_prob: the arithmetic of compute_and_set_lwr on marginal_like
    for (PQuery& pq : sample) {
      double mx = -std::numeric_limits<double>::infinity(), total = 0.0;
      for (const Placement& p : pq) mx = std::max(mx, p.marginal_like());
      for (Placement& p : pq) { const double e = std::exp(p.marginal_like() - mx); p.post_prob(e); total += e; }
      for (Placement& p : pq) p.post_prob(p.post_prob() / total);
    }
  for (PQuery& pq : sample) sort_by_lwr(pq);
  if (options.edpl) {
    // EDPL (epa_dev_edpl): ONE call over all rows, as the file will list them -- the object's index is the query, the
    // recomputed like_weight_ratios are the weights, entry order is the LWR-sorted order of the output
    dev.set_topology(tree);
    std::vector<epa_pair> pairs;
    std::vector<double> distal, weight;
    pairs.reserve(n_rows); distal.reserve(n_rows); weight.reserve(n_rows);
    for (size_t i = 0; i < sample.size(); ++i)
      for (const Placement& p : sample[i]) {
        pairs.push_back(epa_pair{(uint32_t)p.branch_id(), (uint32_t)i});
        distal.push_back(p.distal_length());
        weight.push_back(p.lwr());
      }
    std::vector<double> row_dist(pairs.size()), edpl(sample.size());
    const int rc = epa_dev_edpl(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)sample.size(),
                                row_dist.data(), edpl.data());
    if (rc != EPA_OK)
      throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
    size_t k = 0;
    for (size_t i = 0; i < sample.size(); ++i)
      for (Placement& p : sample[i]) { p.exp_dist(row_dist[k++]); p.edpl(edpl[i]); }
  }
  st.seconds_post = std::chrono::duration<double>(clk::now() - ts).count();
  ts = clk::now();
  std::string dir = outdir;
  if (!dir.empty() && dir.back() != '/') dir += "/";
  const std::string out_path = dir + "epa_result.jplace";
  std::ofstream os(out_path);
  if (!os) throw std::runtime_error{"cannot open " + out_path};
  write_jplace(os, std::vector<Sample>{sample}, tree.numbered_newick(options.precision), invocation, options.precision, nullptr,
               (options.rell_replicates ? kJplaceRell : 0u) | (options.rell_tests ? kJplaceRellTests : 0u) |
                   (options.au ? kJplaceAu : 0u) | (options.kh ? kJplaceKh : 0u) |
                   (options.posterior ? kJplacePosterior : 0u) | (options.edpl ? kJplaceEdpl : 0u));
  os.flush();
  if (!os) { os.close(); std::remove(out_path.c_str()); throw std::runtime_error{"writing " + out_path + " failed"}; }
  st.seconds_write = std::chrono::duration<double>(clk::now() - ts).count();
  st.seconds_loop = std::chrono::duration<double>(clk::now() - t_loop).count();
  return st;
}

}  // namespace epa
