// --dedup: identical reads of a chunk are placed once.  Amplicon and metabarcoding inputs hold each distinct read many
// times; epa_dev_place_chunk_dedup (include/epa_dev.h, "Duplicate queries") finds the classes of identical queries on the
// device, places one representative per class and hands back rep / first.  This loop writes ONE placement object per
// class, in order of first appearance, whose "n" lists every name of the class in file order (jplace allows several names
// per object).  Classes are per chunk: equal reads in different chunks stay separate objects.  The loop is synchronous
// and uses one device; LWR, filter and jplace text are the host stages of the plain run (place.cpp, io.cpp).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "epa_host.hpp"

namespace epa {

Run_Stats place_dedup_file(const Tree& tree, const std::string& query_file, const MSA_Info& msa_info, const std::string& outdir,
                           const Options& options, const std::string& invocation, int device) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
  if (!options.prescoring) throw std::runtime_error{"--dedup runs the fused chunk body: --no-heur is not supported with it"};
  const bool premask = options.premasking && msa_info.gap_count() > 0;
  const size_t nb = tree.num_branches();
  Run_Stats st;
  st.host_threads = configure_host_threads();
  st.chunk_path = "dedup";
  st.dedup = true;
  auto ts = clk::now();
  Device_Evaluator dev(tree, options, device);
  st.ref_tree_logl = dev.ref_tree_logl(0);
  st.seconds_setup = since(ts);
  if (dev.lookup_blocks()) {
    st.lookup_mode = "blocks";
    st.lookup_block = dev.lookup_block();
  }
  const auto t_loop = clk::now();
  auto fail_dev = [&](int rc) {
    throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
  };
  const int mode = options.baseball ? EPA_HEUR_BASEBALL : options.prescoring_by_percentage ? EPA_HEUR_FIXED : EPA_HEUR_DYNAMIC;
  if (epa_dev_set_heuristic(dev.ctx(), mode, mode == EPA_HEUR_FIXED ? options.prescoring_threshold : 0.0) != EPA_OK)
    throw std::runtime_error{epa_dev_last_error(dev.ctx())};

  // one chunk at a time on the direct entry point: one preplacement table (and one block buffer) on the device
  size_t per_chunk = std::max<size_t>(1, options.chunk_size);
  {
    uint64_t fr = 0, tot = 0;
    if (epa_dev_mem_info(dev.ctx(), &fr, &tot) == EPA_OK)
      per_chunk = device_chunk_reads(fr, nb, 1, per_chunk, options.chunk_size_given ? options.chunk_size : 0, dev.bank_bytes());
  }
  st.device_chunk = per_chunk;
  Fasta_Stream reader(query_file);
  std::vector<std::string> texts;
  std::vector<epa_pair>& pairs = dev.pair_buffer();
  std::vector<epa_result>& res = dev.result_buffer();
  std::vector<uint32_t> rep, first;
  size_t offset = 0;
  for (;;) {
    ts = clk::now();
    MSA chunk;
    if (reader.read_next(chunk, per_chunk) == 0) break;
    if (premask) chunk = subset_msa(chunk, msa_info.gap_mask());
    const size_t Q = chunk.size();
    st.seconds_read += since(ts);
    ts = clk::now();
    const Encoded_Chunk enc = encode_chunk(chunk, tree, options);
    st.seconds_encode += since(ts);

    ts = clk::now();
    uint64_t cap = std::max<uint64_t>((uint64_t)Q * 8, pairs.size()), n = 0;
    if (mode == EPA_HEUR_FIXED)
      cap = std::max<uint64_t>(cap, (uint64_t)Q * std::min<size_t>(nb, (size_t)std::ceil(options.prescoring_threshold * (double)nb)));
    else if (mode == EPA_HEUR_BASEBALL)
      cap = std::max<uint64_t>(cap, (uint64_t)Q * std::min<size_t>(nb, 46));
    uint32_t max_span = 0, n_unique = 0;
    for (const uint32_t s : enc.win_span) max_span = std::max(max_span, s);
    rep.resize(Q);
    first.resize(Q);
    epa_dev_set_query_layout(dev.ctx(), enc.stride);
    epa_dev_set_query_packing(dev.ctx(), enc.bits);
    for (;;) {
      if (pairs.size() < cap) pairs.resize(cap);
      if (res.size() < cap) res.resize(cap);
      const int rc = epa_dev_place_chunk_dedup(dev.ctx(), enc.codes.data(), enc.win_begin.data(), enc.win_span.data(), (uint32_t)Q,
                                               max_span, options.prescoring_threshold, pairs.data(), res.data(), cap, &n, nullptr,
                                               rep.data(), first.data(), &n_unique);
      if (rc == EPA_ERR_PAIR_OVERFLOW && cap < (uint64_t)Q * nb) {
        cap = std::min<uint64_t>(cap * 8, (uint64_t)Q * nb);   // candidate overflow
        continue;
      }
      if (rc == EPA_ERR_NEG_INF) throw std::runtime_error{epa_dev_last_error(dev.ctx())};
      if (rc != EPA_OK) fail_dev(rc);
      break;
    }
    st.seconds_place += since(ts);

    ts = clk::now();
    // One PQuery per class, in order of first appearance; the pairs arrive branch-major, which is the order inside every
    // pquery.  Its header is the class's names in file order joined by `", "`: jplace_chunk_text writes a header between
    // the quotes of "n": ["..."], so the object comes out as "n": ["a", "b", "c"]
    std::vector<PQuery> by_class(n_unique);
    {
      std::vector<std::string> names(n_unique);
      for (size_t q = 0; q < Q; ++q) {
        std::string& s = names[rep[q]];
        if (!s.empty()) s += "\", \"";
        s += chunk[q].header();
      }
      for (uint32_t u = 0; u < n_unique; ++u) by_class[u] = PQuery(offset + first[u], std::move(names[u]));
    }
    for (uint64_t i = 0; i < n; ++i)
      by_class[pairs[i].seq_id].emplace_back(pairs[i].branch_id, res[i].lnl, res[i].pendant_length, res[i].distal_length);
    Sample sample;
    for (PQuery& pq : by_class)
      if (pq.size()) sample.push_back(std::move(pq));
    st.seconds_sample += since(ts);
    ts = clk::now();
    compute_and_set_lwr(sample);
    filter(sample, options);
    st.seconds_post += since(ts);
    ts = clk::now();
    texts.push_back(jplace_chunk_text(sample, options.precision, &tree.mapper()));
    st.seconds_text += since(ts);
    st.queries += Q;
    st.dedup_unique += n_unique;
    st.pairs += n;
    offset += Q;
  }

  ts = clk::now();
  std::string dir = outdir;
  if (!dir.empty() && dir.back() != '/') dir += "/";
  const std::string out_path = dir + "epa_result.jplace";
  std::ofstream os(out_path);
  if (!os) throw std::runtime_error{"cannot open " + out_path};
  write_jplace_text(os, texts, tree.numbered_newick(options.precision), invocation);
  os.flush();
  if (!os) { os.close(); std::remove(out_path.c_str()); throw std::runtime_error{"writing " + out_path + " failed"}; }
  st.seconds_write = since(ts);
  st.seconds_loop = since(t_loop);
  return st;
}

}  // namespace epa
