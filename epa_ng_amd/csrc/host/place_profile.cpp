// -q reads.fastq: quality-aware placement.  An ALIGNED FASTQ carries, per record, the aligned read (alignment width,
// '-' gaps) and a quality line of the same width (Phred+33, ignored wherever the read shows no pure state).  Every base
// becomes a row of state likelihoods under the standard tip-error model (epa_profile_from_phred) and the chunk body is
// epa_dev_place_chunk_profile: preplacement from the resident lookup table, the context's heuristic, the general Newton
// kernel (include/epa_dev.h, "Profile queries").  The loop is synchronous and uses one device; LWR, filter and jplace
// text are the host stages of the coded run (place.cpp, io.cpp).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "epa_host.hpp"

namespace epa {

// the FASTQ reader itself (Fastq_Stream, is_fastq_file, fastq_msa_info) is text only and lives in fastq.cpp

Run_Stats place_profile_file(const Tree& tree, const std::string& query_file, const MSA_Info& msa_info, const std::string& outdir,
                             const Options& options, const std::string& invocation, int device) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
  if (!options.prescoring) throw std::runtime_error{"a FASTQ query is preplaced from the lookup table: --no-heur is not supported with it"};
  if (options.memsave == Options::Memsave::kOn)
    throw std::runtime_error{"a FASTQ query is preplaced from the resident lookup table: --memsave on is not supported with it"};
  const bool premask = options.premasking && msa_info.gap_count() > 0;
  const uint32_t S = (uint32_t)tree.model().num_states(), W = (uint32_t)tree.num_sites();
  const size_t nb = tree.num_branches();
  Run_Stats st;
  st.host_threads = configure_host_threads();
  st.chunk_path = "profile";
  st.query_kind = "profile";
  auto ts = clk::now();
  Options dev_options = options;
  dev_options.memsave = Options::Memsave::kOff;   // the resident layout or none: --memsave auto must not fall back to blocks
  Device_Evaluator dev(tree, dev_options, device);
  st.ref_tree_logl = dev.ref_tree_logl(0);
  st.seconds_setup = since(ts);
  const auto t_loop = clk::now();
  auto fail_dev = [&](int rc) {
    throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
  };
  const int mode = options.baseball ? EPA_HEUR_BASEBALL : options.prescoring_by_percentage ? EPA_HEUR_FIXED : EPA_HEUR_DYNAMIC;
  if (epa_dev_set_heuristic(dev.ctx(), mode, mode == EPA_HEUR_FIXED ? options.prescoring_threshold : 0.0) != EPA_OK)
    throw std::runtime_error{epa_dev_last_error(dev.ctx())};

  // a row of S doubles per base is 8 S times a code: the default chunk is smaller than the coded run's; an explicit
  // --chunk-size is honoured as given
  const size_t per_chunk = std::max<size_t>(1, options.chunk_size_given ? options.chunk_size : 10000);
  st.device_chunk = per_chunk;
  Fastq_Stream reader(query_file);
  std::vector<std::string> texts;
  std::vector<Fastq_Record> chunk;
  std::vector<uint8_t> codes, phred;
  std::vector<uint32_t> wb, ws;
  std::vector<double> prof;
  std::vector<epa_pair>& pairs = dev.pair_buffer();
  std::vector<epa_result>& res = dev.result_buffer();
  size_t offset = 0;
  for (;;) {
    ts = clk::now();
    chunk.clear();
    const size_t Q = reader.read_next(chunk, per_chunk);
    if (Q == 0) break;
    st.seconds_read += since(ts);
    ts = clk::now();
    std::vector<const char*> rows(Q);
    for (size_t q = 0; q < Q; ++q) {
      Fastq_Record& r = chunk[q];
      if (premask) {   // both lines by the same column mask
        r.sequence = subset_sequence(r.sequence, msa_info.gap_mask());
        r.quality = subset_sequence(r.quality, msa_info.gap_mask());
      }
      if (r.sequence.size() != W) throw std::runtime_error{"Query sequence length not same as reference alignment!"};
      rows[q] = r.sequence.c_str();
    }
    wb.assign(Q, 0);
    ws.assign(Q, 0);
    uint32_t bad = 0;
    auto check = [&](int rc) {
      if (rc == EPA_ERR_QUERY_ALL_GAP)
        throw std::runtime_error{"Sequence with header '" + chunk[bad].header + "' does not appear to have any non-gap sites!"};
      if (rc == EPA_ERR_INVALID_CHAR) throw std::runtime_error{"char is invalid! (sequence '" + chunk[bad].header + "')"};
      if (rc != EPA_OK) throw std::runtime_error{"query encoding failed"};
    };
    check(epa_encode_queries_compact(S, W, (uint32_t)Q, rows.data(), options.premasking, options.aa_x_as_n, 0, nullptr, wb.data(),
                                     ws.data(), &bad));
    uint32_t mx = 1;
    for (const uint32_t s : ws) mx = std::max(mx, s);
    const uint32_t stride = mx;
    codes.assign(Q * (size_t)stride, 0);
    check(epa_encode_queries_compact(S, W, (uint32_t)Q, rows.data(), options.premasking, options.aa_x_as_n, stride, codes.data(),
                                     wb.data(), ws.data(), &bad));
    phred.assign(Q * (size_t)stride, 0);
    for (size_t q = 0; q < Q; ++q)
      for (uint32_t j = 0; j < ws[q]; ++j) phred[q * stride + j] = (uint8_t)(chunk[q].quality[wb[q] + j] - 33);
    prof.assign(Q * (size_t)stride * S, 0.0);
    if (epa_profile_from_phred(S, (uint32_t)Q, stride, codes.data(), phred.data(), ws.data(), prof.data()) != EPA_OK)
      throw std::runtime_error{epa_dev_last_error(nullptr)};
    st.seconds_encode += since(ts);

    ts = clk::now();
    uint64_t cap = std::max<uint64_t>((uint64_t)Q * 8, pairs.size()), n = 0;
    if (mode == EPA_HEUR_FIXED)
      cap = std::max<uint64_t>(cap, (uint64_t)Q * std::min<size_t>(nb, (size_t)std::ceil(options.prescoring_threshold * (double)nb)));
    else if (mode == EPA_HEUR_BASEBALL)
      cap = std::max<uint64_t>(cap, (uint64_t)Q * std::min<size_t>(nb, 46));
    for (;;) {
      if (pairs.size() < cap) pairs.resize(cap);
      if (res.size() < cap) res.resize(cap);
      const int rc = epa_dev_place_chunk_profile(dev.ctx(), prof.data(), stride, wb.data(), ws.data(), (uint32_t)Q,
                                                 options.prescoring_threshold, pairs.data(), res.data(), cap, &n, nullptr);
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
    // one PQuery per read, in read order; the pairs arrive branch-major, which is the order inside every pquery
    std::vector<PQuery> by_read(Q);
    for (size_t q = 0; q < Q; ++q) by_read[q] = PQuery(offset + q, chunk[q].header);
    for (uint64_t i = 0; i < n; ++i)
      by_read[pairs[i].seq_id].emplace_back(pairs[i].branch_id, res[i].lnl, res[i].pendant_length, res[i].distal_length);
    Sample sample;
    for (PQuery& pq : by_read)
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
