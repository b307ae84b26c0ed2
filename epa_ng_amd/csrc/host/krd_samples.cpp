// --krd A.jplace,B.jplace,..: Kantorovich-Rubinstein distances between placement samples.  Every file is one sample: its
// rows become point masses (multiplicity x like_weight_ratio at edge_num / distal_length, read_jplace_masses), normalised
// to a total of 1; the matrix, and with --krd-masses the per-edge and per-clade masses, come from ONE epa_dev_krd call on
// the tree's topology.  Everything that can be refused without a device is refused before one is opened.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "epa_host.hpp"

namespace epa {

namespace {

// rows x cols values as a tab-separated table: a header line, then one line per row led by its name
void write_table(const std::string& path, const std::vector<std::string>& header, const std::vector<std::string>& row_names,
                 const std::vector<double>& v, size_t cols, unsigned int precision) {
  std::ofstream os(path);
  if (!os) throw std::runtime_error{"cannot open " + path};
  std::string line = "sample";
  for (const std::string& h : header) { line += '\t'; line += h; }
  line += '\n';
  os << line;
  std::vector<char> buf(400 + (size_t)precision);
  for (size_t r = 0; r < row_names.size(); ++r) {
    line = row_names[r];
    for (size_t c = 0; c < cols; ++c) {
      line += '\t';
      line.append(buf.data(), format_fixed(buf.data(), buf.size(), v[r * cols + c], precision));
    }
    line += '\n';
    os << line;
  }
  os.flush();
  if (!os) { os.close(); std::remove(path.c_str()); throw std::runtime_error{"writing " + path + " failed"}; }
}

}  // namespace

Run_Stats krd_files(const Tree& tree, const std::vector<std::string>& files, const std::vector<std::string>& names,
                    const std::string& outdir, const Options& options, bool masses, int device) {
  using clk = std::chrono::steady_clock;
  // ---- everything that can be refused without a device
  if (tree.mapper())
    throw std::runtime_error{"--krd: the reference tree is rooted and --preserve-rooting is on: the file's edge numbers "
                             "are the rooted tree's, which cannot be mapped back to the unrooted working tree in this "
                             "version; run with --preserve-rooting off"};
  const size_t B = tree.num_branches(), S = files.size();
  std::vector<double> blen;
  {
    epa_tree_desc d;
    Tree::Tree_Desc_Storage store;
    tree.fill_tree_desc(d, store);
    blen.swap(store.blen);
  }
  Run_Stats st;
  auto ts = clk::now();
  std::vector<epa_pair> pairs;
  std::vector<double> distal, weight;
  for (size_t s = 0; s < S; ++s) {
    const std::vector<Jplace_Mass> rows = read_jplace_masses(files[s], blen);
    double total = 0.0;
    for (const Jplace_Mass& r : rows) total += r.mass;   // in file order
    if (!std::isfinite(total)) throw std::runtime_error{files[s] + ": the masses of sample '" + names[s] + "' do not add up to a finite total"};
    if (!(total > 0.0))
      throw std::runtime_error{files[s] + ": sample '" + names[s] + "' has a total mass of 0: there is nothing to compare"};
    for (const Jplace_Mass& r : rows) {
      pairs.push_back(epa_pair{r.edge_num, (uint32_t)s});
      distal.push_back(r.distal_length);
      weight.push_back(r.mass / total);
    }
    st.pairs += rows.size();
  }
  st.queries = S;
  st.seconds_read = std::chrono::duration<double>(clk::now() - ts).count();

  // ---- device
  st.host_threads = configure_host_threads();
  st.chunk_path = "krd";
  ts = clk::now();
  Device_Evaluator dev(tree, options, device);
  st.ref_tree_logl = dev.ref_tree_logl(0);
  st.seconds_setup = std::chrono::duration<double>(clk::now() - ts).count();
  if (dev.lookup_blocks()) { st.lookup_mode = "blocks"; st.lookup_block = dev.lookup_block(); }
  const auto t_loop = clk::now();
  ts = clk::now();
  dev.set_topology(tree);
  std::vector<double> krd(S * S), edge, clade;
  if (masses) { edge.resize(S * B); clade.resize(S * B); }
  const int rc = epa_dev_krd(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)S, krd.data(),
                             masses ? edge.data() : nullptr, masses ? clade.data() : nullptr);
  if (rc != EPA_OK)
    throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
  st.seconds_place = std::chrono::duration<double>(clk::now() - ts).count();
  std::cout << "Kantorovich-Rubinstein distances between " << S << " samples (" << st.pairs << " placements)." << std::endl;

  ts = clk::now();
  std::string dir = outdir;
  if (!dir.empty() && dir.back() != '/') dir += "/";
  write_table(dir + "krd.tsv", names, names, krd, S, options.precision);
  if (masses) {
    std::vector<std::string> edges(B);
    for (size_t b = 0; b < B; ++b) edges[b] = std::to_string(b);
    write_table(dir + "edge_masses.tsv", edges, names, edge, B, options.precision);
    write_table(dir + "clade_masses.tsv", edges, names, clade, B, options.precision);
  }
  st.seconds_write = std::chrono::duration<double>(clk::now() - ts).count();
  st.seconds_loop = std::chrono::duration<double>(clk::now() - t_loop).count();
  return st;
}

}  // namespace epa
