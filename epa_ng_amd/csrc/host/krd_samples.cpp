// --krd A.jplace,B.jplace,..: Kantorovich-Rubinstein distances between placement samples.  Every file is one sample: its
// rows become point masses (multiplicity x like_weight_ratio at edge_num / distal_length, read_jplace_masses), normalised
// to a total of 1; the matrix, and with --krd-masses the per-edge and per-clade masses, come from ONE epa_dev_krd call on
// the tree's topology.  Everything that can be refused without a device is refused before one is opened.
// --squash: the same samples clustered by ONE epa_dev_squash call, which returns the matrix too (krd.tsv is byte for byte
// the file written without the flag); squash.tsv and squash.newick come from squash_texts.
// --epca K: ONE epa_dev_epca call on the same masses beside the call above, which it does not touch; epca_eigenvalues.tsv,
// epca_projection.tsv and epca_edges.tsv come from epca_texts.
#include <chrono>
#include <cmath>
#include <cctype>
#include <cstdio>
#include <cstring>
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

void write_text(const std::string& path, const std::string& text) {
  std::ofstream os(path);
  if (!os) throw std::runtime_error{"cannot open " + path};
  os << text;
  os.flush();
  if (!os) { os.close(); std::remove(path.c_str()); throw std::runtime_error{"writing " + path + " failed"}; }
}

}  // namespace

bool squash_name_ok(const std::string& name) {
  for (const char ch : name)
    if (std::strchr("(),:;[]'", ch) || std::isspace((unsigned char)ch)) return false;
  return true;
}

void squash_texts(const std::vector<std::string>& names, const uint32_t* merge_a, const uint32_t* merge_b, const double* merge_dist,
                  const uint32_t* merge_size, unsigned int precision, std::string& table, std::string& newick) {
  const size_t S = names.size(), steps = S ? S - 1 : 0;
  if (!S) throw std::runtime_error{"squash: no samples"};
  std::vector<char> buf(400 + (size_t)precision);
  auto fixed = [&](double v) { return std::string(buf.data(), format_fixed(buf.data(), buf.size(), v, precision)); };
  auto label = [&](size_t id) { return id < S ? names[id] : "cluster" + std::to_string(id - S); };
  auto height = [&](size_t id) { return id < S ? 0.0 : merge_dist[id - S] / 2; };
  table = "step\ta\tb\tdistance\tsize\n";
  std::vector<std::string> text(S + steps);   // a cluster's subtree, moved into its parent's
  std::vector<char> used(S + steps, 0);
  for (size_t s = 0; s < S; ++s) text[s] = names[s];
  for (size_t t = 0; t < steps; ++t) {
    const size_t a = merge_a[t], b = merge_b[t], me = S + t;
    if (!(a < b && b < me) || used[a] || used[b])
      throw std::runtime_error{"squash: step " + std::to_string(t) + " merges " + std::to_string(a) + " and " + std::to_string(b) +
                               ": not two clusters that exist and are unmerged at that step"};
    used[a] = used[b] = 1;
    table += std::to_string(t) + '\t' + label(a) + '\t' + label(b) + '\t' + fixed(merge_dist[t]) + '\t' + std::to_string(merge_size[t]) + '\n';
    std::string node = "(";
    node += text[a]; node += ':'; node += fixed(height(me) - height(a)); node += ',';
    node += text[b]; node += ':'; node += fixed(height(me) - height(b)); node += ')';
    node += label(me);
    std::string().swap(text[a]);
    std::string().swap(text[b]);
    text[me].swap(node);
  }
  newick = text[S + steps - 1] + ";\n";
}

void epca_texts(const std::vector<std::string>& names, size_t K, size_t B, const double* eigenvalue, double total_var,
                const double* edge_vec, const double* proj, unsigned int precision, std::string& eigenvalues, std::string& projection,
                std::string& edges) {
  const size_t S = names.size();
  if (S < 2) throw std::runtime_error{"epca: " + std::to_string(S) + " samples: principal components need two at least"};
  if (K < 1 || K >= S)
    throw std::runtime_error{"epca: " + std::to_string(K) + " components: " + std::to_string(S) + " samples have 1 .. " + std::to_string(S - 1)};
  std::vector<char> buf(400 + (size_t)precision);
  auto fixed = [&](double v) { return std::string(buf.data(), format_fixed(buf.data(), buf.size(), v, precision)); };
  std::string pcs;
  for (size_t k = 0; k < K; ++k) pcs += "\tpc" + std::to_string(k + 1);
  eigenvalues = "component\teigenvalue\tfraction\n";
  for (size_t k = 0; k < K; ++k)
    eigenvalues += std::to_string(k + 1) + '\t' + fixed(eigenvalue[k]) + '\t' + fixed(total_var == 0.0 ? 0.0 : eigenvalue[k] / total_var) + '\n';
  projection = "sample" + pcs + '\n';
  for (size_t s = 0; s < S; ++s) {
    projection += names[s];
    for (size_t k = 0; k < K; ++k) { projection += '\t'; projection += fixed(proj[s * K + k]); }
    projection += '\n';
  }
  edges = "edge_num" + pcs + '\n';
  for (size_t b = 0; b < B; ++b) {   // edge_num is the branch id, as in the mass tables
    edges += std::to_string(b);
    for (size_t k = 0; k < K; ++k) { edges += '\t'; edges += fixed(edge_vec[k * B + b]); }
    edges += '\n';
  }
}

Run_Stats krd_files(const Tree& tree, const std::vector<std::string>& files, const std::vector<std::string>& names,
                    const std::string& outdir, const Options& options, bool masses, bool squash, int device, unsigned int epca) {
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
  auto check = [&](int rc) {
    if (rc != EPA_OK)
      throw std::runtime_error{std::string(epa_dev_last_error(dev.ctx())) + " (epa_dev status " + std::to_string(rc) + ")"};
  };
  std::vector<uint32_t> merge_a, merge_b, merge_size;
  std::vector<double> merge_dist;
  if (squash) {
    merge_a.resize(S - 1); merge_b.resize(S - 1); merge_size.resize(S - 1); merge_dist.resize(S - 1);
    check(epa_dev_squash(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)S, merge_a.data(),
                         merge_b.data(), merge_dist.data(), merge_size.data(), krd.data()));
    if (masses) {   // the masses are epa_dev_krd's outputs; its matrix has the bits the call above returned
      std::vector<double> again(S * S);
      check(epa_dev_krd(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)S, again.data(), edge.data(),
                        clade.data()));
    }
  } else {
    check(epa_dev_krd(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)S, krd.data(),
                      masses ? edge.data() : nullptr, masses ? clade.data() : nullptr));
  }
  std::vector<double> pc_eig, pc_vec, pc_proj;
  double pc_total = 0.0;
  uint32_t pc_sweeps = 0;
  if (epca) {   // a call of its own beside the one above, which it does not touch
    pc_eig.resize(epca); pc_vec.resize((size_t)epca * B); pc_proj.resize(S * epca);
    check(epa_dev_epca(dev.ctx(), pairs.data(), distal.data(), weight.data(), pairs.size(), (uint32_t)S, epca, pc_eig.data(),
                       pc_vec.data(), pc_proj.data(), &pc_total, &pc_sweeps, nullptr, nullptr));
  }
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
  if (squash) {
    std::string table, newick;
    squash_texts(names, merge_a.data(), merge_b.data(), merge_dist.data(), merge_size.data(), options.precision, table, newick);
    write_text(dir + "squash.tsv", table);
    write_text(dir + "squash.newick", newick);
    std::cout << "Squash clustering: " << S - 1 << " merges." << std::endl;
  }
  if (epca) {
    std::string eigenvalues, projection, edges;
    epca_texts(names, epca, B, pc_eig.data(), pc_total, pc_vec.data(), pc_proj.data(), options.precision, eigenvalues, projection, edges);
    write_text(dir + "epca_eigenvalues.tsv", eigenvalues);
    write_text(dir + "epca_projection.tsv", projection);
    write_text(dir + "epca_edges.tsv", edges);
    std::cout << "Edge PCA: " << epca << " components (" << pc_sweeps << " Jacobi sweeps)." << std::endl;
  }
  st.seconds_write = std::chrono::duration<double>(clk::now() - ts).count();
  st.seconds_loop = std::chrono::duration<double>(clk::now() - t_loop).count();
  return st;
}

}  // namespace epa
