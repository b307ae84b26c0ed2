// Stand-alone driver of the host text layer: jplace writer and reader, newick and model-descriptor parsers, FASTA /
// bfast / FASTQ readers.  Links io.cpp, tree.cpp, model.cpp, aa_models.cpp, parse_model.cpp and fastq.cpp only: no
// device library, no GPU.  tests/host_driver_util.py builds it twice (address + undefined-behaviour sanitizers, and the
// product's -O2) and tests/test_host_text_cpu.py runs it as a child process.
//
//   host_text_driver <command> <arguments ...>
//
// prints one line per input, "ok ..." or "throw: <what()>", and exits 0 in both cases: a sanitizer report (or a crash)
// is the only way to another exit status.  Strings that may hold any byte are printed as hex.
//
// configure_host_threads / set_thread_team / set_host_thread_limit are defined HERE, not linked from place.cpp: the
// product's versions also set the device library's encoder threads (epa_encode_set_threads), so they cannot move into a
// device-free file unchanged.  The driver's version applies the thread count the command line asks for.
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <omp.h>

#include "epa_host.hpp"

namespace {
int g_threads = 1;
}
namespace epa {
int configure_host_threads() { omp_set_num_threads(g_threads); return g_threads; }
void set_thread_team(int) {}
void set_host_thread_limit(int n) { if (n > 0) g_threads = n; }
}  // namespace epa

namespace {

std::string hex(const std::string& s) {
  static const char* d = "0123456789abcdef";
  std::string o;
  for (unsigned char c : s) { o += d[c >> 4]; o += d[c & 15]; }
  return o.empty() ? "-" : o;
}
std::string unhex(const std::string& s) {
  if (s == "-") return "";
  std::string o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o += (char)std::stoi(s.substr(i, 2), nullptr, 16);
  return o;
}
std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error{"driver: cannot open " + path};
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}
std::string dbl(double v) {
  char b[64];
  std::snprintf(b, sizeof(b), "%a", v);
  return b;
}

// one line per input: what body() returns, or the exception's text
void guarded(const std::function<std::string()>& body) {
  std::string line;
  try {
    line = body();
  } catch (const std::exception& e) {
    line = std::string("throw: ") + e.what();
  }
  for (char& c : line) if (c == '\n' || c == '\r') c = ' ';
  std::printf("%s\n", line.c_str());
  std::fflush(stdout);
}

// ---- writer <spec> <outdir>: every case of the spec -> <outdir>/<index>.jplace (write_jplace_text over the case's
// chunks, each from jplace_chunk_text).  Spec, white-space separated:
//   case <precision> <extra> <threads> <hex newick> <hex invocation> <chunks>
//   mapper 0 | mapper <n> <map x n> <utree_root_edge> <rtree_proximal_edge> <rtree_distal_edge> <prox_len> <dist_len>
//   per chunk: chunk <objects>, per object: pq <hex name> <rows>, per row: row <edge> <15 values>
//   values: likelihood lwr distal pendant rell elw p_sh p_au p_kh p_wkh p_wsh marginal_like post_prob exp_dist edpl
int cmd_writer(const std::string& spec_path, const std::string& outdir) {
  std::istringstream in(slurp(spec_path));
  std::string tok;
  size_t index = 0;
  auto word = [&]() { std::string w; if (!(in >> w)) throw std::runtime_error{"driver: spec ends early"}; return w; };
  auto num = [&]() { return std::strtod(word().c_str(), nullptr); };
  auto uns = [&]() { return std::strtoull(word().c_str(), nullptr, 10); };
  while (in >> tok) {
    if (tok != "case") throw std::runtime_error{"driver: expected 'case', got " + tok};
    const unsigned precision = (unsigned)uns(), extra = (unsigned)uns();
    g_threads = (int)uns();
    const std::string newick = unhex(word()), invocation = unhex(word());
    const size_t chunks = uns();
    epa::Rtree_Mapper mapper;
    if (word() != "mapper") throw std::runtime_error{"driver: expected 'mapper'"};
    const size_t nmap = uns();
    for (size_t i = 0; i < nmap; ++i) mapper.map_.push_back((unsigned)uns());
    if (nmap) {
      mapper.utree_root_edge = (unsigned)uns();
      mapper.rtree_proximal_edge = (unsigned)uns();
      mapper.rtree_distal_edge = (unsigned)uns();
      mapper.proximal_edge_length = num();
      mapper.distal_edge_length = num();
    }
    std::vector<epa::Sample> samples(chunks);
    for (auto& sample : samples) {
      if (word() != "chunk") throw std::runtime_error{"driver: expected 'chunk'"};
      const size_t objects = uns();
      for (size_t o = 0; o < objects; ++o) {
        if (word() != "pq") throw std::runtime_error{"driver: expected 'pq'"};
        epa::PQuery pq(o, unhex(word()));
        const size_t rows = uns();
        for (size_t r = 0; r < rows; ++r) {
          if (word() != "row") throw std::runtime_error{"driver: expected 'row'"};
          const size_t edge = uns();
          double v[15];
          for (double& x : v) x = num();
          epa::Placement p(edge, v[0], v[3], v[2]);
          p.lwr(v[1]);
          p.rell_support(v[4]); p.elw(v[5]); p.p_sh(v[6]); p.p_au(v[7]);
          p.p_kh(v[8]); p.p_wkh(v[9]); p.p_wsh(v[10]);
          p.marginal_like(v[11]); p.post_prob(v[12]); p.exp_dist(v[13]); p.edpl(v[14]);
          pq.emplace_back(p);
        }
        sample.push_back(std::move(pq));
      }
    }
    const std::string out = outdir + "/" + std::to_string(index) + ".jplace";
    guarded([&]() {
      std::vector<std::string> texts;
      for (const auto& s : samples) texts.push_back(epa::jplace_chunk_text(s, precision, nmap ? &mapper : nullptr, extra));
      std::ofstream os(out, std::ios::binary);
      epa::write_jplace_text(os, texts, newick, invocation, extra);
      os.close();
      if (!os) throw std::runtime_error{"driver: cannot write " + out};
      size_t bytes = 0;
      for (const auto& t : texts) bytes += t.size();
      return "ok " + std::to_string(index) + " " + std::to_string(bytes);
    });
    ++index;
  }
  return 0;
}

// ---- readjplace <file> ...: ok <objects> then per object " <hex name>" and per row ",<edge>:<distal %a>:<pendant %a>"
std::string read_jplace_line(const std::string& path) {
  const auto pqs = epa::read_jplace(path);
  std::string o = "ok " + std::to_string(pqs.size());
  for (const auto& pq : pqs) {
    o += " " + hex(pq.name);
    for (const auto& r : pq.rows) o += "," + std::to_string(r.edge_num) + ":" + dbl(r.distal_length) + ":" + dbl(r.pendant_length);
  }
  return o;
}

std::string msa_line(const epa::MSA& m) {
  std::string o = "ok " + std::to_string(m.size());
  for (const auto& s : m) o += " " + hex(s.header()) + ":" + hex(s.sequence());
  return o;
}

// ---- fasta <chunk> <file> ...: every record through Fasta_Stream::read_next, `chunk` at a time (FASTA or bfast)
std::string fasta_line(const std::string& path, size_t chunk) {
  epa::Fasta_Stream in(path);
  epa::MSA all;
  while (in.read_next(all, chunk)) {}
  return msa_line(all);
}

// ---- views <sites> <chunk> <file> ...: the chunk loop's order (place.cpp): read_next_views, and read_next for a chunk
// the views refuse.  ok <n> <views chunks> <read_next chunks> then the records
std::string views_line(const std::string& path, size_t sites, size_t chunk) {
  epa::Fasta_Stream in(path);
  epa::MSA all;
  size_t by_views = 0, by_read = 0;
  for (;;) {
    epa::MSA part;
    std::vector<const char*> rows;
    in.read_next_views(part, rows, sites, chunk);
    if (!rows.empty()) {
      ++by_views;
      for (size_t i = 0; i < part.size(); ++i) {
        std::string s(rows[i], sites);
        for (char& c : s) c = (char)std::toupper((unsigned char)c);
        all.emplace_back(part[i].header(), s);
      }
      continue;
    }
    if (in.read_next(part, chunk) == 0) break;
    ++by_read;
    for (auto& s : part) all.push_back(s);
  }
  return msa_line(all) + " views=" + std::to_string(by_views) + " read=" + std::to_string(by_read);
}

// ---- wire <sites> <chunk> <premask> <file> ...: bfast records through read_next_wire: per record
// " <hex header>:<win_begin>:<win_span>:<hex codes of the row>"
std::string wire_line(const std::string& path, size_t sites, size_t chunk, bool premask) {
  epa::Fasta_Stream in(path);
  std::string o;
  size_t total = 0;
  for (;;) {
    epa::MSA m;
    epa::Encoded_Chunk e;
    const size_t n = in.read_next_wire(m, e, sites, chunk, premask);
    if (!n) break;
    const size_t ps = (e.stride + 1) / 2;
    for (size_t i = 0; i < n; ++i)
      o += " " + hex(m[i].header()) + ":" + std::to_string(e.win_begin[i]) + ":" + std::to_string(e.win_span[i]) + ":" +
           hex(std::string((const char*)e.codes.data() + i * ps, (e.win_span[i] + 1) / 2));
    total += n;
  }
  return "ok " + std::to_string(total) + (in.is_bfast() ? " bfast" : " fasta") + o;
}

// ---- fastq <chunk> <file> ...: ok <n> fastq=<is_fastq_file> then " <hex header>:<hex read>:<hex quality>", then the
// column mask of fastq_msa_info
std::string fastq_line(const std::string& path, size_t chunk) {
  const bool is = epa::is_fastq_file(path);
  epa::Fastq_Stream in(path);
  std::vector<epa::Fastq_Record> all;
  while (in.read_next(all, chunk)) {}
  std::string o = "ok " + std::to_string(all.size()) + " fastq=" + (is ? "1" : "0");
  for (const auto& r : all) o += " " + hex(r.header) + ":" + hex(r.sequence) + ":" + hex(r.quality);
  const epa::MSA_Info info = epa::fastq_msa_info(path);
  o += " sites=" + std::to_string(info.sites()) + " mask=";
  for (uint8_t g : info.gap_mask()) o += g ? '1' : '0';
  return o;
}

// ---- tree <fasta> <model> <lnl 0|1> <newick file> ...: ok B=<branches> rooted=<0|1> lnl=<%.6f at branch 0 | -> then
// the numbered newick at precision 6
std::string tree_line(const epa::MSA& msa, const epa::Model& model, bool lnl, const std::string& newick_path) {
  const epa::Tree tree(slurp(newick_path), msa, model, epa::Options{});
  char b[64] = "-";
  if (lnl) std::snprintf(b, sizeof(b), "%.6f", tree.ref_tree_logl(0));
  std::string o = "ok B=" + std::to_string(tree.num_branches()) + " rooted=" + (tree.rooted_input() ? "1" : "0") + " lnl=" + b;
  if (lnl) o += " " + tree.numbered_newick(6);
  return o;
}

// ---- model <descriptor> ...: ok cats=<n> alpha=<%a> rates=<%a/...> <to_string>
std::string model_line(const std::string& descriptor) {
  const epa::Model m(descriptor);
  std::string o = "ok cats=" + std::to_string(m.num_ratecats()) + " states=" + std::to_string(m.num_states()) + " pinv=" + dbl(m.pinv()) + " rates=";
  for (size_t k = 0; k < m.ratecat_rates().size(); ++k) o += (k ? "/" : "") + dbl(m.ratecat_rates()[k]);
  return o + " " + m.to_string();
}

}  // namespace

int main(int argc, char** argv) {
  const std::vector<std::string> a(argv + 1, argv + argc);
  try {
    if (a.empty()) throw std::runtime_error{"driver: no command"};
    const std::string& cmd = a[0];
    auto need = [&](size_t n) { if (a.size() < n + 1) throw std::runtime_error{"driver: " + cmd + " needs " + std::to_string(n) + " arguments"}; };
    if (cmd == "writer") { need(2); return cmd_writer(a[1], a[2]); }
    if (cmd == "readjplace") {
      for (size_t i = 1; i < a.size(); ++i) guarded([&]() { return read_jplace_line(a[i]); });
    } else if (cmd == "fasta") {
      need(1);
      for (size_t i = 2; i < a.size(); ++i) guarded([&]() { return fasta_line(a[i], std::stoul(a[1])); });
    } else if (cmd == "views") {
      need(2);
      for (size_t i = 3; i < a.size(); ++i) guarded([&]() { return views_line(a[i], std::stoul(a[1]), std::stoul(a[2])); });
    } else if (cmd == "wire") {
      need(3);
      for (size_t i = 4; i < a.size(); ++i) guarded([&]() { return wire_line(a[i], std::stoul(a[1]), std::stoul(a[2]), a[3] == "1"); });
    } else if (cmd == "fastq") {
      need(1);
      for (size_t i = 2; i < a.size(); ++i) guarded([&]() { return fastq_line(a[i], std::stoul(a[1])); });
    } else if (cmd == "tree") {
      need(3);
      epa::MSA msa;
      std::unique_ptr<epa::Model> model;
      for (size_t i = 4; i < a.size(); ++i)
        guarded([&]() {
          if (!model) { msa = epa::read_fasta(a[1]); model.reset(new epa::Model(a[2])); }
          return tree_line(msa, *model, a[3] == "1", a[i]);
        });
    } else if (cmd == "model") {
      for (size_t i = 1; i < a.size(); ++i) guarded([&]() { return model_line(a[i]); });
    } else if (cmd == "parse_model") {
      for (size_t i = 1; i < a.size(); ++i) guarded([&]() { return "ok " + epa::parse_model(a[i]); });
    } else if (cmd == "threads") {   // the thread count jplace_chunk_text really gets: a self-check of the build
      need(1);
      g_threads = std::stoi(a[1]);
      int got = 0;
#pragma omp parallel num_threads(epa::configure_host_threads())
      {
#pragma omp single
        got = omp_get_num_threads();
      }
      std::printf("ok %d\n", got);
    } else {
      throw std::runtime_error{"driver: unknown command " + cmd};
    }
  } catch (const std::exception& e) {
    std::printf("throw: %s\n", e.what());
  }
  return 0;
}
