// Aligned FASTQ reader (quality-aware queries, place_profile.cpp): four lines per record -- '@' name, the aligned read,
// '+', one Phred+33 quality character per alignment column.  Text only: nothing here needs the device library, so the
// reader can be linked and checked on its own (tests/host_driver).
#include <cctype>
#include <fstream>

#include "epa_host.hpp"

namespace epa {

bool is_fastq_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  char c = 0;
  while (f.get(c))
    if (c != '\n' && c != '\r' && c != ' ' && c != '\t') return c == '@';
  return false;
}

Fastq_Stream::Fastq_Stream(const std::string& path) : path_(path), in_(path, std::ios::binary) {
  if (!in_) throw std::runtime_error{"file_check failed: " + path};
}

// one line without its line end; false at the end of the file
static bool fastq_line(std::istream& in, std::string& line) {
  if (!std::getline(in, line)) return false;
  while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
  return true;
}

size_t Fastq_Stream::read_next(std::vector<Fastq_Record>& out, size_t max_records) {
  size_t n = 0;
  std::string head, plus;
  while (n < max_records) {
    do {
      if (!fastq_line(in_, head)) return n;
    } while (head.empty());   // blank lines between records
    const std::string where = path_ + ": FASTQ record " + std::to_string(records_ + 1);
    if (head[0] != '@') throw std::runtime_error{where + ": the header line does not begin with '@'"};
    Fastq_Record r;
    r.header = head.substr(1);
    const std::string named = where + " ('" + r.header + "')";
    if (!fastq_line(in_, r.sequence) || !fastq_line(in_, plus) || !fastq_line(in_, r.quality))
      throw std::runtime_error{named + ": the record is incomplete (four lines: @name, aligned read, +, qualities)"};
    if (plus.empty() || plus[0] != '+') throw std::runtime_error{named + ": the third line does not begin with '+'"};
    if (r.sequence.size() != r.quality.size())
      throw std::runtime_error{named + ": the read has " + std::to_string(r.sequence.size()) + " columns, its quality line " +
                               std::to_string(r.quality.size()) + " (an aligned FASTQ carries one quality character per alignment column)"};
    for (char& c : r.sequence) c = (char)std::toupper((unsigned char)c);
    for (const char c : r.quality)
      if (c < 33 || c > 126) throw std::runtime_error{named + ": a quality character lies outside Phred+33 ('!' .. '~')"};
    out.push_back(std::move(r));
    ++records_;
    ++n;
  }
  return n;
}

MSA_Info fastq_msa_info(const std::string& path) {
  MSA_Info info;
  Fastq_Stream in(path);
  std::vector<Fastq_Record> part;
  for (;;) {
    part.clear();
    if (in.read_next(part, 4096) == 0) break;
    for (const Fastq_Record& r : part) info.add(r.sequence);
  }
  return info;
}

}  // namespace epa
