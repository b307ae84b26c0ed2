// epa-ng-amd: command-line front end keeping EPA-ng's flags for the placement path
// (src/main.cpp:96-270).  Flags outside the hot path (binary dump, bfast conversion, --split)
// are rejected with a message, not silently ignored.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "epa_host.hpp"

using namespace epa;

static void usage() {
  std::cout <<
      "epa-ng-amd - Evolutionary Placement Algorithm, MI355X placement evaluator\n"
      "  -t,--tree FILE        reference tree (newick, unrooted or rooted)\n"
      "  -s,--ref-msa FILE     reference MSA (fasta)\n"
      "  -q,--query FILE       query MSA (fasta, aligned to the reference), or an aligned FASTQ (leading '@'): per record\n"
      "                        the aligned read and one Phred+33 quality character per alignment column.  Every base then\n"
      "                        enters as state likelihoods (called state 1 - e, every other state e / (states - 1), e = 10^(-Q / 10)) instead\n"
      "                        of a hard call: one device, chunk by chunk; --devices a,b / --rank / --world / --no-heur /\n"
      "                        --rescore / --memsave on are refused with it\n"
      "  -m,--model STR|FILE   model descriptor, e.g. GTR{..}+FU{..}+G4{a} (default GTR+G), or a RAxML 8\n"
      "                        info / RAxML-NG .bestModel / IQ-TREE report file\n"
      "  -w,--outdir DIR       output directory (default ./)\n"
      "  -g,--dyn-heur X       accumulated-LWR preplacement threshold (default 0.99999)\n"
      "  -G,--fix-heur X       fixed fraction of branches\n"
      "  --baseball-heur       baseball heuristic\n"
      "  --no-heur             thorough placement on every branch\n"
      "  --filter-acc-lwr X | --filter-min-lwr X | --filter-min N | --filter-max N\n"
      "  --rescore FILE.jplace  no placement: evaluate the placements of FILE (jplace version 3: edge_num, distal_length,\n"
      "                        pendant_length of every row) again under this tree, alignment and model; likelihood and\n"
      "                        like_weight_ratio are recomputed, everything else is kept.  No heuristic, optimiser or\n"
      "                        filter flag applies (they are refused); one device; --preserve-rooting off for rooted trees\n"
      "  --rell N              with --rescore: RELL bootstrap support of every row among the rows of its placement object,\n"
      "                        from N (1 .. 1048576) resamplings of the per-site log-likelihoods; written as a sixth\n"
      "                        field \"rell_support\".  Two steps: place first, then --rescore out.jplace --rell N\n"
      "  --rell-seed S         seed of the resampling (default 1); the result depends on N, S and the input file alone\n"
      "  --rell-tests          with --rescore --rell N: two more fields from the same N replicates, directly after\n"
      "                        \"rell_support\": \"elw\", the expected likelihood weight (the like_weight_ratio averaged over\n"
      "                        the replicates; its cumulative sum gives a confidence set), and \"p_sh\", the p-value of the\n"
      "                        Shimodaira-Hasegawa test of the row against the best row of its placement object\n"
      "  --au                  with --rescore --rell N: one more field, \"p_au\", directly after \"rell_support\" (after \"p_sh\" with\n"
      "                        --rell-tests): the p-value of the approximately unbiased test (Shimodaira 2002) of the row, from\n"
      "                        N replicates at each of ten replicate lengths (0.5 .. 1.4 of the sites).  Unlike p_sh it does\n"
      "                        not grow more conservative with the number of rows.  AU wants N of the order of 10000 per\n"
      "                        scale (CONSEL's default)\n"
      "  --kh                  with --rescore --rell N: three more fields from the same N replicates, directly after \"p_au\" (or\n"
      "                        whatever precedes its place): \"p_kh\", the p-value of the Kishino-Hasegawa test of the row against\n"
      "                        the best row of its placement object; \"p_wkh\", the same against the row that is furthest ahead in\n"
      "                        standard deviations of the difference; \"p_wsh\", the weighted Shimodaira-Hasegawa test, which unlike\n"
      "                        p_sh does not let a row far off set the scale for the others.  At most 1024 rows per object\n"
      "  --posterior           with --rescore: marginal likelihood of every row's edge, integrated over the attachment point\n"
      "                        (uniform on the edge) and the pendant length (exponential prior), and its normalisation over\n"
      "                        the rows of the placement object; written as the fields \"marginal_like\" and \"post_prob\"\n"
      "                        (after \"rell_support\", \"elw\", \"p_sh\", \"p_au\", \"p_kh\" .. when --rell, --rell-tests, --au, --kh are given).  Only edge_num of a row enters them\n"
      "  --prior-mean M        mean of the pendant prior (default: the mean branch length of the reference tree)\n"
      "  --posterior-nodes KX,KP  Gauss-Legendre nodes along the edge x Gauss-Laguerre pendant nodes, 1 .. 64 each (default 8,16)\n"
      "  --edpl                with --rescore: the expected distance between placement locations (EDPL, Matsen et al.): are the\n"
      "                        rows of an object neighbours or on opposite sides of the tree?  Two more fields after all others:\n"
      "                        \"exp_dist\", the like_weight_ratio-weighted mean path distance from the row's attachment point to\n"
      "                        the rows of its object, and \"edpl\", the object's value (the weighted mean of exp_dist), repeated\n"
      "                        on each of its rows.  Weights are the recomputed like_weight_ratios; pendant lengths do not enter\n"
      "  --krd A.jplace,B.jplace,..  no placement: every file is one sample of placements on this reference tree (its rows weigh\n"
      "                        multiplicity x like_weight_ratio, normalised to 1 per file); writes krd.tsv, the matrix of\n"
      "                        Kantorovich-Rubinstein (earth mover's) distances between the samples, as `guppy kr` and\n"
      "                        `gappa analyze krd` define it for exponent 1: a header line sample<TAB>names, then one line per\n"
      "                        sample; a sample is named after its file, without directory and .jplace.  Needs -t, -s, -m and\n"
      "                        -w as --rescore does, takes no -q; one device; --rescore / --dedup / --devices a,b / --rank are\n"
      "                        refused with it; --preserve-rooting off for rooted trees\n"
      "  --krd-masses          with --krd: also edge_masses.tsv and clade_masses.tsv, per sample the mass on every edge and in the\n"
      "                        subtree below it (the edge included), columns by edge_num: the inputs of squash clustering and edge PCA\n"
      "  --squash              with --krd: squash clustering of the samples (Matsen & Evans; `guppy squash`, `gappa analyze\n"
      "                        squash`): the two clusters at the smallest distance are merged into the average of their samples'\n"
      "                        masses, whose distances to the others are computed on the tree, until one is left.  Writes\n"
      "                        squash.tsv (step<TAB>a<TAB>b<TAB>distance<TAB>size; a and b are sample names or cluster<k>, the\n"
      "                        cluster of step k) and squash.newick (the cluster tree: inner nodes cluster<k> at height distance / 2,\n"
      "                        branch = height(parent) - height(child), negative where the distances invert) beside krd.tsv.\n"
      "                        Two files at least; sample names with ( ) , : ; [ ] ' or white space are refused\n"
      "  --epca K              with --krd: edge principal components of the samples (Matsen & Evans; `guppy epca`, `gappa analyze\n"
      "                        edgepca`): per sample and inner edge the mass on the edge's child side minus the mass on its root\n"
      "                        side (edges next to a leaf are left out), centred over the samples; the first K principal\n"
      "                        components.  Writes epca_eigenvalues.tsv (component<TAB>eigenvalue<TAB>fraction of the total\n"
      "                        variance), epca_projection.tsv (sample<TAB>pc1..pcK: the samples on those axes) and epca_edges.tsv\n"
      "                        (edge_num<TAB>pc1..pcK: the unit-length axes, zeros on left-out edges; the entry of largest\n"
      "                        magnitude is positive, and an edge's sign follows the rooting at the first branch) beside krd.tsv.\n"
      "                        2 .. 1024 files, K in 1 .. files - 1; combines with --squash and --krd-masses\n"
      "  --precision N         output digits (default 10)\n"
      "  --chunk-size N        queries per chunk (default 50000; EPA-ng's CPU default is 5000)\n"
      "  --device-min-chunk N  a device chunk holds at least N queries whatever --chunk-size says\n"
      "                        (default 40000; 0: chunks of exactly --chunk-size)\n"
      "  --dedup               place identical reads of a chunk once (amplicon / metabarcoding inputs): one placement object per\n"
      "                        class of identical reads, in order of first appearance, its \"n\" listing all the class's names in\n"
      "                        file order.  Classes are per chunk: equal reads in different chunks stay separate objects (raise\n"
      "                        --chunk-size to merge them).  One device, chunk by chunk; --devices a,b / --rank / --world /\n"
      "                        --no-heur / --rescore / a FASTQ query are refused with it\n"
      "  --no-pre-mask         evaluate all sites of every query\n"
      "  --raxml-blo           radius-1 local branch-length optimisation instead of the sliding rule\n"
      "  --rate-scalers auto|on|off  per-rate-category numerical scaling (auto: on above 2000 tips)\n"
      "  --memsave auto|on|off  device lookup tables rebuilt per branch block and chunk instead of resident: 3.1 x\n"
      "                        (nucleotide) / 1.65 x (20 states) larger references fit (auto: only when they have to)\n"
      "  --preserve-rooting on|off  rooted reference tree: report on the rooted tree (default on)\n"
      "  -T,--threads N        upper limit on the host threads (parsing, encoding, LWR / filter, jplace text)\n"
      "  --device N            GPU ordinal (default 0)\n"
      "  --devices a,b,..      place on several GPUs of the node (chunks are dealt to them in turn)\n"
      "  --rank R --world N --comm-file F   one process per GPU: rank R places its contiguous slice of the\n"
      "                        queries, results are gathered to rank 0 over RCCL; rank 0 leaves the RCCL id in F\n"
      "                        (defaults: RANK / WORLD_SIZE / LOCAL_RANK / EPA_COMM_FILE of the environment)\n"
      "  --stats-json FILE     the time breakdown of the run as JSON\n"
      "  --comm-nonce STR      marks this run's id record in F (default: EPA_COMM_NONCE / TORCHELASTIC_RUN_ID); give\n"
      "                        one whenever the launcher can: without it a record is only checked for its age\n"
      "  --comm-probe-seconds S  bound of the handshake every rank runs before placing (default 120)\n"
      "  --comm-timeout S      bound of every later wait for a peer (default EPA_COMM_TIMEOUT_S, else 600)\n"
      "  --comm-rows-per-read N  rows per rank and gather = chunk x N (default 8; more rows take the carry path)\n"
      "                        RCCL is bound at run time: the library named by EPA_RCCL_LIB, else librccl.so.1 on the\n"
      "                        loader's search path (LD_LIBRARY_PATH), else /opt/rocm/lib/librccl.so.1\n";
}

int main(int argc, char** argv) {
  const auto start = std::chrono::steady_clock::now();
  std::string invocation;
  for (int i = 0; i < argc; ++i) { invocation += argv[i]; invocation += " "; }
  std::string tree_file, ref_file, query_file, outdir = "./", model_desc = "GTR+G", stats_json, rescore_file;
  std::vector<std::string> placing_flags;   // flags that steer heuristic, optimiser or filter: meaningless with --rescore
  Options opt;
  int device = 0;
  bool dedup = false;   // --dedup: the loop of place_dedup.cpp
  std::string krd_list;   // --krd: comma-separated jplace files, one sample each (krd_samples.cpp)
  bool krd_given = false, krd_masses = false, krd_squash = false, epca_given = false;
  std::string epca_arg;   // --epca K: edge principal components of the samples of --krd
  bool device_given = false, rell_given = false, prior_given = false, nodes_given = false, rank_given = false;
  std::string diag_flag;   // --host-heuristic / --device-min-chunk: steer the coded chunk loop only
  std::vector<int> devices;
  // one process per GPU (place_ranks.cpp): --rank / --world / --comm-file, or what torchrun / mpirun export
  auto env_int = [](const char* a, const char* b, int dflt) {
    const char* v = std::getenv(a);
    if (!v && b) v = std::getenv(b);
    return v ? std::atoi(v) : dflt;
  };
  int rank = env_int("EPA_RANK", "RANK", 0), world = env_int("EPA_WORLD", "WORLD_SIZE", 1);
  const int local_rank = env_int("EPA_LOCAL_RANK", "LOCAL_RANK", rank);
  std::string comm_file = std::getenv("EPA_COMM_FILE") ? std::getenv("EPA_COMM_FILE") : "";
  if (const char* e = std::getenv("EPA_COMM_NONCE")) opt.comm_nonce = e;
  if (opt.comm_nonce.empty()) if (const char* e = std::getenv("TORCHELASTIC_RUN_ID")) opt.comm_nonce = e;
  auto need = [&](int& i) -> std::string {
    if (i + 1 >= argc) { std::cerr << "missing value for " << argv[i] << "\n"; std::exit(1); }
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-g" || a == "--dyn-heur" || a == "-G" || a == "--fix-heur" || a == "--baseball-heur" || a == "--no-heur" ||
        a == "--raxml-blo" || a.rfind("--filter-", 0) == 0)
      placing_flags.push_back(a);
    if (a == "-t" || a == "--tree") tree_file = need(i);
    else if (a == "-s" || a == "--ref-msa" || a == "--msa") ref_file = need(i);
    else if (a == "-q" || a == "--query") query_file = need(i);
    else if (a == "-m" || a == "--model") model_desc = need(i);
    else if (a == "-w" || a == "--outdir" || a == "--out-dir") outdir = need(i);
    else if (a == "-g" || a == "--dyn-heur") { opt.prescoring_threshold = std::stod(need(i)); opt.prescoring_by_percentage = false; }
    else if (a == "-G" || a == "--fix-heur") { opt.prescoring_threshold = std::stod(need(i)); opt.prescoring_by_percentage = true; }
    else if (a == "--baseball-heur") opt.baseball = true;
    else if (a == "--no-heur") opt.prescoring = false;
    else if (a == "--filter-acc-lwr") { opt.support_threshold = std::stod(need(i)); opt.acc_threshold = true; }
    else if (a == "--filter-min-lwr") { opt.support_threshold = std::stod(need(i)); opt.acc_threshold = false; }
    else if (a == "--filter-min") opt.filter_min = (unsigned)std::stoul(need(i));
    else if (a == "--filter-max") opt.filter_max = (unsigned)std::stoul(need(i));
    else if (a == "--rescore") rescore_file = need(i);
    else if (a == "--rell") { opt.rell_replicates = (unsigned)std::stoul(need(i)); rell_given = true; }
    else if (a == "--rell-seed") { opt.rell_seed = std::stoull(need(i)); rell_given = true; }
    else if (a == "--rell-tests") opt.rell_tests = true;
    else if (a == "--au") opt.au = true;
    else if (a == "--kh") opt.kh = true;
    else if (a == "--posterior") opt.posterior = true;
    else if (a == "--edpl") opt.edpl = true;
    else if (a == "--krd") { krd_list = need(i); krd_given = true; }
    else if (a == "--krd-masses") krd_masses = true;
    else if (a == "--squash") krd_squash = true;
    else if (a == "--epca") { epca_arg = need(i); epca_given = true; }
    else if (a == "--prior-mean") {
      const std::string v = need(i);
      char* end = nullptr;
      opt.prior_mean = std::strtod(v.c_str(), &end);
      if (v.empty() || *end) opt.prior_mean = -1.0;   // not a number: refused below
      prior_given = true;
    }
    else if (a == "--posterior-nodes") {
      const std::string v = need(i);
      unsigned long kx = 0, kp = 0;
      char tail = 0;
      if (std::sscanf(v.c_str(), "%lu,%lu%c", &kx, &kp, &tail) != 2 || v.find('-') != std::string::npos) kx = kp = 0;
      opt.posterior_kx = kx > 64 ? 0u : (unsigned)kx;
      opt.posterior_kp = kp > 64 ? 0u : (unsigned)kp;
      nodes_given = true;
    }
    else if (a == "--precision") opt.precision = (unsigned)std::stoul(need(i));
    else if (a == "--chunk-size") { opt.chunk_size = (unsigned)std::stoul(need(i)); opt.chunk_size_given = true; }
    else if (a == "--device-min-chunk") { diag_flag = a; opt.device_min_chunk = (unsigned)std::stoul(need(i)); opt.device_min_chunk_given = true; }
    else if (a == "--no-pre-mask") opt.premasking = false;
    else if (a == "--raxml-blo") opt.sliding_blo = false;   // src/main.cpp:239-242
    else if (a == "--rate-scalers") {                       // src/main.cpp:248-250,399-407
      const std::string v = need(i);
      if (v == "auto") opt.scaling = Options::NumericalScaling::kAuto;
      else if (v == "on") opt.scaling = Options::NumericalScaling::kOn;
      else if (v == "off") opt.scaling = Options::NumericalScaling::kOff;
      else { std::cerr << "--rate-scalers: " << v << " not in {auto,on,off}\n"; return 1; }
    }
    else if (a == "--memsave") {
      const std::string v = need(i);
      if (v == "auto") opt.memsave = Options::Memsave::kAuto;
      else if (v == "on") opt.memsave = Options::Memsave::kOn;
      else if (v == "off") opt.memsave = Options::Memsave::kOff;
      else { std::cerr << "--memsave: " << v << " not in {auto,on,off}\n"; return 1; }
    }
    else if (a == "--preserve-rooting") {  // src/main.cpp:196-199, 410-418
      const std::string v = need(i);
      if (v == "off") opt.preserve_rooting = false;
      else if (v == "on") opt.preserve_rooting = true;
      else { std::cerr << "--preserve-rooting: " << v << " not in {on,off}\n"; return 1; }
    }
    else if (a == "-T" || a == "--threads") {
      opt.num_threads = (unsigned)std::stoul(need(i));
      set_host_thread_limit((int)opt.num_threads);   // caps the OpenMP host stages; the placement itself runs on the GPU
    }
    else if (a == "--device") { device = std::stoi(need(i)); device_given = true; }
    else if (a == "--devices") {
      std::stringstream ls(need(i));
      std::string tok;
      while (std::getline(ls, tok, ',')) if (!tok.empty()) devices.push_back(std::stoi(tok));
    }
    else if (a == "--rank") { rank = std::stoi(need(i)); rank_given = true; }
    else if (a == "--world") { world = std::stoi(need(i)); rank_given = true; }
    else if (a == "--comm-file") { comm_file = need(i); rank_given = true; }
    else if (a == "--comm-nonce") opt.comm_nonce = need(i);
    else if (a == "--comm-probe-seconds") opt.comm_probe_seconds = std::stod(need(i));
    else if (a == "--comm-timeout") opt.comm_timeout_seconds = std::stod(need(i));
    else if (a == "--comm-rows-per-read") opt.comm_rows_per_read = std::stoi(need(i));
    else if (a == "--comm-self-send") opt.comm_self_send = true;       // test hook
    else if (a == "--host-heuristic") { diag_flag = a; opt.host_heuristic = true; }   // diagnostics
    else if (a == "--no-pipeline") opt.no_pipeline = true;
    else if (a == "--dedup") dedup = true;
    else if (a == "--stats-json") stats_json = need(i);
    else if (a == "--redo" || a == "--verbose") {}
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else { std::cerr << "option " << a << " is outside the placement hot path of this build\n"; return 1; }
  }
  if (opt.edpl && rescore_file.empty()) {   // before anything else: no file is read, no device opened
    std::cerr << "--edpl works on an existing result: place first, then run again with --rescore out.jplace --edpl\n";
    return 1;
  }
  // --krd compares existing results: what it does not do is refused before any file is parsed or a device is opened
  std::vector<std::string> krd_files_list, krd_names;
  if (krd_masses && !krd_given) { std::cerr << "--krd-masses adds the mass tables to the output of --krd and needs it: --krd A.jplace,B.jplace --krd-masses\n"; return 1; }
  if (krd_squash && !krd_given) { std::cerr << "--squash clusters the samples of --krd and needs it: --krd A.jplace,B.jplace,C.jplace --squash\n"; return 1; }
  if (epca_given && !krd_given) { std::cerr << "--epca finds the principal components of the samples of --krd and needs it: --krd A.jplace,B.jplace,C.jplace --epca 2\n"; return 1; }
  if (krd_given) {
    const char* const what = "--krd (distances between placement samples) ";
    if (!query_file.empty()) { std::cerr << what << "reads placements, not sequences: -q is not supported with it\n"; return 1; }
    if (!rescore_file.empty()) { std::cerr << what << "compares the files as they are: --rescore is not supported with it\n"; return 1; }
    if (dedup) { std::cerr << what << "places no reads: --dedup is not supported with it\n"; return 1; }
    if (devices.size() > 1) { std::cerr << what << "runs on one device: --devices with several GPUs is not supported with it\n"; return 1; }
    if (rank_given || world > 1 || !comm_file.empty()) {
      std::cerr << what << "runs in one process: --rank / --world / --comm-file are not supported with it\n";
      return 1;
    }
    if (!placing_flags.empty() || rell_given || opt.rell_tests || opt.au || opt.kh || opt.posterior || opt.edpl || prior_given || nodes_given) {
      std::cerr << what << "places and rescores nothing: " << (placing_flags.empty() ? "the flags of --rescore" : placing_flags[0])
                << " cannot be combined with it\n";
      return 1;
    }
    std::stringstream ls(krd_list);
    std::string tok;
    while (std::getline(ls, tok, ',')) {
      if (tok.empty()) continue;
      std::string name = tok.substr(tok.find_last_of('/') == std::string::npos ? 0 : tok.find_last_of('/') + 1);
      const std::string ext = ".jplace";
      if (name.size() > ext.size() && name.compare(name.size() - ext.size(), ext.size(), ext) == 0) name.resize(name.size() - ext.size());
      for (size_t k = 0; k < krd_names.size(); ++k)
        if (krd_names[k] == name) {
          std::cerr << "--krd: " << krd_files_list[k] << " and " << tok << " both give the sample name '" << name
                    << "': a sample is named after its file, rename one of them\n";
          return 1;
        }
      krd_files_list.push_back(tok);
      krd_names.push_back(name);
    }
    if (krd_files_list.empty() || krd_files_list.size() > 4096) {
      std::cerr << "--krd: one call compares 1 .. 4096 files (" << krd_files_list.size() << " given)\n";
      return 1;
    }
  }
  if (krd_squash) {
    if (krd_files_list.size() < 2) {
      std::cerr << "--squash: clustering needs two samples at least (" << krd_files_list.size() << " file given)\n";
      return 1;
    }
    for (size_t k = 0; k < krd_names.size(); ++k)
      if (!squash_name_ok(krd_names[k])) {
        std::cerr << "--squash: the sample name '" << krd_names[k] << "' (" << krd_files_list[k] << ") holds one of ( ) , : ; [ ] ' or white "
                  << "space and would need quoting in squash.newick: rename the file\n";
        return 1;
      }
  }
  unsigned int epca_k = 0;
  if (epca_given) {
    const size_t files = krd_files_list.size();
    if (files < 2 || files > 1024) {
      std::cerr << "--epca: principal components take 2 .. 1024 samples (" << files << " given)\n";
      return 1;
    }
    char* end = nullptr;
    const long long k = std::strtoll(epca_arg.c_str(), &end, 10);
    if (epca_arg.empty() || *end || k < 1 || k > (long long)files - 1) {
      std::cerr << "--epca " << epca_arg << ": " << files << " samples have 1 .. " << files - 1 << " components\n";
      return 1;
    }
    epca_k = (unsigned int)k;
  }
  if (tree_file.empty() || ref_file.empty() || (query_file.empty() && !krd_given)) { usage(); return 1; }
  // the reference's CLI checks (src/main.cpp:165-218, 368-370)
  if (!(opt.prescoring_threshold >= 0.0 && opt.prescoring_threshold <= 1.0)) {
    std::cerr << "-g / -G: " << opt.prescoring_threshold << " not in [0, 1]\n";
    return 1;
  }
  if (!(opt.support_threshold >= 0.0 && opt.support_threshold <= 1.0)) {
    std::cerr << "--filter-acc-lwr / --filter-min-lwr: " << opt.support_threshold << " not in [0, 1]\n";
    return 1;
  }
  if (opt.filter_min > opt.filter_max) { std::cerr << "filter-min must not exceed filter-max!\n"; return 1; }
  if (opt.au && (rescore_file.empty() || opt.rell_replicates == 0)) {
    std::cerr << "--au adds p_au from multiscale replicates, N of --rell per scale, to an existing result: place first, then "
                 "--rescore out.jplace --rell N --au\n";
    return 1;
  }
  if (opt.kh && (rescore_file.empty() || opt.rell_replicates == 0)) {
    std::cerr << "--kh adds p_kh, p_wkh and p_wsh from the replicates of --rell to an existing result: place first, then "
                 "--rescore out.jplace --rell N --kh\n";
    return 1;
  }
  if (rell_given && rescore_file.empty()) {
    std::cerr << "--rell / --rell-seed work on an existing result: place first, then run again with "
                 "--rescore out.jplace --rell N\n";
    return 1;
  }
  if (rell_given && (opt.rell_replicates == 0 || opt.rell_replicates > (1u << 20))) {
    std::cerr << "--rell: the number of replicates must be 1 .. 1048576 (--rell-seed needs --rell N)\n";
    return 1;
  }
  if (opt.rell_tests && (rescore_file.empty() || opt.rell_replicates == 0)) {
    std::cerr << "--rell-tests adds elw and p_sh from the replicates of --rell and needs them: --rescore out.jplace --rell N "
                 "--rell-tests\n";
    return 1;
  }
  if ((prior_given || nodes_given) && !opt.posterior) {
    std::cerr << "--prior-mean / --posterior-nodes shape the rule of --posterior and need it: --rescore out.jplace --posterior\n";
    return 1;
  }
  if (opt.posterior && rescore_file.empty()) {
    std::cerr << "--posterior works on an existing result: place first, then run again with --rescore out.jplace --posterior\n";
    return 1;
  }
  if (prior_given && !(std::isfinite(opt.prior_mean) && opt.prior_mean > 0.0)) {
    std::cerr << "--prior-mean: the mean of the pendant prior must be positive and finite\n";
    return 1;
  }
  if (nodes_given && (opt.posterior_kx < 1 || opt.posterior_kp < 1)) {
    std::cerr << "--posterior-nodes: KX,KP with both node counts in 1 .. 64\n";
    return 1;
  }
  if (!rescore_file.empty()) {   // what --rescore does not do is refused, not silently ignored
    if (!placing_flags.empty()) {
      std::cerr << "--rescore evaluates the file's placements as they are: " << placing_flags[0]
                << " does not apply and cannot be combined with it\n";
      return 1;
    }
    if (devices.size() > 1) { std::cerr << "--rescore runs on one device: --devices with several GPUs is not supported with it\n"; return 1; }
    if (world > 1 || !comm_file.empty()) {
      std::cerr << "--rescore runs in one process: --rank / --world / --comm-file are not supported with it\n";
      return 1;
    }
  }
  // an aligned FASTQ query runs the profile chunk loop (place_profile.cpp): synchronous, one device, resident tables.
  // What that loop does not do is refused here, before any file is parsed or a device is opened
  const bool fastq = !krd_given && is_fastq_file(query_file);
  if (fastq) {
    const char* const what = "a FASTQ query (quality-aware placement) ";
    if (!rescore_file.empty()) { std::cerr << what << "is placed, not rescored: --rescore is not supported with it\n"; return 1; }
    if (devices.size() > 1) { std::cerr << what << "runs on one device: --devices with several GPUs is not supported with it\n"; return 1; }
    if (rank_given || world > 1 || !comm_file.empty()) {
      std::cerr << what << "runs in one process: --rank / --world / --comm-file are not supported with it\n";
      return 1;
    }
    if (!opt.prescoring) { std::cerr << what << "is preplaced from the lookup table: --no-heur is not supported with it\n"; return 1; }
    if (opt.memsave == Options::Memsave::kOn) {
      std::cerr << what << "is preplaced from the resident lookup table: --memsave on is not supported with it\n";
      return 1;
    }
    if (!diag_flag.empty()) { std::cerr << what << "runs its own chunk loop: " << diag_flag << " is not supported with it\n"; return 1; }
  }
  // --dedup runs a chunk loop of its own (place_dedup.cpp): synchronous, one device.  Refused in the same way
  if (dedup) {
    const char* const what = "--dedup (identical reads placed once) ";
    if (!rescore_file.empty()) { std::cerr << what << "places reads: --rescore is not supported with it\n"; return 1; }
    if (devices.size() > 1) { std::cerr << what << "runs on one device: --devices with several GPUs is not supported with it\n"; return 1; }
    if (rank_given || world > 1 || !comm_file.empty()) {
      std::cerr << what << "runs in one process: --rank / --world / --comm-file are not supported with it\n";
      return 1;
    }
    if (!opt.prescoring) { std::cerr << what << "runs the fused chunk body: --no-heur is not supported with it\n"; return 1; }
    if (fastq) { std::cerr << what << "compares coded reads: a FASTQ query is not supported with it\n"; return 1; }
    if (!diag_flag.empty() || opt.no_pipeline) {
      std::cerr << what << "runs its own chunk loop: " << (diag_flag.empty() ? "--no-pipeline" : diag_flag) << " is not supported with it\n";
      return 1;
    }
  }
  try {
    std::ifstream tf(tree_file);
    if (!tf) throw std::runtime_error{"file_check failed: " + tree_file};
    std::stringstream ss;
    ss << tf.rdbuf();
    MSA ref = read_fasta(ref_file);
    // "Peeking into MSA files and generating masks" (src/main.cpp:468-494): columns that are all-gap in
    // the reference or in the whole query file leave both alignments (unless --no-pre-mask)
    // (--krd has no query file: the reference's own gap columns are the mask)
    MSA_Info ref_info(ref), qry_info = krd_given ? MSA_Info(ref) : fastq ? fastq_msa_info(query_file) : MSA_Info::from_file(query_file);
    if (ref_info.sites() != qry_info.sites()) {
      std::cerr << "The reference and query alignment files do not seem to have the same alignment width! ("
                << ref_info.sites() << " vs. " << qry_info.sites() << "). Are the query sequences not aligned?\n";
      return 1;
    }
    MSA_Info::or_mask(ref_info, qry_info);
    if (opt.premasking && ref_info.gap_count() > 0) {
      std::cout << "Premasking: " << ref_info.gap_count() << " of " << ref_info.sites()
                << " columns are gaps in the whole reference or the whole query alignment and are removed." << std::endl;
      ref = subset_msa(ref, ref_info.gap_mask());
    }
    {  // --model may name a RAxML 8 info / RAxML-NG .bestModel / IQ-TREE report file (src/main.cpp:433-436)
      std::ifstream mf(model_desc);
      if (mf.good()) model_desc = parse_model(model_desc);
    }
    const Model model(model_desc);
    std::cout << "Using model parameters: " << model.to_string() << std::endl;
    const auto t_tree = std::chrono::steady_clock::now();
    const double secs_parse = std::chrono::duration<double>(t_tree - start).count();   // reference MSA, query-file peek, masks, model
    const Tree tree(ss.str(), ref, model, opt);
    if (tree.rooted_input())
      std::cout << "Rooted reference tree: placements are reported on the "
                << (tree.mapper() ? "rooted tree (--preserve-rooting on)." : "unrooted tree (--preserve-rooting off).")
                << std::endl;
    const double secs_tree = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_tree).count();
    if (devices.empty()) devices.push_back(device);
    const bool rank_mode = world > 1 || !comm_file.empty();   // a 1-rank communicator is legal (tests, 1-GPU nodes)
    const Run_Stats st = krd_given
        ? krd_files(tree, krd_files_list, krd_names, outdir, opt, krd_masses, krd_squash, devices[0], epca_k)
        : fastq
        ? place_profile_file(tree, query_file, qry_info, outdir, opt, invocation, devices[0])
        : dedup
        ? place_dedup_file(tree, query_file, qry_info, outdir, opt, invocation, devices[0])
        : !rescore_file.empty()
        ? rescore(tree, rescore_file, query_file, qry_info, outdir, opt, invocation, devices[0])
        : rank_mode
        ? simple_mpi_ranks(tree, query_file, qry_info, outdir, opt, invocation, device_given ? device : local_rank, rank, world, comm_file)
        : simple_mpi(tree, query_file, qry_info, outdir, opt, invocation, devices);
    if (rank_mode && rank != 0) {
      std::cout << "rank " << rank << " of " << world << ": " << st.queries << " sequences placed" << std::endl;
      return 0;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    std::cout << "Reference tree log-likelihood: " << st.ref_tree_logl << "\n";
    std::cout << st.queries << (krd_given ? " Samples done! (" : " Sequences done! (") << st.pairs
              << (krd_given ? " placements)\n" : " thorough pairs)\n")
              << "Time breakdown [s]: tree + MSA " << secs_tree << ", device setup " << st.seconds_setup
              << ", read queries " << st.seconds_read << ", wait for encoded chunk " << st.seconds_stage_wait
              << ", device " << st.seconds_place + st.seconds_thorough << ", lwr+filter " << st.seconds_post
              << ", write jplace " << st.seconds_write << "\n"
              << "Elapsed Time: " << secs << "s" << std::endl;
    if (!stats_json.empty()) {   // the same numbers, machine-readable (bench.py's cli_e2e leg)
      std::ofstream sj(stats_json);
      sj << "{\"queries\": " << st.queries << ", \"pairs\": " << st.pairs << ", \"host_threads\": " << st.host_threads
         << ", \"elapsed_s\": " << secs << ", \"tree_msa_s\": " << secs_tree << ", \"parse_inputs_s\": " << secs_parse
         << ", \"device_setup_s\": " << st.seconds_setup
         << ", \"loop_s\": " << st.seconds_loop << ", \"read_index_s\": " << st.seconds_read << ", \"encode_s\": " << st.seconds_encode
         << ", \"stage_wait_s\": " << st.seconds_stage_wait << ", \"device_calls_s\": " << st.seconds_place + st.seconds_thorough
         << ", \"build_sample_s\": " << st.seconds_sample << ", \"lwr_filter_s\": " << st.seconds_post
         << ", \"jplace_text_s\": " << st.seconds_text << ", \"write_s\": " << st.seconds_write
         << ", \"chunk_path\": \"" << st.chunk_path << "\", \"device_chunk\": " << st.device_chunk
         << ", \"lookup_mode\": \"" << st.lookup_mode << "\", \"lookup_block\": " << st.lookup_block
         << ", \"query_kind\": \"" << st.query_kind << "\"";
      if (st.dedup) sj << ", \"dedup\": {\"reads\": " << st.queries << ", \"unique\": " << st.dedup_unique << "}";
      sj << "}\n";
    }
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\nAborting with a failure." << std::endl;
    return 1;
  }
  return 0;
}
