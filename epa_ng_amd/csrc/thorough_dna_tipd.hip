// The TIPD instantiations of k_thorough_dna (pairs whose branch has a tip on the distal side: thorough_dna.hip,
// process_pair) and their launcher launch_dna_tipd, compiled as a translation unit of their own.
#define TH_TIPD_UNIT 1
#include "thorough_dna.hip"
