// k_thorough_dna<2, .., TAILH, .., TDPP, TIPD> alone (see thorough_dna.hip, TH_TIPD_UNIT): built with the default
// scheduler, under which this compiler's register allocator does not crash on it.
#define TH_TIPD_UNIT 2
#include "thorough_dna.hip"
