// parse_solo.hip — the solo / spread parse kernels (k_parse_solo, one image's
// substreams on scalar engines; parse_lanes.hip) as a translation unit of
// their own, so that the lanes kernels and these get the code-generation
// flags each is fastest with (Makefile PARSE_SCHED / SOLO_SCHED; A/B in
// DESIGN 5.11).
#define HG_PARSE_TU 2
// (the lanes units' cold-branch hints stay out of the scalar engines: their code is the one before the
// lean body, instruction for instruction)
#define HG_NO_COLD_HINTS 1
#include "parse_lanes.hip"
