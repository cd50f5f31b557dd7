// parse_lean.hip — the lean lanes parse kernel (k_parse_lean: parse_lanes.hip's
// lanes body compiled for the 4:2:0 tool set without PCM, transform_skip,
// cu_transquant_bypass and in-picture slice segments, EngT) as a translation
// unit of its own, with its own code-generation flags (Makefile LEAN_FLAGS; the
// general unit's SLP threshold costs this body 32 VGPRs).
#define HG_PARSE_TU 3
#include "parse_lanes.hip"
