// What every advance entry point of the device-resident beam searches shares, for the .hip files only (csrc/beam.hip, diverse.hip,
// constrain.hip, coverage.hip, phrase.hip): the plain tables with their sizes as one struct that the argument structs embed, its range and
// null checks, and the kernels' guard on the state words they size their pools by.
#pragma once
#include "beam_kernels.h"
#include "common.h"

namespace gtos_beam {

// In the order the entry points take them.  state: one row of BS_WORDS per beam (per group in the diverse search).
struct BeamTables {
    int B, k, t, V, tot, min_t, max_t;
    const float* topv;
    const int* topi;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    double* slot_score;
    int* state;
    int* bp_parent;
    int* bp_token;
    int* comp_step;
    int* comp_parent;
    double* comp_score;
    int* active;
};

// the entry points' range check (-10) of the sizes
static inline bool sizes_ok(const BeamTables& a) {
    return a.k >= 1 && a.k <= MAX_K && a.t >= 0 && a.t < a.max_t && a.V >= 1 && a.tot >= a.V;
}

// the entry points' null check (-23) of the tables
static inline bool tables_ok(const BeamTables& a) {
    return a.topv && a.topi && a.flag_shared && (a.tot <= a.V || a.flag_local) && a.slot_score && a.state && a.bp_parent && a.bp_token &&
           a.comp_step && a.comp_parent && a.comp_score && a.active;
}

// A not-done beam (or group) of `width` slots has 0 .. width live slots and fewer than width completions.  A kernel sizes its pool in
// LDS by these words and leaves a beam whose words lie outside the range alone.  No search produces such words (place_cut marks a
// beam done when it reaches width completions, and fills at most width slots), so for every state a search can reach this is a no-op.
__device__ __forceinline__ bool words_in_range(int nlive, int ncomp, int width) {
    return nlive >= 0 && nlive <= width && ncomp >= 0 && ncomp < width;
}

}  // namespace gtos_beam
