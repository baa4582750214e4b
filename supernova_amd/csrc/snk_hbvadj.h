// snk_hbvadj.h -- the per-vertex From / To lists of a snk_hbv, in the order a.hbv has them (AddEdge's, graph/DigraphTemplate.h:2572-2582:
// a vertex's out-edges ascending by target vertex, equal targets in edge-id order; in-edges likewise by source vertex).  One function
// derives them (snk_hbv.hip); a.hbv, a.hbx and the branch ids of a.pathsX (the position of an edge in From(its left vertex)) all read
// the lists it made.
#pragma once
#include <stdint.h>

#include <vector>

#include "snk_ctx.h"

struct snk_hbv_lists {           // CSR: the list of vertex v is [off[v], off[v + 1])
    std::vector<uint64_t> from_off, to_off;      // [n_vertices + 1]
    std::vector<int32_t> from_v, from_e;         // per out-edge: its target vertex, its edge id
    std::vector<int32_t> to_v, to_e;             // per in-edge: its source vertex, its edge id
};
// SNK_E_ARG: an edge whose vertices lie outside [0, n_vertices); `who` names the caller in the message.  May throw std::bad_alloc.
int snk_hbv_lists_build(const snk_hbv* h, snk_hbv_lists* out, const char* who, char* err, size_t errcap);
// The 2-bit image of HBV edge e as a.hbv and a.hbx hold it (base j at bits 2 (j % 4) of byte j / 4; a reverse-complement copy is read
// backwards and complemented) -> its number of bases.  An edge of more than 2^32 - 1 bases leaves buf empty (the files hold a u32).
uint64_t snk_hbv_edge_image(const snk_hbv* h, int32_t e, const uint64_t* off, const uint8_t* bases, std::vector<uint8_t>& buf);
