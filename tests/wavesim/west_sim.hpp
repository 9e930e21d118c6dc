// TEST INFRASTRUCTURE (not product code): what csrc/tmpc_west.hip needs of the HIP dialect beyond hip_sim.hpp.  The fibers of the
// execution model are cooperative (a lane runs until its next rendezvous), so an atomic is a plain read-modify-write.
#pragma once
#include "hip_sim.hpp"

inline unsigned atomicAdd(unsigned *p, unsigned v) { const unsigned o = *p; *p = o + v; return o; }
inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; if (v < o) *p = v; return o; }
inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }
