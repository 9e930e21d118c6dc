// The fused closed loop through the explicit law (closed_loop_law: solve_body<..., FUSED = 3>, tmpc_kernels.hip) as a translation
// unit of its own, like tmpc_fused.hip.
#define TMPC_FUSED_TU 3
#include "tmpc_kernels.hip"
