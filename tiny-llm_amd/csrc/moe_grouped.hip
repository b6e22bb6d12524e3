// The grouped-expert route's kernels and their launch body (moe_grouped.h), in a translation unit of their own: the decode step's
// code objects (engine.hip and the decode matmuls) hold none of them.
#define TL_MOE_GROUPED_KERNELS 1
#include "moe_grouped.h"
