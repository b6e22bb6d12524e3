// The decode-shaped expert route's kernels and their launch body (moe_decode.h), in a translation unit of their own: the code
// objects of a step with the route off (engine.hip and the decode matmuls) hold none of them.
#define TL_MOE_DECODE_KERNELS 1
#include "moe_decode.h"
