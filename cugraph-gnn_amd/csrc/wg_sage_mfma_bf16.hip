// The one-kernel SAGE layer (wg_sage_mfma.hip) over a bfloat16 feature table: the same kernel template with 8-byte row loads,
// instantiated here so that it compiles next to the float32 kernels.
#define WG_SAGE_X16_TYPE __bf16
#define WG_SAGE_X16_LAUNCH launch_bf16
#include "wg_sage_mfma.hip"
