// ldt_resize4_fmt.hip — the band kernel's formatted-store instantiations
// (k_resize4<SRC, KS, GEN, true>, ldt_set_output_format): the same source as
// ldt_resize4.hip, compiled here so that the two sets build side by side and
// the float32 CHW kernels stay alone in their object file.
#define LDT_RESIZE4_FMT_TU 1
#include "ldt_resize4.hip"
