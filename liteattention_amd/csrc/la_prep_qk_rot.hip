// la_prep_qk_rot.hip — the head-rotating forms of the q / k prologue (la_qk_prep_rot, la_qk_prep_fp8_rot, la_qk_prep_smooth_rot): the two
// templates of la_prep_qk.hip instantiated with HAD = true, in a code object of their own behind launch_qk_prep_rot. A separate
// translation unit so that the unrotated kernels are compiled exactly as before, the two halves build in parallel, and this half alone
// is built without packed fp32 instructions (build.py).
#define LA_QK_PREP_HADAMARD 1
#include "la_prep_qk.hip"
