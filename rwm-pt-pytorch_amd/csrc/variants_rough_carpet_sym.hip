// Instantiates the fused PT-RWM kernel for the folded RoughCarpet specialisation (modes -m, 0, +m; see targets.h).
// no stand-alone log-density kernels (ptrwm_logdensity evaluates the three-term form) and no wide object: the folded step
// kernels exist up to width 64, like every one-thread-per-replica step kernel (Makefile WIDE_VSRCS, capi.hip)
#define PTRWM_TU_NO_LOGP
#include "variants.h"

namespace ptrwm {
PTRWM_DEFINE_TARGET_VARIANTS(rough_carpet_sym_variants, RoughCarpetSym);
}  // namespace ptrwm
