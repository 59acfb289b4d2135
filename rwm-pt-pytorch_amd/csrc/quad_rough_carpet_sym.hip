// Instantiates the lane-split (quad) PT-RWM kernel for the folded RoughCarpet target (all proposals, all lane widths).
// no state_f64 twins: such runs take the two-term kernels (variants.h PTRWM_TU_NO_F64, capi.hip)
#define PTRWM_TU_NO_F64
#include "variants.h"

namespace ptrwm {
PTRWM_DEFINE_QUAD_VARIANTS(rough_carpet_sym_variants, QRoughCarpetSym);
}  // namespace ptrwm
