// fused_phi_medium.hip — the `medium` product set (SN_PREC_MEDIUM) of the phi stage kernels: the same source as fused_phi.hip, instantiated in a
// translation unit of its own so that it compiles beside the default set (build.py compiles every .hip file in parallel).
#include "../../include/signnet_hip.h"
#define SN_PREC_TU SN_PREC_MEDIUM
#include "fused_phi.hip"
