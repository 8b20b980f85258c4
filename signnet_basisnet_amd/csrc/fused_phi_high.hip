// fused_phi_high.hip — the `high` product set (SN_PREC_HIGH) of the phi stage kernels: the same source as fused_phi.hip, instantiated in a
// translation unit of its own so that it compiles beside the default set (build.py compiles every .hip file in parallel).
#include "../../include/signnet_hip.h"
#define SN_PREC_TU SN_PREC_HIGH
#include "fused_phi.hip"
