// Host entry points of the Ogden hyperelasticity kernel (hyperelastic.hip).  Like the Ramberg-Osgood kernels it lives in a
// translation unit of its own (ramberg_osgood.hpp says why: new kernels inside dxmat.hip's device module change the code
// generated for the existing ones); this header declares host functions only, so dxmat.hip's device code does not see the law.
// A custom-hardening build compiles dxmat.hip alone and never serves this law.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"

namespace dxm {

// slots of LawParams the kernel reads (filled by dxmat.hip::build_params from [alpha, mu, K]); prm.mu = mu, prm.kappa = K
constexpr int OG_A = 0;       // a = alpha / 2
constexpr int OG_AM2 = 1;     // a - 2: the one exponent that goes through exp / log per eigenvalue
constexpr int OG_MA3 = 2;     // -a / 3: det(C)^(-a/3) = J^(-alpha/3)
constexpr int OG_M = 3;       // m = a - 1: the principal stresses are mu g c_i^m + q / c_i

constexpr int OGDEN_NSLOTS = 6;   // PK2Stress (the isochoric part only), MFront vector convention

// Launch shape: one workgroup per 256 points up to 256 per CU, as for the FeFp kernels whose I/O skeleton this kernel shares
// (every tile costs the same here, but the shape is the one that kernel was measured with; unmeasured for this law)
constexpr int OGDEN_BLOCKS_PER_CU = 256;

__attribute__((visibility("hidden"))) const void* ogden_kernel_fn();

// one launch over cnt points: F (cnt, 9) -> PK1 (cnt, 9), dP/dF (cnt, 81), s1 = PK2Stress (6 slots of leading dimension ld)
__attribute__((visibility("hidden"))) void ogden_launch(int grid, hipStream_t st, const LawParams& prm, int64_t cnt, const double* F,
                                                        double* s1, int64_t ld, double* P, double* ct, BlockStats* bs);

}  // namespace dxm
