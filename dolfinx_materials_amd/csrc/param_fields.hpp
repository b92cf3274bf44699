// Host entry points of the J2 kernels with per-point parameter fields (param_fields.hip), and the record of streams the kernels take.
// small_strain_field_kernel is defined beside small_strain_kernel (small_strain.hpp: one tile body for both) and, like the
// Ramberg-Osgood kernels (ramberg_osgood.hpp), instantiated in a translation unit of its own: the device modules of dxmat.hip and
// ramberg_osgood.hip compile to exactly the instruction streams they had before this form existed
// (tools/check_device_asm.py compares them).  A custom-hardening build compiles dxmat.hip alone and refuses fields.
#pragma once
#include <hip/hip_runtime.h>

#include "dxm_common.hpp"
#include "gradient.hpp"

namespace dxm {

// Per-point parameter fields (param_fields.hip): up to five SoA streams of KERNEL parameters, indexed by the point like the state
// slots (8 B-per-lane coalesced loads at gi).  A null pointer means the uniform value of LawParams.
enum { PF_LAMBDA = 0, PF_MU = 1, PF_SIG0 = 2, PF_H1 = 3, PF_H2 = 4, PF_COUNT = 5 };
struct ParamStreams { const double* p[PF_COUNT]; };

// one launch of small_strain_field_kernel<law, tl, grad_kind> (law: LAW_J2_LINEAR | LAW_J2_VOCE; tl: TL_*; grad_kind: MeshSource
// kind, 0 = strain array), with the dynamic LDS of the uniform J2 kernels.  Returns false for a law without this form.
__attribute__((visibility("hidden"))) bool param_fields_launch(int law, int tl, int grad_kind, int grid, int dyn_lds, hipStream_t st,
                                                               const LawParams& prm, const ParamStreams& pf, int64_t cnt,
                                                               const double* grad, const double* s0, double* s1, int64_t ld,
                                                               double* flux, double* ct, BlockStats* bs, const MeshSource& src);

// (lambda, mu) streams from E and nu with the expressions of dxmat.hip::build_params, every operation individually rounded;
// E_dev / nu_dev null: the uniform value E_u / nu_u.  Asynchronous on st.
__attribute__((visibility("hidden"))) void param_fields_elastic_streams(int64_t n, const double* E_dev, double E_u, const double* nu_dev,
                                                                        double nu_u, double* lambda_dev, double* mu_dev, hipStream_t st);

}  // namespace dxm
