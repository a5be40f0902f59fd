// The shape predicates of the PER-POINT FIELD, stated once (host only; the forward's is defined in patch_rows.hip with its entries, the
// backward's in field_bwd.hip; field_train.hip uses both and the routes behind the decoder chain).
#pragma once
#include <cstdint>

#include "../../include/dpdist_capi.h"

namespace dpd {

// a chunk of n clouds times T queries the field gather takes (k <= 0: the window is not known to the caller)
bool field_shape_ok(int n, int T, int m, int k, int KP);

// the predicate of the slot-summed backward (field_bwd.hip) -> the slot capacity, 0 = refused (k <= 0 / H <= 0: not known to the caller)
int field_bwd_cap(int n, int T, int m, int k, int KP, int H);

// what dpd_field_bwd does behind the decoder chain, on checked arguments (field_bwd.hip): slot sum + query route, slot product + window
// scatter (dfv != NULL), the chain of a shared query set; keep_gs: form gs without a surface gradient as well
int field_routes(const float* g1, const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist,
                 const int32_t* slot_vox, const int32_t* slot_cloud, int n, int T, int m, int k, int KP, int H, int cap,
                 const dpd_decoder_params* p, float* dq, float* gs, float* dXs, float* dfv, int accumulate, float* gq, long gq_cloud_stride,
                 bool keep_gs, void* stream);

}  // namespace dpd
