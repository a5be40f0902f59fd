// The shape predicate of the PER-POINT FIELD, stated once (host only; defined in patch_rows.hip with the forward's entries, used by
// field_bwd.hip for the backward's).
#pragma once

namespace dpd {

// a chunk of n clouds times T queries the field gather takes (k <= 0: the window is not known to the caller)
bool field_shape_ok(int n, int T, int m, int k, int KP);

}  // namespace dpd
