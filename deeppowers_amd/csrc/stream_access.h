// stream_access.h - 16-byte accesses that go around the Infinity Cache (device): what the dyadic kernels (kernels_poly.h) and the baby-step stream of
// the deferred-division products (kernels_rotate.h) share.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.h"

namespace dpfhe {

// non-temporal 16-byte accesses (two 8-byte halves: the builtin takes scalars) for streams that cannot stay in the 256 MiB Infinity Cache
template <bool NT>
__device__ __forceinline__ U64x2 ld_vec(const U64x2* p) {
    if (NT) { U64x2 v; v.a = __builtin_nontemporal_load(&p->a); v.b = __builtin_nontemporal_load(&p->b); return v; }
    return *p;
}
template <bool NT>
__device__ __forceinline__ void st_vec(U64x2* p, const U64x2& v) {
    if (NT) { __builtin_nontemporal_store(v.a, &p->a); __builtin_nontemporal_store(v.b, &p->b); }
    else *p = v;
}

}  // namespace dpfhe
