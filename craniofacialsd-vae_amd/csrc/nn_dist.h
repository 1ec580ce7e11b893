// The one squared distance of the nearest-neighbour searches (chamfer.hip:
// brute force; nn_grid.hip: uniform grid).  Both searches must return the
// same BITS for the same (query, reference) pair, so both evaluate it here.
#pragma once
#include "cfsd_common.h"

namespace cfsd {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Difference form (q - r)^2 summed over x, y, z with one fixed rounding
// sequence -- sub, sub, sub, mul, fma, fma, contraction pinned off -- wherever
// a pair is evaluated.  V = f32x2: two queries ride in the halves of packed
// fp32 operands against one reference point (the brute-force walk); V = float:
// one query against one point (the grid walk).  The packed instructions round
// each half exactly as the scalar ones do, so the two instantiations agree
// bit for bit.
template <typename V>
__device__ __forceinline__ V nn_dist(V qx, V qy, V qz, float rx, float ry, float rz) {
#pragma clang fp contract(off)
  const V dx = qx - rx, dy = qy - ry, dz = qz - rz;
  return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}

}  // namespace cfsd
