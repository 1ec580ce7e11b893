// Run-time -> compile-time selection for the host dispatch of the conv kernels.
// A kernel family names the shapes it instantiates in one ShapeList (or
// IntList); for_shape / for_value call a generic lambda with the entry that
// matches the run-time value, as a type, so every launch is an ordinary
// templated function:
//
//   using MfmaShapes = ShapeList<Shape<32, 32>, Shape<32, 64>>;
//   int rc = for_shape(MfmaShapes{}, cin, cout, [&](auto s) {
//     using S = decltype(s);
//     return launch_foo<S::cin, S::cout>(args...);
//   });
//   if (rc != kNoShape) return rc;
//
// Only the listed entries are instantiated: a list is exactly the set of
// kernels its family puts into the library.
#pragma once
#include <limits.h>

#include "cfsd_common.h"

namespace cfsd {

// "no entry of the list matched" (never a CFSD_* code or a hipError_t)
constexpr int kNoShape = INT_MIN;

template <int CIN, int COUT>
struct Shape {
  static constexpr int cin = CIN, cout = COUT;
};
template <typename... S>
struct ShapeList {};

template <int V>
struct Int {
  static constexpr int value = V;
};
template <int... V>
struct IntList {};

template <typename T>
struct Type {
  using type = T;
};

template <typename... S, typename F>
int for_shape(ShapeList<S...>, int cin, int cout, F&& f) {
  int rc = kNoShape;
  (void)((cin == S::cin && cout == S::cout && (rc = f(S{}), true)) || ...);
  return rc;
}

template <int... V, typename F>
int for_value(IntList<V...>, int v, F&& f) {
  int rc = kNoShape;
  (void)((v == V && (rc = f(Int<V>{}), true)) || ...);
  return rc;
}

using Acts = IntList<CFSD_ACT_ELU, CFSD_ACT_NONE>;

// Storage type of an operand: bf16_t for CFSD_DT_BF16, float otherwise (the
// caller has validated dt).
template <typename F>
int for_storage(int dt, F&& f) {
  return CFSD_DT_TYPE(dt) == CFSD_DT_BF16 ? f(Type<bf16_t>{}) : f(Type<float>{});
}

}  // namespace cfsd
