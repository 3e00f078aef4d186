// cornell_moe_amd/csrc/chebei1.hpp -- what chebei1.hip (the Chebyshev-scalarised expected improvement) lends to logchebei1.hip (its
// log form with constraints): the constants of the fixed quadrature and the two operations that are rounded by themselves.  Device
// code only; every unit that includes it compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace moe {

namespace {

constexpr int kChebBreaks = 14;  // breakpoints per objective

__constant__ double kChebC[kChebBreaks] = {-38.0, -8.0, -6.0, -4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0};
// the 8-point Gauss-Legendre rule on [-1, 1]
__constant__ double kChebX[8] = {-0x1.ebab1cb0acc67p-1, -0x1.97e4ab249f41ep-1, -0x1.0d129583284b4p-1, -0x1.77ac94f3c7345p-3,
                                 0x1.77ac94f3c7345p-3,  0x1.0d129583284b4p-1,  0x1.97e4ab249f41ep-1,  0x1.ebab1cb0acc67p-1};
__constant__ double kChebW[8] = {0x1.9ea1d04ca0374p-4, 0x1.c76fb531d2b96p-3, 0x1.413c50a255615p-2, 0x1.736360b199343p-2,
                                 0x1.736360b199343p-2, 0x1.413c50a255615p-2, 0x1.c76fb531d2b96p-3, 0x1.9ea1d04ca0374p-4};

// a product and a sum that are rounded by themselves wherever they are inlined (never fused with a neighbour)
__device__ __forceinline__ double rmul(double x, double y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ double radd(double x, double y) {
#pragma clang fp contract(off)
  return x + y;
}

}  // namespace

}  // namespace moe
