// The 64 x 64 fp64 MFMA tile helpers of the kriging kernels (krige.hip, gpp.hip): a workgroup of 256
// threads stages two operand tiles in LDS and each wave accumulates a 32 x 32 quadrant.
#pragma once
#include "common.h"
#include "z_kernel.h"  // d4, mfma_f64

namespace hmsc {
namespace {

constexpr int KB = 64;             // tile size (dense.hip's panel size)
constexpr int KLD = KB + 1;        // padded LDS leading dimension
constexpr int KU = KB * KB / 256;  // tile elements per thread

// a 64 x 64 tile's elements M[r0 + a, c0 + b] (a = p & 63 runs along a column: coalesced), all
// loads issued before any use, at clamped (always valid) addresses; na, nb >= 1
__device__ __forceinline__ void kg_load(double (&v)[KU], const double* M, size_t ld, int r0, int c0, int na, int nb) {
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int p = threadIdx.x + 256 * u, a = p & 63, b = p >> 6;
    v[u] = M[(size_t)(r0 + min(a, na - 1)) + ld * (size_t)(c0 + min(b, nb - 1))];
  }
}

// ... into LDS, zero padded: S[a + KLD b], or transposed (TR) S[b + KLD a]; lower: entries with
// b > a are zero (a diagonal tile of a factor, whose upper triangle is scratch)
template <bool TR>
__device__ __forceinline__ void kg_store(double* S, const double (&v)[KU], int na, int nb, bool lower = false) {
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int p = threadIdx.x + 256 * u, a = p & 63, b = p >> 6;
    S[TR ? b + KLD * a : a + KLD * b] = (a < na && b < nb && !(lower && b > a)) ? v[u] : 0.0;
  }
}

// out[r][c] += sum_k SA[r + KLD k] SB[c + KLD k] over the wave's 32 x 32 quadrant, formed
// transposed so that a lane's entries are 16 consecutive rows of a column:
// acc[a][b][q] = out[qr + 16 b + lm][qc + 16 a + lk + 4 q]
__device__ __forceinline__ void kg_mma(d4 (&acc)[2][2], const double* SA, const double* SB) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lm = lane & 15, lk = lane >> 4;
  const int qr = 32 * (w & 1), qc = 32 * (w >> 1);
#pragma unroll 4
  for (int s = 0; s < KB / 4; ++s) {
    const int k = 4 * s + lk;
    const double b0 = SA[qr + lm + KLD * k], b1 = SA[qr + 16 + lm + KLD * k];
    const double a0 = SB[qc + lm + KLD * k], a1 = SB[qc + 16 + lm + KLD * k];
    acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
    acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
    acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
    acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
  }
}

__device__ __forceinline__ void kg_zero(d4 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
}

// visit the quadrant's entries: f(r, c, value)
template <class F>
__device__ __forceinline__ void kg_each(const d4 (&acc)[2][2], F f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lm = lane & 15, lk = lane >> 4;
  const int qr = 32 * (w & 1), qc = 32 * (w >> 1);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) f(qr + 16 * b + lm, qc + 16 * a + lk + 4 * q, acc[a][b][q]);
}

// the i-th new unit of a launch among the call's
__device__ __forceinline__ int kg_unit(const int* unit, int i) { return unit ? unit[i] : i; }

}  // namespace
}  // namespace hmsc
