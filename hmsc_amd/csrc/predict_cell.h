// What predict.hip, summary.hip and community.hip share: the kernels' argument block, its upload
// from hmsc_predict_args, the two LDS tiles' staging and the per-cell epilogue of predict.Hmsc
// (R/predict.R:198-227).  All three kernels form L with the same fma chain in the same k order and
// hand it to predict_cell with the same cell index and counters, so for one key a cell is the
// same double in each.  The host side of the slab walks is slab_engine.h's.
#pragma once
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"
#include "rng.h"

namespace hmsc {

constexpr uint32_t S_PREDICT = 30;
constexpr int PT_I = 64, PT_J = 32, PK_MAX = HMSC_KCAP;

struct PredArgs {
  int ny, ns, nc, nr, nsamples, K, expected;
  // The rows of a launch, and their only description: [row0, row0 + ny) of a call with nyTotal rows
  // (a slab of slab_engine.h; hmsc_predict has (0, ny)).  X, the cell index and the outputs are the
  // whole call's: row0 + i against nyTotal.  Pi and the bound i < ny are the launch's own: Pi's
  // row i is the launch's row i, its leading dimension ldPi (the standalone entries point Pi at
  // row0 of the whole call's table, ldPi = nyTotal; a map lays each slab's local table, ldPi = ny).
  int row0, nyTotal, ldPi;
  int np[HMSC_MAX_LEVELS], nf[HMSC_MAX_LEVELS];
  const double* X;
  const double* Beta;    // nsamples x nc x ns
  const double* sigma;   // nsamples x ns
  const int* family;     // ns
  const double* yscale;  // 2 x ns
  const int* Pi;         // ny x nr (leading dimension ldPi), 0-based
  const double* Eta[HMSC_MAX_LEVELS];     // nsamples x np x nf
  const double* Lambda[HMSC_MAX_LEVELS];  // nsamples x nf x ns
  double* out;           // nsamples x ny x ns
  Key key;
};

// Poisson(lam) by PTRS (Hormann 1993, the transformed rejection numpy uses) for lam >= 10,
// sequential inversion below; uniforms from the cell's own counters
__device__ inline double rpois_dev(double lam, Key key, uint32_t cell, uint32_t s) {
  if (!(lam < INFINITY)) return NAN;  // NaN or +inf: R's rpois gives NaN (with a warning)
  if (!(lam > 0.0)) return 0.0;
  if (lam < 10.0) {
    const double u = uniforms(key, cell, 1, S_PREDICT, s).a;
    double p = exp(-lam), c = p;
    int k = 0;
    while (u > c && k < 1000) {
      ++k;
      p *= lam / k;
      c += p;
    }
    return (double)k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (uint32_t t = 0; t < 256; ++t) {
    const Uniform2 uv = uniforms(key, cell, 1 + t, S_PREDICT, s);
    const double U = uv.a - 0.5, V = uv.b;
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
  }
  return floor(lam);  // not reached in practice (acceptance ~0.9 per trial)
}

// The value of cell (i, j) of sample s from its linear predictor L: expected value or draw by
// family, then the YScalePar back-transform.  cell = i + ny j (pred_cell_index).
// sg = sigma[s, j], fam = family[j], (m, sd) = YScalePar[, j].
__device__ __forceinline__ double predict_cell(const PredArgs& a, double L, double sg, int fam, double m, double sd,
                                               uint32_t cell, int s) {
  double z;
  if (a.expected) {
    z = fam == 2 ? 0.5 * erfc_fast(-L * 0.7071067811865476) : fam == 3 ? exp(L + 0.5 * sg) : L;
  } else {
    z = fma(sqrt(sg), normal(a.key, cell, 0, S_PREDICT, (uint32_t)s), L);
    if (fam == 2) z = z > 0.0 ? 1.0 : 0.0;
    if (fam == 3) z = rpois_dev(exp(z), a.key, cell, (uint32_t)s);
  }
  if (m != 0.0 || sd != 1.0) z = fma(z, sd, m);
  return z;
}

// the cell index of row i (of the launch) and species j: (row0 + i) + nyTotal j, which is also the
// cell's place in a ny x ns column-major output of the whole call
__device__ __forceinline__ size_t pred_cell_index(const PredArgs& a, int i, int j) {
  return (size_t)(a.row0 + i) + (size_t)a.nyTotal * j;
}

// sA[site][k] (row stride LD = K | 1) for k in [k0, K) of the 64 sites from i0, sample s: the X
// columns, then each level's Eta rows of the sites' units.  sPi (may be null): the tile's units
// [level][site] in LDS, else they are read from a.Pi.
__device__ __forceinline__ void stage_sites(const PredArgs& a, double* sA, int LD, int i0, int s, int k0, int t,
                                            const int* sPi = nullptr) {
  const int ny = a.ny, nc = a.nc;
  for (int p = t + k0 * PT_I; p < PT_I * a.K; p += 256) {
    const int ii = p % PT_I, k = p / PT_I, i = i0 + ii;
    double v = 0.0;
    if (i < ny) {
      if (k < nc) {
        v = a.X[(size_t)(a.row0 + i) + (size_t)a.nyTotal * k];
      } else {
        int kk = k - nc, r = 0;
        while (kk >= a.nf[r]) kk -= a.nf[r++];
        const int u = sPi ? sPi[r * PT_I + ii] : a.Pi[i + (size_t)a.ldPi * r];
        v = a.Eta[r][(size_t)s * a.np[r] * a.nf[r] + u + (size_t)a.np[r] * kk];
      }
    }
    sA[ii * LD + k] = v;
  }
}

// sB[k][species] of the 32 species from j0, sample s: [Beta_s; Lambda_1,s; ...]
__device__ __forceinline__ void stage_species(const PredArgs& a, double* sB, int j0, int s, int t) {
  const int ns = a.ns, nc = a.nc;
  for (int p = t; p < a.K * PT_J; p += 256) {
    const int k = p / PT_J, jj = p % PT_J, j = j0 + jj;
    double v = 0.0;
    if (j < ns) {
      if (k < nc) {
        v = a.Beta[(size_t)s * nc * ns + k + (size_t)nc * j];
      } else {
        int kk = k - nc, r = 0;
        while (kk >= a.nf[r]) kk -= a.nf[r++];
        v = a.Lambda[r][(size_t)s * a.nf[r] * ns + kk + (size_t)a.nf[r] * j];
      }
    }
    sB[k * PT_J + jj] = v;
  }
}

// acc[q] = L of (site ii, species jb + 4 q): one fma chain per cell over k = 0 .. K - 1
__device__ __forceinline__ void linear_predictor(const double* sA, const double* sB, int LD, int K, int ii, int jb,
                                                 double acc[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.0;
  for (int k = 0; k < K; ++k) {
    const double x = sA[ii * LD + k];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = fma(x, sB[k * PT_J + jb + 4 * q], acc[q]);
  }
}

// The checks and uploads of hmsc_predict_args that every predict launch needs (all but `out`).
// pi0 is the source of a copy on the stream: the caller declares it before the owner.
inline PredArgs upload_pred_args(const hmsc_predict_args* p, DeviceOwner& own, hipStream_t st, std::vector<int>& pi0) {
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns, nc = p->nc;
  int K = p->nc;
  for (int r = 0; r < p->nr; ++r) K += p->nf[r];
  pi0.assign((size_t)ny * std::max(1, p->nr), 0);
  PredArgs a{};
  a.ny = p->ny;
  a.ns = p->ns;
  a.nc = p->nc;
  a.nr = p->nr;
  a.nsamples = p->nsamples;
  a.K = K;
  a.expected = p->expected;
  a.row0 = 0;
  a.nyTotal = a.ldPi = p->ny;
  a.X = own.upload(p->X, ny * nc, st);
  a.Beta = own.upload(p->Beta, S * nc * ns, st);
  a.sigma = own.upload(p->sigma, S * ns, st);
  a.family = own.upload(p->family, ns, st);
  a.yscale = own.upload(p->YScalePar, 2 * ns, st);
  for (int r = 0; r < p->nr; ++r) {
    a.np[r] = p->np[r];
    a.nf[r] = p->nf[r];
    for (size_t i = 0; i < ny; ++i) {
      const int u = p->Pi[i + ny * r] - 1;
      HMSC_REQUIRE(u >= 0 && u < p->np[r], "predict: Pi out of range");
      pi0[i + ny * r] = u;
    }
    a.Eta[r] = own.upload(p->Eta[r], S * p->np[r] * p->nf[r], st);
    a.Lambda[r] = own.upload(p->Lambda[r], S * p->nf[r] * ns, st);
  }
  a.Pi = own.upload(pi0.data(), pi0.size(), st);
  a.key = Key{(uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
  return a;
}

// the limits every predict launch keeps; K = nc + sum nf
inline int check_pred_limits(const hmsc_predict_args* p) {
  HMSC_REQUIRE(p->nr >= 0 && p->nr <= HMSC_MAX_LEVELS, "predict: bad nr");
  int K = p->nc;
  for (int r = 0; r < p->nr; ++r) K += p->nf[r];
  HMSC_REQUIRE(K <= PK_MAX, "predict: nc + sum(nf) must be <= 128");
  HMSC_REQUIRE((size_t)p->ny * p->ns < ((size_t)1 << 32), "predict: ny * ns must fit 32-bit cell counters");
  return K;
}

inline size_t pred_lds_bytes(int K) { return ((size_t)PT_I * (K | 1) + (size_t)K * PT_J) * sizeof(double); }

}  // namespace hmsc
