// The slab engine: the host side that hmsc_predict_summary (summary.hip), hmsc_predict_community
// (community.hip) and hmsc_predict_map (map.hip) share.  A call's ny rows are walked in slabs of
// whole 64-row tiles; a slab is one launch whose PredArgs::{row0, ny, nyTotal} name its rows
// (predict_cell.h).  Per slab a value kernel writes the slab's samples to a scratch slab and a
// statistics kernel reduces them into whole-call outputs at row0, so no result depends on the slab
// size.  Here: the two block descriptors (they are the kernels' arguments as they stand), their
// argument checks, the slab planner, the allocation of outputs and slab, and the copy back.  The
// kernels and their launches stay beside their contracts in summary.hip and community.hip.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "predict_cell.h"

namespace hmsc {

constexpr int NQ_MAX = 8, NW_MAX = 16, NPAIR_MAX = 8;
constexpr uint64_t SCRATCH_DEFAULT = (uint64_t)1 << 30;
constexpr uint64_t BLOCKS_MAX = (uint64_t)1 << 23;  // workgroups of one launch of community kernel A

// per-cell summaries: mean, occ, n of every cell, quantiles of the flagged columns.  (What the
// summary kernel reads comes first and together: with probs between them it spilled to scratch.)
struct CellBlock {
  int nslot, nq;        // flagged columns, probabilities
  const int* slot;      // ns: a flagged column's slot 0 .. nslot - 1, else -1
  double* slab;         // nsamples x nslot x (rows of the largest slab), null without flagged columns
  double* mean;         // nyTotal x ns
  double* occ;          // nyTotal x ns
  int* n;               // nyTotal x ns
  const int* cols;      // nslot: the species column of a slot
  double* quant;        // nq x nyTotal x ns
  double probs[NQ_MAX];
};

// community columns of one transform: n, mean and quantiles per (row, column)
struct CommunityBlock {
  int nw, transform, nq;
  int nslots;           // 2 x site pairs (the standalone entry's; 0 on maps)
  double probs[NQ_MAX];
  int normalise[NW_MAX];
  int pair_site[2 * NPAIR_MAX];  // rows of the whole call
  const double* W;      // ns x nw
  double* slab;         // nsamples x nw x (rows of the largest slab)
  int* n;               // nyTotal x nw
  double* mean;         // nyTotal x nw
  double* quant;        // nq x nyTotal x nw
  double* comm;         // nsamples x (nyTotal x nw), or null
  double* pairbuf;      // nsamples x nw x nslots, or null
};

// one slab, queued on st: the samples' values into g.slab, then their statistics into the outputs
void launch_values(hipStream_t st, const PredArgs& a, const CellBlock& g);  // summary.hip
void launch_statistics(hipStream_t st, const PredArgs& a, const CellBlock& g);
void launch_values(hipStream_t st, const PredArgs& a, const CommunityBlock& g);  // community.hip
void launch_statistics(hipStream_t st, const PredArgs& a, const CommunityBlock& g);

// name: the entry, the prefix of every message.  The checks keep the order each entry had.
inline void check_nq(const std::string& name, int nq) {
  HMSC_REQUIRE(nq >= 0 && nq <= NQ_MAX, name + ": at most 8 probabilities (nq = " + std::to_string(nq) + ")");
}
inline void take_probs(const std::string& name, int nq, const double* probs, double out[NQ_MAX]) {
  for (int k = 0; k < nq; ++k) {
    HMSC_REQUIRE(probs[k] >= 0.0 && probs[k] <= 1.0, name + ": every probability must lie in [0, 1]");
    out[k] = probs[k];
  }
}

// g's host part, and the slot of every column / the column of every slot (sources of alloc's uploads)
inline void check_cells(const std::string& name, const hmsc_summary_args* q, size_t ns, const double* quant, CellBlock& g,
                        std::vector<int>& slot, std::vector<int>& cols) {
  g = CellBlock{};
  g.nq = q ? q->nq : 0;
  check_nq(name, g.nq);
  HMSC_REQUIRE(g.nq == 0 || (q->probs != nullptr && q->qcols != nullptr && quant != nullptr),
               name + ": nq > 0 needs probs, qcols and quant");
  if (g.nq > 0) take_probs(name, g.nq, q->probs, g.probs);
  slot.assign(ns, -1);
  if (g.nq > 0)
    for (size_t j = 0; j < ns; ++j)
      if (q->qcols[j]) slot[j] = (int)cols.size(), cols.push_back((int)j);
  g.nslot = (int)cols.size();
}

// map: a block of hmsc_predict_map (no site pairs; its n and mean are checked here), else
// hmsc_predict_community's (pairs into pr)
inline void check_community(const std::string& name, const hmsc_community_args* c, int ny, bool map, const int32_t* n,
                            const double* mean, const double* quant, const double* pr, CommunityBlock& g) {
  g = CommunityBlock{};
  const int npairs = c->npairs;
  HMSC_REQUIRE(c->nw >= 1 && c->nw <= NW_MAX, name + ": nw must lie in 1 .. 16 (nw = " + std::to_string(c->nw) + ")");
  HMSC_REQUIRE(c->W != nullptr && c->normalise != nullptr, name + ": W and normalise must not be NULL");
  check_nq(name, c->nq);
  if (map) {
    HMSC_REQUIRE(npairs == 0, name + ": site contrasts (pairs) are not served on maps");
    HMSC_REQUIRE(n != nullptr && mean != nullptr, name + ": a community block needs n and mean");
  }
  HMSC_REQUIRE(c->nq == 0 || (c->probs != nullptr && quant != nullptr), name + ": nq > 0 needs probs and quant");
  HMSC_REQUIRE(npairs >= 0 && npairs <= NPAIR_MAX, name + ": at most 8 site pairs (npairs = " + std::to_string(npairs) + ")");
  HMSC_REQUIRE(npairs == 0 || (c->pairs != nullptr && pr != nullptr), name + ": npairs > 0 needs pairs and pr");
  g.nw = c->nw, g.transform = c->transform ? 1 : 0, g.nq = c->nq, g.nslots = 2 * npairs;
  take_probs(name, c->nq, c->probs, g.probs);
  for (int k = 0; k < 2 * npairs; ++k) {
    HMSC_REQUIRE(c->pairs[k] >= 0 && c->pairs[k] < ny,
                 name + ": pair index " + std::to_string(c->pairs[k]) + " outside 0 .. ny - 1");
    g.pair_site[k] = c->pairs[k];
  }
  for (int m = 0; m < g.nw; ++m) g.normalise[m] = c->normalise[m] ? 1 : 0;
}

// The rows of a slab: slab_rows as given; else the whole 64-row tiles whose ncol slab columns of
// nsamples doubles per row fit scratch_bytes (0: 1 GiB), all ny rows when there is no column.  cap
// (a community block may be in the call): at most 2^23 workgroups, (tile, sample) each; the caller
// refuses more than 2^23 samples, where its order of refusals has that.  At most ny.
inline size_t plan_slab_rows(const std::string& name, const char* of, size_t ny, size_t S, size_t ncol, size_t slab_rows,
                             uint64_t scratch_bytes, bool cap) {
  if (slab_rows == 0 && ncol > 0) {
    const uint64_t budget = scratch_bytes ? scratch_bytes : SCRATCH_DEFAULT;
    const uint64_t tile_bytes = (uint64_t)S * PT_I * ncol * 8;
    HMSC_REQUIRE(tile_bytes <= budget, name + ": one 64-row tile" + of + " needs " + std::to_string(tile_bytes) +
                                           " bytes of scratch, scratch_bytes allows " + std::to_string(budget));
    slab_rows = (size_t)(budget / tile_bytes) * PT_I;
  }
  if (slab_rows == 0) slab_rows = ny;
  if (cap) slab_rows = std::min(slab_rows, (size_t)(BLOCKS_MAX / S) * PT_I);
  return std::min(slab_rows, ny);
}

// the outputs (a.nyTotal rows), the slab, NaN on the quantile planes; the uploads are queued on st
inline void alloc(DeviceOwner& own, hipStream_t st, const PredArgs& a, size_t slab_rows, const std::vector<int>& slot,
                  const std::vector<int>& cols, CellBlock& g) {
  const size_t cells = (size_t)a.nyTotal * a.ns;
  g.slot = own.upload(slot.data(), slot.size(), st);
  g.mean = own.alloc<double>(cells);
  g.occ = own.alloc<double>(cells);
  g.n = own.alloc<int>(cells);
  if (g.nq > 0) {
    g.quant = own.alloc<double>(g.nq * cells);
    HIP_OK(hipMemsetAsync(g.quant, 0xFF, g.nq * cells * 8, st));  // NaN off the flagged columns
  }
  if (g.nslot > 0) {
    g.slab = own.alloc<double>((size_t)a.nsamples * g.nslot * slab_rows);
    g.cols = own.upload(cols.data(), cols.size(), st);
  }
}

inline void alloc(DeviceOwner& own, hipStream_t st, const PredArgs& a, size_t slab_rows, const double* W, bool comm,
                  CommunityBlock& g) {
  const size_t S = a.nsamples, cells = (size_t)a.nyTotal * g.nw;
  g.W = own.upload(W, (size_t)a.ns * g.nw, st);
  g.slab = own.alloc<double>(S * g.nw * slab_rows);
  g.n = own.alloc<int>(cells);
  g.mean = own.alloc<double>(cells);
  if (g.nq > 0) g.quant = own.alloc<double>(g.nq * cells);
  if (comm) g.comm = own.alloc<double>(S * cells);
  if (g.nslots > 0) g.pairbuf = own.alloc<double>(S * g.nw * g.nslots);
}

// queued on st; the caller waits
inline void copy_out(hipStream_t st, const PredArgs& a, const CellBlock& g, double* mean, double* occ, int32_t* n,
                     double* quant) {
  const size_t cells = (size_t)a.nyTotal * a.ns;
  HIP_OK(hipMemcpyAsync(mean, g.mean, cells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(occ, g.occ, cells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(n, g.n, cells * 4, hipMemcpyDeviceToHost, st));
  if (g.nq > 0) HIP_OK(hipMemcpyAsync(quant, g.quant, g.nq * cells * 8, hipMemcpyDeviceToHost, st));
}

inline void copy_out(hipStream_t st, const PredArgs& a, const CommunityBlock& g, int32_t* n, double* mean, double* quant) {
  const size_t cells = (size_t)a.nyTotal * g.nw;
  HIP_OK(hipMemcpyAsync(n, g.n, cells * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(mean, g.mean, cells * 8, hipMemcpyDeviceToHost, st));
  if (g.nq > 0) HIP_OK(hipMemcpyAsync(quant, g.quant, g.nq * cells * 8, hipMemcpyDeviceToHost, st));
}

// f's work on st, waited for, charged to ms
template <class F>
void timed(hipStream_t st, double& ms, F&& f) {
  const auto t0 = std::chrono::steady_clock::now();
  f();
  HIP_OK(hipStreamSynchronize(st));
  ms += ms_since(t0);
}

// The standalone entries' walk: a holds the whole call (upload_pred_args: every row's Pi, leading
// dimension nyTotal); per slab the value kernel, then the statistics kernel.
template <class Block>
void run_slabs(hipStream_t st, PredArgs a, size_t slab_rows, const Block& g, double& values_ms, double& statistics_ms) {
  const size_t ny = a.nyTotal;
  const int* Pi = a.Pi;
  for (size_t row0 = 0; row0 < ny; row0 += slab_rows) {
    a.row0 = (int)row0, a.ny = (int)std::min(slab_rows, ny - row0), a.Pi = Pi + row0;
    timed(st, values_ms, [&] { launch_values(st, a, g); });
    timed(st, statistics_ms, [&] { launch_statistics(st, a, g); });
  }
}

}  // namespace hmsc
