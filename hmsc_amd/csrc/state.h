// Device-resident state of one Hmsc chain (or one species shard of a chain).
//
// HBM layout (all fp64 column-major like R unless noted):
//   Z        ny x ns_loc          latent responses (the only large mutable array)
//   Ycode    ny x ns_loc  int8    0 / 1 / -1(NA)           (probit cells)
//   Yval     ny x ns_loc          YScaled (only if non-probit species exist)
//   X        ny x nc              XScaled
//   BL       K x ns_loc           [Beta; Lambda_1; ...; Lambda_nr]   (K = nc + sum nf_r)
//   Psi      NF x ns_loc          [Psi_1; ...; Psi_nr]               (NF = sum nf_r)
//   Delta    NF                   [Delta_1; ...]
//   Eta_r    np_r x nf_r          per level, column-major
// Live K/NF change only through updateNf (transient), which repacks on the host;
// buffers are allocated at nfMax so no reallocation ever happens.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "devmem.h"
#include "rng.h"

namespace hmsc {

constexpr int SEL_MAX = 8;       // ncsel (hmsc_model): selections of covariates per chain

struct Level {
  int np = 0, nf = 0, nfmax = 0, nfmin = 0;
  // factors this level's buffers hold: min(nfMax, K cap - nc) -- Eta storage, record slots;
  // and the factors its spatial workspace is laid out for now (grown with nf, spatial.hip)
  int nfcap = 0, nf_alloc = 0;
  double nu = 3, a1 = 50, b1 = 1, a2 = 50, b2 = 1;
  double* Eta = nullptr;        // np x nfmax storage, live np x nf (ld = np)
  int* Pi = nullptr;            // ny, 0-based unit of each row
  int* unit_ptr = nullptr;      // np+1 CSR over rows of each unit
  int* unit_rows = nullptr;     // ny
  int* Alpha = nullptr;         // nfmax (host mirror in State::h_alpha)
  int uniform_n = 0;            // common row count of every unit (0 if they differ)
  // spatial "Full" level (spatial.hip): alphapw grid of R/computeDataParameters.R:53-81
  bool spatial = false;
  int nalpha = 0;
  double* alphapw = nullptr;    // nalpha x 2
  double* iWg = nullptr;        // np x np x nalpha
  double* RiWg = nullptr;       // np x np x nalpha (upper triangular; lower for NNGP / GPP)
  int riw_lower = 0;            // RiWg lower: NNGP's Vecchia factor, GPP's / the device-built Full grid's chol(W)^-1
  double* detWg = nullptr;      // nalpha
  double* AlphaD = nullptr;     // nfmax: 1-based grid index of each factor (recorded)
  double* spWork = nullptr;     // dense (np nf)^2 Eta system + Alpha likelihoods
  // 'GPP' level in R's low-rank form (spatial.hip, R/computeDataParameters.R:138-194)
  bool gpp = false;
  int nK = 0;
  double* idDg = nullptr;       // np x nalpha
  double* idDW12g = nullptr;    // np x nK x nalpha
  double* Fg = nullptr;         // nK x nK x nalpha
  double* iFg = nullptr;        // nK x nK x nalpha
  // 'NNGP' level in the sparse Vecchia form (spatial.hip, R/computeDataParameters.R:82-136):
  // RiW_g = D_g^-1/2 (I - A_g), A_g[i, nb(i, k)] over the nnK nearest earlier units
  bool nngp = false;
  int nnK = 0;                  // neighbours per unit (rL$nNeighbours)
  int* nnIdx = nullptr;         // nnK x np: earlier neighbours of unit i (ascending), -1 padded
  double* nnA = nullptr;        // nalpha x nnK x np: Vecchia coefficients A_g[i, nb(i, k)]
  double* nnD = nullptr;        // nalpha x np: conditional variances D_g[i]
  int* nnPerm = nullptr;        // np: unit at each position of the factorization order (RCM)
  int* nnPos = nullptr;         // np: position of each unit
  int* nnChPtr = nullptr;       // np + 1: CSR of the rows whose support {i} + nb(i) holds the unit
  int* nnCh = nullptr;          // entries i (nnK + 1) + slot, slot 0 = the unit itself (B = 1), ascending i
  int nnBwUnits = 0;            // bandwidth of the precision in units (RCM order)
  int nnAssembledN = 0;         // size of the last assembled system (its band layout zeroed for it)
  // covariate-dependent level (hmsc_model etaShare / xScale): the level whose units and Eta
  // this one shares (eta_owner < this index: Eta aliases the owner's buffer), the covariate
  // column scaling its XEta columns (np, unit order), and -- on the owner -- the levels of
  // its group (xgroup consecutive levels from it)
  int eta_owner = -1;
  double* xs = nullptr;
  int xgroup = 1;
  bool eta_alias() const { return eta_owner >= 0; }
};

struct State {
  // dims
  int ny = 0, ns = 0, nc = 0, nt = 0, nr = 0;
  int sp0 = 0, nsl = 0;          // species shard [sp0, sp0+nsl)
  int rank = 0, nranks = 1;
  int device = 0;
  uint32_t mask = HMSC_UP_ALL;
  Key key{0, 0};
  int noise_mode = 0;
  bool has_na = false;           // any NA in the local Y
  bool any_normal = false;       // any family==1 species (local)
  bool any_var = false;          // any species with estimated variance (distr[,2]==1)
  bool any_poisson = false;
  bool any_xs = false;           // a covariate-dependent level (Level::xs): general updateEta path
  bool all_probit = true;
  bool isigma_fixed_one = true;  // all probit and iSigma never set from outside: iSigma == 1
  int K = 0, NF = 0, Kmax = 0, NFmax = 0;
  double f0 = 0;
  Level lev[HMSC_MAX_LEVELS];

  // every device buffer, pinned buffer, stream and event of the chain: the pointer and handle
  // fields below (and Level's) are views of what it holds, released by free_state (capi.cpp)
  DeviceOwner own;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  // side stream: updateGammaV, Gamma2's iV-only algebra and updateLambdaPriors of sweep t
  // only feed sweep t+1, so they overlap updateEta / updateZ of sweep t
  hipStream_t side = nullptr, side2 = nullptr;  // side: GammaV + Gamma2 prep; side2: LambdaPriors
  // a captured recorded sweep asks updateZ's slab-sum launch to carry the record pack (part 1)
  bool pack_req = false, pack_done = false;
  hipEvent_t ev_bl = nullptr, ev_side = nullptr, ev_side2 = nullptr;
  int side_pending = 0;          // bit 0: side has unjoined work (ev_side), bit 1: side2 (ev_side2)
  // co-launched sweep (see launch_side_fused): only the GammaV algebra stays on `side`; its
  // Philox sweep counter is snapshotted into d_iter_side by the launch that forks it, so the
  // main stream may advance d_iter for the next sweep while it runs
  bool side_fused = false;
  // HMSC_SIDE_PARTIALS=1 (read at create): the species partials always from post_bl_kernel on
  // the side stream, forked on the device at the tails flag -- the fused launch ends ~5 us
  // sooner, but the side work beside Eta and z costs them about as much (same 1000-step rate)
  // and a replay's first sweeps wait longer for it (20-step line ~2 % lower)
  bool side_partials = false;
  // kernel record copies (HMSC_KERNEL_COPY, kernels.hip rec_copy_kernel): graph replays' packs
  // raise pack_flags and a copy kernel per sample moves it to the host ring
  bool kcopy = false;
  bool cap_kcopy = false;          // the capture in progress packs with flags
  uint64_t* pack_flags = nullptr;  // [3 parts][ring_slots]
  int* pack_ticket = nullptr;      // [3 parts, copy kernel]
  uint32_t run_nonce = 0;          // desc[4]: flags of an earlier run never match
  double* host_rec_dev = nullptr;  // the pinned host ring's device address
  int cap_pack_mask = 0;           // pack parts captured since the last reset (capture_sweeps)
  // graph sweeps after the first of a capture (cap_sweep > 0): the side work is not forked
  // from the main stream nor joined into it by graph edges (each a ~5-6 us cross-queue gap on
  // the critical path) but synchronised by device flags: its first launch waits for the fused
  // launch's tails (gbl_sync[2]), and the next fused launch waits for its side_sync flags
  int cap_sweep = -1;
  bool edge_free = true;    // (HMSC_SIDE_EDGES=1: graph edges everywhere)
  // The test and measurement switches of the launch structure, read once when the chain is
  // created (capi.cpp read_create_knobs): every launch and capture of a chain sees one setting
  struct Knobs {
    bool no_tail_defer = false;   // HMSC_NO_TAIL_DEFER: the BetaLambda tail reduces in its own launch
    bool no_bl_predraw = false;   // HMSC_NO_BL_PREDRAW: BetaLambda's noise drawn in its prologue
    bool no_side_gate = false;    // HMSC_NO_SIDE_GATE: the fused launch polls the side flags itself
    bool g2_part_inline = false;  // HMSC_G2_PART_INLINE: Gamma2's partials ahead of the first BetaLambda bodies
    bool g2f_global = false;      // HMSC_G2F_GLOBAL: Gamma2's final stage in global memory at any size
    bool graph_debug = false;     // HMSC_GRAPH_DEBUG: print each captured graph's node and edge counts
    bool diag_timing = false;     // HMSC_DIAG_TIMING: print hmsc_run's enqueue, wait and unpack times
    int unpack_threads = 4;       // HMSC_UNPACK_THREADS: record unpack workers
    std::string z_sched;          // HMSC_Z_SCHED="n1xt1,n2xt2,...": the z grid's site-chunk schedule, forced
    bool z_general = false;       // HMSC_Z_GENERAL: every chain draws by the general (NA-capable, scaled) pair draw
    int z_stamp_by = 0, z_stamp_chunk = 0;  // HMSC_Z_STAMP_WG="by,chunk": the stamped z workgroup (stamps build)
  } knobs;
  // edge_free for the capture in progress / the graphs held: only while this chain is the one
  // live chain on its device in the process.  Device-side joins need the main and side streams
  // on separate hardware queues; the streams of several chains (nParallel > 1 on one GPU) can
  // share the few queues and wait on each other in a cycle, so their graphs keep
  // graph edges, and graphs captured edge-free are rebuilt once a second chain appears.
  bool edge_free_now = false, graph_edge_free = false;
  bool counted_live = false;  // counted in capi.cpp's live chains of its device
  int z_lean_last = -1;  // the last drawing z launch's pair draw: 0 general, 1 lean (debug_get "zlean")
  int g2bl_last_tail = -1, g2bl_last_nb = 0;  // the last fused Gamma2 + BetaLambda launch's layout (debug_get "g2bl")
  bool side_gated = false;  // the last slab launch waited for the side chain's flags (SideGate)
  bool side_tail = false;   // the last side chain raises side_sync (the next fused launch may join it on the device)
  // the capture in progress forked the side stream at the graph's root, so its first sweep's
  // side work waits for the tails flag on the device too (no edge from the fused launch)
  bool side_root = false;
  bool psi_side = true;     // the last sweep's psi draws ran on the side stream (post_bl_kernel), not in the tail
  int* side_sync = nullptr;      // [GammaV, delta chain per level ..., Gamma2 prep, (slot SIDE_ARB_SLOT) the
                                 // sharded Eta solve's all-reduce-B flag]: epoch of the sweep
  bool shard_dev = false;        // this sharded sweep joins and forks its side chain on the device (sweep_sharded)
  double* gvt = nullptr;         // the BetaLambda tail's GammaV / psi partial tiles
  int gvt_ld = 0;
  double* Gamma_side = nullptr;  // GammaV's Gamma, for the side stream's record pack
  uint32_t* d_iter_side = nullptr;
  double* gv_part = nullptr;     // GammaV species partials (not shared with Gamma2's ABpart)

  // model (device)
  double *X = nullptr, *Tr = nullptr, *Yval = nullptr, *Yraw = nullptr;
  int8_t* Ycode = nullptr;
  uint64_t* Ybits = nullptr;     // ceil(nsl / 32) x ny: the same codes + 1, 2 bits per species (z kernel)
  double* logtab = nullptr;      // z_log_table: the z kernel's table log (ZLOG_N x ZLOG_W)
  int* fam = nullptr;            // ns_loc family code
  int* varest = nullptr;         // ns_loc distr[,2]
  double *V0 = nullptr, *iUGamma = nullptr, *mGamma = nullptr, *UGammaL = nullptr, *UGamma = nullptr;
  double* geWork = nullptr;      // updateGammaEta workspace (gamma_eta.hip), only if that updater is on
  size_t geWork_doubles = 0;     // its size (grown with the levels' nf)
  double *aSigma = nullptr, *bSigma = nullptr;
  double *XX = nullptr, *TT = nullptr, *V0g = nullptr, *V0gXXV0g = nullptr, *iV0 = nullptr;
  double* V0inv = nullptr;       // V0^-1 (initial riwish draw)
  double* iUmG = nullptr;        // iUGamma %*% mGamma
  double* V0gXX = nullptr;       // Gamma2 prior covariance times X'X
  double* g2prep = nullptr;      // Gamma2 iV-only matrices [A1|B1|TR|LS]
  double* scratch2 = nullptr;    // side-stream scratch
  bool g2prep_valid = false;
  int* na_cols = nullptr;        // local species with any NA
  int* na_index = nullptr;       // nsl: row of species j in Gna, or -1
  int n_na_cols = 0;
  int* na_rows = nullptr;        // rows with any NA in the whole Y (every rank of a sharded chain: the same rows)
  int8_t* row_na = nullptr;      // ny: 1 if the row has an NA
  int* row_slot = nullptr;       // ny: index into na_rows, or -1
  int n_na_rows = 0;
  int* dev_flags = nullptr;      // device error flags (Cholesky failures)
  int* gbl_sync = nullptr;       // gamma2_bl_kernel's in-launch handshake [ticket, Gamma epoch, tails epoch, error]
  std::vector<int> h_na_cols;

  // chain state (device)
  double *Z = nullptr, *BL = nullptr, *Psi = nullptr, *Delta = nullptr;
  double *Gamma = nullptr, *iV = nullptr, *iSigma = nullptr;
  double* rho = nullptr;          // updateRho grid index, 1-based (R's rho), as a double

  // phylogeny (hM$C != NULL, phylo.hip): spectral form of computeDataParameters' Qg grid
  bool phylo = false;
  int nrho = 0;
  int phNmax = 0;                // K * ns the dense BetaLambda workspace holds
  double* phU = nullptr;         // ns x ns eigenvectors of C
  double* phWinv = nullptr;      // nrho x ns  1 / q_g,i
  double* phRbase = nullptr;     // nrho  log(rhopw[,2]) - nc/2 logdet Q_g
  double* phTt = nullptr;        // ns x nt  U^T Tr
  double* phBt = nullptr;        // nc x ns  Beta U
  double* phEt = nullptr;        // nc x ns  Beta U - Gamma Tt^T
  double* phTTw = nullptr;       // nt x nt  Tr^T iQ Tr
  double* phWork = nullptr;      // dense BetaLambda / Rho workspace

  // reduced-rank regression covariates (rrr.hip; hmsc_model ncRRR > 0): the last ncRRR columns
  // of X are XRRR wRRR^T, rewritten -- with everything derived from them -- whenever wRRR
  // changes (rrr_refresh_x)
  int ncRRR = 0, ncORRR = 0;
  double nuRRR = 3, a1RRR = 1, b1RRR = 1, a2RRR = 50, b2RRR = 1;
  double* XRRR = nullptr;        // ny x ncORRR  hM$XRRRScaled
  double* XAtXR = nullptr;       // ncNRRR x ncORRR  t(XScaled) XRRR (constant)
  double* XRtXR = nullptr;       // ncORRR x ncORRR  t(XRRR) XRRR (constant)
  double* wRRR = nullptr;        // ncRRR x ncORRR
  double* PsiRRR = nullptr;      // ncRRR x ncORRR
  double* DeltaRRR = nullptr;    // ncRRR
  double* rrrPart = nullptr;     // the Z pass' per-workgroup partials (Z chunks, then the Eta columns)
  double* rrrWork = nullptr;     // its reduced sums and the dense wRRR system (rrr_work_doubles)

  // variable selection (betasel.hip; hmsc_model ncsel > 0).  BLx = m o BL is what every reader
  // of X Beta takes; without selections it is BL itself
  int ncsel = 0, selTot = 0;     // selections, and the groups of all of them (sum of selNg)
  int selNg[SEL_MAX] = {}, selOff[SEL_MAX] = {}, selNcov[SEL_MAX] = {}, selGoff[SEL_MAX] = {};
  std::vector<double> h_selQ;
  int* selOwner = nullptr;       // nc: the selection holding column c, or -1
  int* selCov = nullptr;         // ncsel x nc: the columns of selection i (selNcov[i] of them)
  int* selSpg = nullptr;         // ncsel x ns: 0-based group of species j in selection i
  int* selPerm = nullptr;        // ncsel x ns: the species sorted by group, index order within a group
  int* selGoffD = nullptr;       // per selection ng + 1 offsets into its selPerm row (selGoff[i]: where they start)
  int* selBoff = nullptr;        // ncsel: selOff on the device
  double* selQ = nullptr;        // selTot prior inclusion probabilities
  double* selB = nullptr;        // selTot BetaSel (0 / 1)
  double* selM = nullptr;        // nc x ns column mask m
  double* selLR = nullptr;       // selTot: lldif + pridif of the last update
  double* selSc = nullptr;       // selTot: the absolute scale of its terms
  double* selTerm = nullptr;     // ns x 3 per-species terms
  double* BLx = nullptr;         // K x ns  m o BL (== BL when ncsel == 0)

  // per-sweep workspaces
  double* XEta = nullptr;        // ny x Kmax    [X, Eta_1[Pi_1], ...] materialised per Eta update
  bool xeta_valid = false;
  // G's Eta rows from the fused Eta pass' tile partials not reduced yet: the next updateZ
  // launch reduces them on extra workgroups (z_kernel.h), any other reader of G first calls
  // flush_g (kernels.hip)
  bool g_pending = false;
  int g_ntile = 0, g_nf = 0;
  // debug counters (hmsc_debug_get "eta_fused"): eta_fused_kernel launches issued so far (a
  // captured one counts once), the last one's NFB bucket and EtaMode
  uint64_t eta_fused_launches = 0;
  int eta_fused_nfb = 0, eta_fused_mode = 0;
  double* XZ = nullptr;          // K x ns_loc   XEta^T (Yx o Z)
  double* G = nullptr;           // Kmax x Kmax  XEta^T XEta
  double* ZTr = nullptr;         // ny x nt      Z Tr (local species)
  double* XZ_part = nullptr;     // nchunk x K x ns_loc
  // the next sweep's BetaLambda noise and psi gamma variates, drawn ahead by the Eta launch
  // (kernels.hip bl_predraw_body): [species][64] (lane k < K: xi; 32 + f: psi's gamma), and
  // the (sweep, K) they were drawn for
  double* bl_pre = nullptr;
  int* bl_pre_tag = nullptr;
  double* G_part = nullptr;      // nchunk x Kmax^2
  double* ZTr_part = nullptr;    // ntile_j x ny x nt
  double* Gna = nullptr;         // n_na_cols x Kmax^2 masked grams
  double* ZL = nullptr;          // ny x NFP   Z * (Lambda diag(iSigma))^T, all levels
  double* ZL_part = nullptr;     // zl_split x ny x NFP
  double* CR = nullptr;          // Kmax x NFmax  BL diag(iSigma) Lambda_all^T
  double* CR_part = nullptr;     // species-block partials of CR
  double* LS = nullptr;          // NFmax x ns_loc  Lambda_all diag(iSigma) (fused Eta kernel)
  double* crw_part = nullptr;    // the fused Eta constants' partial tiles (kernels.hip crw_body / crw_tail)
  int* crw_ticket = nullptr;     // [crw_kernel, crw_tail's groups, crw_tail's per-group tickets, crw_flag]
  int* crw_flag = nullptr;
  double* etaW = nullptr;        // 16 x 16  L^-1 of Q = I + Lambda diag(iSigma) Lambda^T (fused Eta kernel)
  double* Msmall = nullptr;      // per-level masked row grams (NA rows)
  double* scratch = nullptr;     // single-workgroup updaters
  double* psi_rs = nullptr;      // psi-lambda^2 row-sum partials
  double* ABpart = nullptr;      // GammaV species-partials
  double* dbg_prec = nullptr;    // optional debug: per-species precisions
  bool zt_valid = false;         // XZ/G/ZTr computed for the current Z and Eta
  int nchunk = 0, ntile_j = 0, zl_split = 0, NFP = 0;
  // the z grid's site-chunk schedule, fixed at create (zdraw.hip z_schedule_setup): segment i is
  // z_seg_n[i] chunks of z_seg_t[i] 64-site tiles, z_chunks chunks in all (<= nchunk)
  int z_seg_n[4] = {0, 0, 0, 0}, z_seg_t[4] = {0, 0, 0, 0}, z_chunks = 0;
  size_t scratch_doubles = 0;
  size_t scratch2_doubles = 0;  // Gamma2's prep working set, then its final stage's arrays past 64 KB

  // recording ring
  double* ring = nullptr;
  int ring_slots = 0;
  size_t slot_doubles = 0;
  double* host_rec = nullptr;    // pinned host ring (ring_slots slots)
  uint64_t* copied_host = nullptr;  // fine-grained pinned counter: samples whose D2H copy landed
  uint64_t* copied_dev = nullptr;   // its device address
  std::shared_ptr<struct UnpackPool> unpack_pool;
  int* trsv_sync = nullptr;  // the dense handshake block (DENSE_SYNC_INTS ints, zeroed): sync-free solves, fused panel

  // per-sweep hipGraph (single rank, no updateNf): captured once, replayed every sweep; the
  // kernels read the Philox sweep counter from d_iter, which the graph's first node advances
  uint32_t* d_iter = nullptr;          // the Philox sweep counter captured kernels read (a slot of d_iters)
  uint32_t* d_iters = nullptr;         // one counter per captured sweep; a replay's last kernel advances them
  bool capturing = false;
  bool use_graph = true;
  bool graph_dirty = true;
  int graph_K = -1, graph_NF = -1;
  // gx[rec][k]: 2^k consecutive sweeps (rec: each followed by the record pack), k = 0 ..
  // log2(graph_sweeps); a run of n sweeps replays its binary decomposition, largest first
  static constexpr int GRAPH_LEVELS = 7;  // up to 64 sweeps per replay
  hipGraphExec_t gx[2][GRAPH_LEVELS] = {};
  int gx_pack_mask[2][GRAPH_LEVELS] = {};  // kcopy: the pack parts every recorded sweep of the graph raises (-1: mixed)
  // The first sweep of a replay's side work (side chain [+ record pack part 2]) runs outside
  // the graph: a graph launch submits its side-stream nodes only after all its main-stream
  // nodes (~16 us of host time per sweep), so that sweep's side chain started late and the
  // next sweep's fused launch waited for it.  capture_sweeps keeps it as a closure per graph
  // (ext_side, launched on the side stream ahead of the graph by replay_sweeps) instead.
  std::function<void()> ext_pending;                // built while capturing sweep 0
  std::function<void()> ext_side[2][GRAPH_LEVELS];  // per graph in gx
  uint32_t* d_ext_iter = nullptr;                   // the external side work's sweep counter
  hipEvent_t ev_ext = nullptr;                      // after it: the record copy waits on it
  hipEvent_t ev_ext_go = nullptr;                   // the replay's start, which it waits behind
  bool ext_launched = false;
  int graph_sweeps = 4;                 // sweeps per replay, a power of two (HMSC_GRAPH_SWEEPS)
  uint32_t dev_iter_next = 0;           // the sweep the device's d_iters slots already hold (valid_iters)
  bool valid_iters = false;
  int32_t* d_rec_desc = nullptr;        // {iter0, transient, thin, samples} of the current run
  hipEvent_t ev_graph = nullptr;        // after a recording replay: the copy stream waits on it
  int eager_streak = 0;          // eager steady sweeps since the graph was invalidated

  // live launch timing of the timed kernels (common.h kt_record): per-sweep-slot first
  // start / last finish wall-clock ticks, KT_N blocks of 2 * KT_SLOTS
  unsigned long long* d_kt = nullptr;
  bool kt_on = false;

  // live kernel timing (HIP events on this chain's stream), id -> launches
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[12];

  // RCCL (species-sharded chain), or a host transport (hmsc_create_sharded_host)
  void* comm = nullptr;
  double* allreduce_buf = nullptr;
  hmsc_allreduce_fn host_allreduce = nullptr;
  void* host_allreduce_ctx = nullptr;
  std::vector<double> host_ar_buf;

  // ---- species-sharded chain (kernels.hip "species-sharded sweep", capi.cpp sweep_sharded).
  // A sharded chain (nranks > 1, or a 1-rank chain created with a communicator or a host
  // transport) reduces its cross-species sums in exactly two all-reduces per sweep:
  //   A (after updateZ, for the next sweep's updateGamma2): ar_a = [X^T Z Tr (nc nt) |
  //     Lambda_all Tr (NF nt) | #(iSigma != 1)]   (R/updateGamma2.R:36,46)
  //   B (after updateBetaLambda): ar_b = [ZL = Z (Lambda diag(iSigma))^T (ny NF, site-major) |
  //     CR = BL diag(iSigma) Lambda^T (K x NF, ld K) | GammaV's E E^T, B Tr (nc^2 + nc nt) |
  //     sum_j psi lambda^2 (NF) | NA rows: CR masked to the row's observed species
  //     (n_na_rows x K x NF)]   (R/updateEta.R:45-55,59-70, R/updateGammaV.R:16-18,
  //     R/updateLambdaPriors.R:22-32)
  // Everything downstream of a sum (Gamma, iV, Delta, Eta) is drawn redundantly on every
  // rank from the same Philox counters, so the ranks' copies stay bit-identical.
  bool sharded = false;
  bool any_na_global = false;    // any NA in the whole Y (the fusion decisions of every rank agree)
  double* ar_a = nullptr;
  double* ar_b = nullptr;
  double* ar_host = nullptr;     // pinned host staging of the host transport (max of A, B)
  size_t ar_host_doubles = 0;
  int* shard_ticket = nullptr;   // [g2 stats ticket, spare]: zero between launches
  bool g2s_valid = false;        // ar_a holds the reduced Gamma2 sums of the current Z, BL, iSigma
  // debug counters (hmsc_debug_get "ar_calls"): collectives issued / executed and their doubles;
  // the all-reduces a captured sweep contains (graph replays add ar_per_graph_sweep per sweep)
  uint64_t ar_calls = 0, ar_doubles = 0;
  int ar_in_capture = 0, ar_per_graph_sweep = -1;
  // host transport inside graph capture: a sweep is captured as segments split at its
  // all-reduces (the host sums between them); cap_segs collects them during the capture
  struct Seg {
    hipGraphExec_t g = nullptr;
    size_t ar_n = 0;             // doubles of ar_host to all-reduce after this segment (0: none)
    double* ar_dev = nullptr;    // (the device buffer the next segment copies the sum back into)
  };
  std::vector<std::pair<hipGraph_t, size_t>>* cap_segs = nullptr;
  std::vector<Seg> gseg[2];      // [with record]: one sweep of a host-transport sharded chain

  std::vector<int> h_nf() const {
    std::vector<int> v(nr);
    for (int r = 0; r < nr; ++r) v[r] = lev[r].nf;
    return v;
  }
  int loff(int r) const {  // row offset of level r inside BL
    int o = nc;
    for (int q = 0; q < r; ++q) o += lev[q].nf;
    return o;
  }
  int foff(int r) const {  // row offset of level r inside Psi / Delta
    int o = 0;
    for (int q = 0; q < r; ++q) o += lev[q].nf;
    return o;
  }
  void refresh_dims() {
    NF = 0;
    for (int r = 0; r < nr; ++r) NF += lev[r].nf;
    K = nc + NF;
  }
};

// the Philox sweep counter a launch reads on the device: the captured sweep's slot, or null for
// an eager launch (which passes iter by value, common.h SWEEP_ITER)
inline const uint32_t* iter_src(const State& s) { return !s.capturing ? nullptr : s.d_iter; }
// the live-timing block of timed kernel id (common.h KtId), or null with the timers off
inline unsigned long long* kt_slot(const State& s, int id) {
  return s.kt_on ? s.d_kt + (size_t)id * 2 * KT_SLOTS : nullptr;
}

enum ProfId {
  PROF_Z = 0, PROF_ZL = 1, PROF_BL = 2, PROF_ETA_UNIT = 3, PROF_SWEEP = 4,
  PROF_ETA_SP = 5,  // spatial updateEta (assembly + blocked Cholesky + solves)
  PROF_CHOL = 6,    // the blocked Cholesky inside it
  PROF_ALPHA = 7,   // updateAlpha (grid quadratic forms + draw)
  PROF_GE = 8,      // updateGammaEta (all levels)
  PROF_RHO = 9,     // updateRho
  PROF_WRRR = 10,   // updatewRRR's pass over Z
  PROF_BETASEL = 11,  // updateBetaSel (all selections)
  PROF_N = 12
};
static_assert(PROF_N <= 12, "State::prof_ev holds 12 profile ids");

struct ProfScope {  // records a start/stop event pair around one launch when profiling is on
  State& s;
  int id;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(State& st, int i) : s(st), id(i) {
    if (s.prof) {
      a = s.own.event();
      b = s.own.event();
      (void)hipEventRecord(a, s.stream);
    }
  }
  ~ProfScope() {
    if (s.prof) {
      (void)hipEventRecord(b, s.stream);
      s.prof_ev[id].emplace_back(a, b);
    }
  }
};

// launchers implemented in kernels.hip
void launch_init(State& s);
void launch_update_z(State& s, uint32_t iter, bool use_raw_y);
void launch_zt_refresh(State& s);
int z_resident_slots(const State& s);
void z_schedule_setup(State& s);  // the z grid's site-chunk schedule and s.nchunk (zdraw.hip)
void z_require_shard_start(int sp0);  // a species shard starts at a species quad (zdraw.hip)
int z_xeta_cols_for(int Kmax);  // XEta columns the z kernel reads (zdraw.hip)
void ext_add_record(State& s);  // add record pack part 2 to the external first-sweep side work (kernels.hip)
void launch_xeta(State& s);
void flush_g(State& s);
// SideGate: the slab launch after updateZ waits (one extra workgroup) for the flags of this
// sweep's side chain that the next sweep's fused Gamma2 + BetaLambda launch would otherwise
// poll at its start (kernels.hip side_gate_next); n = 0: no gate
struct SideGate {
  const int* flags = nullptr;
  int n = 0;
  uint32_t iter = 0;
  const uint32_t* iter_dev = nullptr;
  int* err = nullptr;
};
SideGate side_gate_next(State& s, uint32_t iter);
void launch_slab_sum2(const double* p0, double* o0, int64_t n0, int np0, const double* p1, double* o1, int64_t n1,
                      int np1, hipStream_t st, SideGate gate = SideGate{});
// the same with the main-stream record pack (part 1) of a captured recorded sweep appended
void launch_slab_sum2_pack(State& s, const double* p0, double* o0, int64_t n0, int np0, const double* p1, double* o1,
                           int64_t n1, int np1, SideGate gate = SideGate{});
void launch_beta_lambda(State& s, uint32_t iter);
void launch_gamma_v(State& s, uint32_t iter, hipStream_t st);
void launch_gamma2(State& s, uint32_t iter);
bool gamma2_bl_fusion_ok(const State& s);
// What the fused Gamma2 + BetaLambda launch of a sweep hands to that sweep's launch_side_fused
// (all false when it did not run, and on a sharded chain)
struct TailHandoff {
  bool cr_done = false;  // its tail formed the fused Eta constants (CR, W, LS)
  bool defer = false;    // ... with its reductions left to the Eta launch (EF_DEFER)
  // ... and also formed GammaV's and LambdaPriors' species partials (gvt), which the side chain
  // reads instead of post_bl_kernel's
  bool tail_gv = false;
};
TailHandoff launch_gamma2_bl(State& s, uint32_t iter);  // updateGamma2 + updateBetaLambda in one launch
int live_chains_on(int device);                  // chains created and not destroyed on a device (capi.cpp)
// a species-sharded chain on RCCL: a recorded graph sweep packs its main-stream quantities in
// updateZ's slab launch and the side chain's (Gamma, iV, Delta) on the side stream after it,
// so no pack launch waits behind all-reduce A on the main stream (capi.cpp record_after_sweep)
inline bool sharded_pack_split(const State& s) { return s.sharded && s.comm != nullptr; }
// side_sync words: GammaV, the delta chains, Gamma2's prep (1 + nr), then the sharded Eta solve's
// all-reduce-B flag (sweep_sharded's edge-free sweeps)
constexpr int SIDE_ARB_SLOT = 2 + HMSC_MAX_LEVELS, SIDE_SYNC_INTS = SIDE_ARB_SLOT + 1;
inline int* arb_flag_ptr(State& s) { return s.side_sync + SIDE_ARB_SLOT; }
void launch_lambda_priors(State& s, uint32_t iter, hipStream_t st);
void launch_eta(State& s, uint32_t iter);
void launch_inv_sigma(State& s, uint32_t iter);
// record pack; slot == nullptr: device-chosen (graph replay).  part: 0 all, 1 the main-stream
// quantities (BL, Psi, iSigma, Eta), 2 the side-stream ones (Gamma, iV, Delta) on `side`
void launch_record(State& s, double* slot, int part = 0);
void launch_rec_copy(State& s, int k, int parts);
bool side_fusion_ok(const State& s);
// phylogeny branch (phylo.hip)
size_t phylo_work_doubles(int ns, int Kmax, int nc, int nrho);
void launch_phylo_gv_sums(State& s, uint32_t iter, hipStream_t st);
void launch_rho(State& s, uint32_t iter, hipStream_t st);
void launch_beta_lambda_phylo(State& s, uint32_t iter);
void launch_side_fused(State& s, uint32_t iter, TailHandoff h);
// blocked dense fp64 factorisation / solves (dense.hip)
// The dense handshake block (one per chain, State::trsv_sync, zero-initialised): [0] ticket,
// [1] done count, [2 + b] flag of 64-block b of a sync-free solve, [DENSE_SYNC_ERR] the error
// word every bounded in-launch wait raises a bit of on timeout (HS_ERR_*; the host checks it
// after a run, capi.cpp check_device_flags), [DENSE_SYNC_TEST] a test hook
// (hmsc_debug_poison).
constexpr int TRSV_SF_MAXB = 4096;
constexpr int DENSE_SYNC_ERR = 2 + TRSV_SF_MAXB;
constexpr int DENSE_SYNC_TEST = DENSE_SYNC_ERR + 1;
constexpr int DENSE_SYNC_INTS = DENSE_SYNC_ERR + 2;
enum HsErr { HS_ERR_TRSV_FLAG = 1, HS_ERR_TRSV_TICKET = 2, HS_ERR_CHOL_PANEL = 4 };
constexpr int HS_TEST_SKIP_PUBLISH = 1;  // DENSE_SYNC_TEST: the next fused panel step withholds its flag
// a one-shot entry's check of the error word it copied back
inline void dense_handshake_check(int hs) {
  if (hs != 0)
    throw HmscError(-5, "internal: an in-launch handshake of the blocked dense solver timed out (error bits " +
                            std::to_string(hs) + "); the result is invalid");
}
// bw > 0: A is banded (A[i, j] = 0 for i - j > bw, entries outside the band zero on entry);
// the factor keeps the band, and only the band's tiles are touched (n bw^2 work instead of n^3).
// sync: the dense handshake block (enables the fused panel step), or null.
void dense_potrf_lower(hipStream_t st, double* A, int n, int lda, double* ws, int* info, int bw = 0,
                       int* sync = nullptr);
// sync: the dense handshake block for the one-launch sync-free solve, or null for one launch
// per 64-block
void dense_trsv_lower(hipStream_t st, const double* L, int n, int lda, double* x, int trans, double* ws, int bw = 0,
                      int* sync = nullptr);
void dense_trtri_lower(hipStream_t st, const double* L, int ldl, int n, double* M, int ldm, double* dinv,
                       bool have_dinv);
// workspace of dense_potrf_lower + dense_trsv_lower: the 64 x 64 diagonal-block inverses, then n
inline size_t dense_ws_doubles(int n) { return (size_t)((n + 63) / 64) * 64 * 64 + (size_t)n + 64; }
// rows per 64-column panel of the tile-band layout of a band matrix of bandwidth bw (pass
// lda = -dense_band_ld(bw) to dense_potrf_lower / dense_trsv_lower; dense.hip aix): the panel's
// diagonal tile, the tiles below it in the band, and one more for the transposed solve's
// tile-aligned reach
inline int dense_band_ld(int bw) { return 64 * (2 + (bw + 63) / 64); }
void dense_lauum_lower(hipStream_t st, const double* M, int ldm, int n, double* out, int ldo);
// out = U diag(d) U^T (full symmetric), d = dbase + n (*rho - 1) or its reciprocal
void dense_gram_diag(hipStream_t st, const double* U, int ldu, int n, const double* dbase, const double* rho,
                     bool recip, double* out, int ldo);
// R <- L^-1 R for the n x m matrix R (ld ldr), from dense_potrf_lower's factor and workspace
// (krige.hip): one launch, a workgroup per 64 columns of R, no in-launch handshake
void dense_trsm_lower(hipStream_t st, const double* L, int n, int ldl, const double* ws, double* R, size_t ldr, int m);
// kriging at new spatial units (krige.hip; a KrigeLevel of krige_level.h owns the buffers)
struct KrigeDev {
  int np, nn, sdim, S, nfmax;
  int N;                 // np + the call's new units: rows of coords / dist (hmsc_krige: np + nn)
  const int* unit;       // nn: this launch's new units among the call's (a slab of hmsc_predict_map), or
                         // null: 0 .. nn - 1.  The unit's index is its row np + unit[i] and the counter of z.
  size_t ldo;            // out[(s nfmax + h) ldo + i] (hmsc_krige: nn)
  uint64_t seed;
  uint32_t stream;       // S_KRIGE + LEVEL_STRIDE * level
  const double* coords;  // N x sdim, or null
  const double* dist;    // N^2, or null
  const double* Eta;     // S x np x nfmax
  const int* col_s;      // sample / factor of every (s, h) pair, grouped by grid index
  const int* col_h;
  double* K11;           // np x np
  double* R;             // np x (nn + c_max): [K12 | E_g]
  double* W;             // nn x nn ('Full')
  double* Z;             // nn x c_max ('Full')
  double* v;             // nn (predictMeanField)
  double* out;           // S x nn x nfmax, zeroed
  double* ws1;           // dense_ws_doubles(np)
  double* ws2;           // dense_ws_doubles(nn) ('Full')
  int* sync;             // the dense handshake block, zeroed
  const double* knots;   // nK x sdim, column-major ('GPP')
  int nK;
};
// events of one group, recorded at the boundaries of: kernel matrices, potrf K11, trsm, mean,
// syrk, potrf W, trmm (ev: KRIGE_GROUP_PHASES + 1 events, or null)
constexpr int KRIGE_GROUP_PHASES = 7;
// modes 0-2 for the c pairs col0 .. col0 + c - 1 at grid value a; info[0] / info[1] are raised
// when K11 / W is not positive definite
void krige_launch_group(hipStream_t st, const KrigeDev& d, int mode, double a, int col0, int c, int* info,
                        hipEvent_t* ev);
// the same in two parts for a call that walks its new units in slabs (krige.hip): per grid value
// what the fitted units alone decide, then per slab d.R (np x nn), d.v, d.unit, d.out, d.ldo
void krige_plan_group(hipStream_t st, const KrigeDev& d, double a, int col0, int c, double* K11, double* ws, double* Y,
                      int* info);
void krige_slab_group(hipStream_t st, const KrigeDev& d, int mode, double a, int col0, int c, const double* K11,
                      const double* ws, const double* Y, hipEvent_t* ev);
// mode 3 for all pairs: group g is the pairs g_off[g] .. g_off[g + 1] - 1 at grid value g_alpha[g]
void krige_launch_nn(hipStream_t st, const KrigeDev& d, int k, int ngroups, const double* g_alpha, const int* g_off,
                     int* info);
// mode 4, 'GPP' (gpp.hip).  The plan's workspace, shared by the grid values of a call and carved from
// gpp_plan_doubles(np, nK, cmax) doubles: A (Wss's place, then iF), F (then chol(iF)), M (a factor's
// inverse), W12 (np x nK), idD (np), E (np x cmax), T and Zk (nK x cmax), ws (dense_ws_doubles(nK)).
struct GppWork {
  double *A, *F, *M, *W12, *idD, *E, *T, *Zk, *ws;
};
inline size_t gpp_plan_doubles(int np, int nK, int cmax) {
  const size_t k = (size_t)nK, n = (size_t)np, c = (size_t)cmax;
  return 3 * k * k + n * k + n + n * c + 2 * k * c + dense_ws_doubles(nK);
}
GppWork gpp_carve(double* base, int np, int nK, int cmax);
// once per grid value a > 0, for the c pairs col0 .. col0 + c - 1: iWss (nK x nK) and C = mu + eps
// (nK x c), the resident state.  info[0 .. 2] are raised when Wss, F or iF is not positive definite,
// info[3] = np - i for the lowest fitted unit i on a knot or with dD_i <= 0.  ev: GPP_PLAN_PHASES + 1
// events or null, at the boundaries of: Wss and W12, iWss, dD and F, iF and chol(iF), C.
constexpr int GPP_PLAN_PHASES = 5;
void gpp_plan_group(hipStream_t st, const KrigeDev& d, const GppWork& w, double a, int col0, int c, double* iWss,
                    double* Cm, int* info, hipEvent_t* ev);
// per slab of d.nn new units (d.unit): sqrt(dDn) into d.v, then out = Wns C + d.v o z_new into d.out
// (ld d.ldo).  ev: 3 events or null, at the boundaries of: the dDn pass, the slab product.
void gpp_slab_group(hipStream_t st, const KrigeDev& d, double a, int col0, int c, const double* iWss, const double* Cm,
                    hipEvent_t* ev);
// the 'Full' alphapw grid on the device (R/computeDataParameters.R:53-81) from coordinates
// (np x sdim, column-major) or a distance matrix (np x np): RiWg = chol(W_g)^-1 (lower),
// iWg = RiWg^T RiWg, detWg = log det W_g
void spatial_full_grid(hipStream_t st, int np, int sdim, const double* coords, const double* dist,
                       const double* alphas, int G, double* iWg, double* RiWg, double* detWg, int* info);
// spatial "Full" levels (spatial.hip)
size_t spatial_work_doubles(const State& s, int r);
// NNGP level setup on the host: nearest earlier neighbours, Vecchia coefficients over the
// alphapw grid, detWg, the RCM factorization order and its bandwidth (device arrays of Level)
void setup_nngp_level(State& s, int r, const double* coords, int sdim, int k, const double* alphapw, int G);
void launch_eta_spatial(State& s, int r, uint32_t iter);
void launch_alpha(State& s, uint32_t iter);
// updateGammaEta (gamma_eta.hip)
size_t gamma_eta_work_doubles(const State& s);
void launch_gamma_eta(State& s, uint32_t iter);  // GammaV + LambdaPriors + Eta, co-launched
void join_side(State& s);
// the side streams given (side, and side2 when not null) wait for the main stream's work so far
void fork_side(State& s, hipStream_t side, hipStream_t side2 = nullptr);
void launch_copied_flag(State& s, uint64_t value);
size_t record_slot_doubles(const State& s);
// ---- species-sharded sweep (kernels.hip); ar_point is the transport (capi.cpp)
struct ArbLayout {
  size_t zl = 0, cr = 0, gv = 0, rs = 0, na = 0, n = 0;  // offsets into ar_b, n = doubles in use
  int ldcr = 0;
};
ArbLayout arb_layout(const State& s);
size_t arb_capacity(const State& s);
void ar_point(State& s, double* buf, size_t n);
void sweep_sharded(State& s, uint32_t iter);
void run_updater_sharded(State& s, uint32_t which, uint32_t iter);
bool sharded_fused_ok(const State& s);
void read_stamps(double* out, int n);  // diagnostic build (HMSC_STAMPS)
void read_zstamps(double* out, int n);  // the z kernel's phase stamps (zdraw.hip)
// reduced-rank regression covariates (rrr.hip)
constexpr int RRR_MAX_K = 8;     // ncRRR
constexpr int RRR_MAX_N = 256;   // ncRRR * ncORRR: the dense wRRR system's size
size_t rrr_part_doubles(const State& s);
size_t rrr_work_doubles(const State& s);
void launch_rrr_init(State& s);                  // R/computeInitialParameters.R:20-27
void launch_rrr_refresh(State& s);               // X's RRR columns, XX and the validity flags, after wRRR changed
void launch_wrrr(State& s, uint32_t iter);       // R/updatewRRR.R
void launch_wrrr_priors(State& s, uint32_t iter);  // R/updatewRRRPriors.R
// variable selection (betasel.hip)
void launch_sel_refresh(State& s);               // the mask and BLx = m o BL, after BL or BetaSel changed
void launch_betasel(State& s, uint32_t iter);    // R/updateBetaSel.R

}  // namespace hmsc
