/*
 * hmsc_amd.h — C ABI of the MI355X-native Gibbs sampler behind Hmsc's sampleMcmc().
 *
 * The reference (taddallas/HMSC, R package Hmsc 3.0-4) has no native code and no
 * FFI: its boundary is the R function sampleMcmc() (R/sampleMcmc.R:68-71) whose
 * per-chain body sampleChain() (R/sampleMcmc.R:155-327) runs the sweep loop
 * (:219-325) over R-level updaters.  Each entry point below names the reference
 * interface it replaces.  A maintainer binds them from R with the .Call shim in
 * INTEGRATION.md; this repository binds them with ctypes (hmsc_amd/_lib.py).
 *
 * Conventions
 *   - every matrix is column-major fp64 exactly as R stores it (no transposes);
 *   - Y carries R's NA as NaN; Pi is R's 1-based hM$Pi (stored as int32 here);
 *   - caller owns every input buffer; hmsc_create copies them to the device;
 *   - caller allocates every output buffer;
 *   - return 0 on success, <0 on error; hmsc_last_error() gives the message
 *     (thread-local); no C++ exception or longjmp crosses this boundary.
 */
#ifndef HMSC_AMD_H
#define HMSC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMSC_MAX_LEVELS 8

/* updater switches: R's updater=list(NAME=FALSE) (R/sampleMcmc.R:17,221-294) as a bitmask */
enum hmsc_updater {
  HMSC_UP_GAMMA2 = 1u << 0,       /* updateGamma2       R/updateGamma2.R:6      */
  HMSC_UP_GAMMAETA = 1u << 1,     /* updateGammaEta     R/updateGammaEta.R:7    */
  HMSC_UP_BETALAMBDA = 1u << 2,   /* updateBetaLambda   R/updateBetaLambda.R:8  */
  HMSC_UP_WRRR = 1u << 3,         /* updatewRRR         R/updatewRRR.R:7 (ignored when ncRRR == 0) */
  HMSC_UP_BETASEL = 1u << 4,      /* updateBetaSel      R/updateBetaSel.R:3 (ignored when ncsel == 0) */
  HMSC_UP_GAMMAV = 1u << 5,       /* updateGammaV       R/updateGammaV.R:4      */
  HMSC_UP_RHO = 1u << 6,          /* updateRho          R/updateRho.R:1         */
  HMSC_UP_LAMBDAPRIORS = 1u << 7, /* updateLambdaPriors R/updateLambdaPriors.R:3 */
  HMSC_UP_WRRRPRIORS = 1u << 8,   /* updatewRRRPriors   R/updatewRRRPriors.R:3 (ignored when ncRRR == 0) */
  HMSC_UP_ETA = 1u << 9,          /* updateEta          R/updateEta.R:4         */
  HMSC_UP_ALPHA = 1u << 10,       /* updateAlpha        R/updateAlpha.R:3       */
  HMSC_UP_INVSIGMA = 1u << 11,    /* updateInvSigma     R/updateInvSigma.R:3    */
  HMSC_UP_Z = 1u << 12,           /* updateZ            R/updateZ.R:4           */
  HMSC_UP_ALL = 0x1FFFu
};

/* The hM fields consumed by the sampler (R/Hmsc.R:118-167 after construction and
 * setPriors defaults R/setPriors.Hmsc.R:28-77, R/setPriors.HmscRandomLevel.R:31-108).
 * Zero-initialise the struct and set struct_size = sizeof(hmsc_model) (HMSC_MODEL_SIZE):
 * hmsc_create refuses any other value, so a caller built against an older header (a shorter
 * struct) gets an error instead of having fields read past its end. */
typedef struct hmsc_model {
  int32_t struct_size;    /* sizeof(hmsc_model) of the header the caller was built with */
  int32_t ny, ns, nc, nt, nr;
  const double* Y;        /* ny*ns  hM$YScaled (NaN = NA)                      */
  const double* Yraw;     /* ny*ns  hM$Y (initial Z, R/computeInitialParameters.R:254); may equal Y */
  const double* X;        /* ny*nc  hM$XScaled                                 */
  const double* Tr;       /* ns*nt  hM$TrScaled                                */
  const int32_t* Pi;      /* ny*nr  hM$Pi, 1-based                             */
  const int32_t* np;      /* nr     hM$np                                      */
  const int32_t* distr;   /* ns*4   hM$distr (family, variance, link, -)       */
  const double* V0;       /* nc*nc  */
  double f0;
  const double* mGamma;   /* nc*nt  */
  const double* UGamma;   /* (nc*nt)^2 */
  const double* aSigma;   /* ns */
  const double* bSigma;   /* ns */
  /* per random level r < nr (hM$rL[[r]]) */
  const double* nu;
  const double* a1;
  const double* b1;
  const double* a2;
  const double* b2;
  const int32_t* nfMin;
  const int32_t* nfMax;
  const int32_t* sDim;    /* > 0: spatial level (see spatialMethod below); the number of
                           * coordinate columns when sCoord[r] is given             */
  const int32_t* xDim;    /* 0 for every level passed: a covariate-dependent level is passed
                           * expanded, see etaShare / xScale at the end */
  /* Phylogeny (hM$C; NULL = none).  The grid of R/computeDataParameters.R:19-39
   * (iQg/RQg/detQg over hM$rhopw) is taken in spectral form: the caller passes the
   * eigendecomposition of C (R: e <- eigen(hM$C, symmetric=TRUE); numpy: eigh), from which
   * every Q_g = rho_g C + (1-rho_g) I (or -rho_g iC + (1+rho_g) I for rho_g < 0) follows. */
  const double* C;        /* ns*ns (only tested for != NULL)                  */
  int32_t nrho;           /* nrow(hM$rhopw)                                    */
  const double* rhopw;    /* nrho*2 column-major: grid value, prior weight     */
  const double* C_vectors;/* ns*ns eigenvectors of C, column-major             */
  const double* C_values; /* ns    eigenvalues of C (> 0)                      */
  /* Spatial levels (rL$sDim > 0): the alphapw grid of R/computeDataParameters.R:47-196,
   * per level r (entries of non-spatial levels ignored / NULL), as the dense prior
   * precision of each grid point.  iWg, RiWg are np*np*nalpha column-major (R's
   * [np, np, alphaN] arrays) with RiWg' RiWg = iWg, detWg nalpha = log det W.  RiWg is
   * upper triangular, except for NNGP (R's lower-triangular factor) and GPP (lower).
   *   Full: computeDataParameters' iWg / RiWg / detWg as they are (:53-81).
   *   NNGP: not through these arrays -- sCoord and nNeighbours below (sparse Vecchia form).
   *   GPP:  iWg = diag(idDg[,g]) - idDW12g[,,g] iFg[,,g] t(idDW12g[,,g]) = W^-1, passed as
   *         RiWg = solve(t(chol(W))) (lower) with W = D + W12 iW22 t(W12), iWg = t(RiWg) RiWg,
   *         detWg = detDg (:138-194; the precision R/updateEta.R:148-196 samples from).
   * NNGP and GPP levels need np == ny (R/updateEta.R:140,165 build Diagonal(ny)). */
  const int32_t* spatialMethod;              /* nr: 0 none, 1 Full, 2 NNGP, 3 GPP        */
  const int32_t* nalpha;                     /* nr: nrow(rL$alphapw)                     */
  const double* alphapw[HMSC_MAX_LEVELS];    /* nalpha*2: grid value, prior weight      */
  const double* iWg[HMSC_MAX_LEVELS];      /* Full (host grid) only; NNGP: see sCoord */
  const double* RiWg[HMSC_MAX_LEVELS];
  const double* detWg[HMSC_MAX_LEVELS];
  /* 'Full' levels may leave iWg / RiWg / detWg NULL and hand over the level's geometry
   * instead -- the coordinates hM$rL[[r]]$s of its units in unit order (np x sDim[r],
   * column-major) or their distance matrix (np x np) --: the device then evaluates the grid
   * itself (dist(), exp(-d/alpha), chol, inverse on the matrix cores), storing
   * RiWg = chol(W_g)^-1 (lower; RiWg' RiWg = iWg as before).  At np = 5000 this is the
   * path that fits: two 20 GB grids are built in HBM without a host copy. */
  const double* sCoord[HMSC_MAX_LEVELS];
  const double* distMat[HMSC_MAX_LEVELS];
  /* 'GPP' levels may instead (iWg / RiWg / detWg NULL) hand over computeDataParameters'
   * predictive-process grid as R keeps it (R/computeDataParameters.R:138-194): nKnots[r]
   * knots, idDg (np x nalpha), idDW12g (np x nK x nalpha), Fg and iFg (nK x nK x nalpha),
   * detDg (nalpha), all column-major.  updateEta then samples R's low-rank form
   * (R/updateEta.R:148-196: per-unit nf x nf blocks and one (nK nf)^2 factorization, no
   * np^2 array anywhere) and updateAlpha evaluates R's GPP statistic (R/updateAlpha.R:35-75). */
  const int32_t* nKnots;                     /* nr (entries of non-GPP levels ignored)  */
  const double* idDg[HMSC_MAX_LEVELS];
  const double* idDW12g[HMSC_MAX_LEVELS];
  const double* Fg[HMSC_MAX_LEVELS];
  const double* iFg[HMSC_MAX_LEVELS];
  const double* detDg[HMSC_MAX_LEVELS];
  /* 'NNGP' levels (spatialMethod 2) hand over the coordinates of their units (sCoord[r], unit
   * order) and rL$nNeighbours (nNeighbours[r]; R's default 10): the library finds the nearest
   * earlier neighbours (FNN::get.knn restated), evaluates the Vecchia factor of every alphapw
   * grid point (R/computeDataParameters.R:82-136) and samples in that sparse form (np nNeighbours
   * numbers per grid point; updateEta factors the band of the precision in reverse Cuthill-McKee
   * order).  NNGP levels never take iWg / RiWg. */
  const int32_t* nNeighbours;                /* nr (entries of non-NNGP levels ignored) */
  /* Covariate-dependent levels (HmscRandomLevel(xData=...), rL$xDim = ncr > 0): R's
   * LRan = sum_k (Eta[Pi,] * x[dfPi, k]) %*% Lambda[,,k] (R/updateZ.R:24-29) is passed as ncr
   * consecutive levels r0 .. r0+ncr-1 that share the units (same np, Pi), nf and Eta:
   * etaShare[r] = r0 for each of them (the level whose Eta they use; r itself, or a negative
   * value, for an ordinary level; NULL: none shared) and xScale[r] = column k of rL$x in unit
   * order (np doubles), so level r0+k's XEta columns are Eta[Pi,] * x[Pi, k] and its Lambda,
   * Psi and Delta are R's Lambda[,,k], Psi[,,k] and Delta[,k] with priors nu[k], a1[k], b1[k],
   * a2[k], b2[k] (R/updateBetaLambda.R:22-53, R/updateLambdaPriors.R:34-48).  updateEta draws
   * the shared Eta once per unit from lambdaLocal = sum_k x[q, k] Lambda[,,k]
   * (R/updateEta.R:93-108) and updateNf adds or drops a factor of all ncr levels together
   * (R/updateNf.R).  Not with spatial levels, updateGammaEta or species sharding. */
  const int32_t* etaShare;                   /* nr, or NULL                              */
  const double* xScale[HMSC_MAX_LEVELS];     /* np[r] each, or NULL                      */
  /* Reduced-rank regression covariates (Hmsc(XRRR = ..., ncRRR = ...), R/Hmsc.R:343-420;
   * ncRRR = 0: none, the fields below are not read).  With ncRRR > 0, nc above is hM$nc =
   * ncNRRR + ncRRR (V0, mGamma, UGamma, Gamma, iV and Beta are sized by it), while X stays
   * hM$XScaled, ny x ncNRRR with ncNRRR = nc - ncRRR: the last ncRRR columns of the design
   * matrix are XRRR %*% t(wRRR), which the library rewrites whenever wRRR changes
   * (R/updatewRRR.R:62-73).  Limits of this build: ncRRR <= 8 and ncRRR * ncORRR <= 256 (the
   * wRRR conditional is one dense (ncRRR ncORRR)^2 system factored by one workgroup); the RRR
   * columns count towards K = nc + sum(nf) <= 128.  Refused with ncRRR > 0 in this version:
   * species sharding, HMSC_UP_GAMMAETA, phylogeny (C), spatial levels and covariate-dependent
   * (xScale) levels. */
  int32_t ncRRR, ncORRR;
  const double* XRRR;     /* ny*ncORRR  hM$XRRRScaled                            */
  double nuRRR, a1RRR, b1RRR, a2RRR, b2RRR;  /* hM$nuRRR ... (R/setPriors.Hmsc.R:78-102) */
  /* Variable selection (Hmsc(XSelect = list(...)), R/Hmsc.R:48-59; ncsel = 0: none, the fields
   * below are not read).  Selection i < ncsel switches the covariates covGroup_i on or off per
   * species group: selNg[i] groups, selCov[c + nc i] != 0 where column c is in covGroup_i,
   * selSpGroup[j + ns i] the 1-based group of species j, and selQ the prior inclusion
   * probabilities q_i of all selections one after the other (sum of selNg).  X stays one matrix:
   * the reference's per-species list X[[j]] (deselected columns zeroed) is applied as a 0/1 mask
   * on Beta wherever X Beta or crossprod(X) is formed.  Deviation from Hmsc 3.0-4: the
   * Metropolis ratio of updateBetaSel uses the Gaussian log-density of Z where
   * R/updateBetaSel.R:53,79 evaluates pnorm(log.p = TRUE).  Kept as in the reference: the
   * initial Z is drawn from the unmasked X; BetaSel is not part of a posterior sample.
   * Refused with ncsel > 0 in this version: species sharding, phylogeny (C), ncRRR > 0, spatial
   * levels, covariate-dependent (xScale) levels, a column in two selections, ncsel > 8, and
   * the updater bits HMSC_UP_GAMMA2 and HMSC_UP_GAMMAETA (R/sampleMcmc.R:207-216 clears them:
   * "X is not a matrix"). */
  int32_t ncsel;
  const int32_t* selNg;      /* ncsel */
  const int32_t* selCov;     /* nc*ncsel, 0/1 */
  const int32_t* selSpGroup; /* ns*ncsel, 1-based */
  const double* selQ;        /* sum(selNg) */
} hmsc_model;

#define HMSC_MODEL_SIZE ((int32_t)sizeof(hmsc_model))

/* Sampler state = R's parList (R/computeInitialParameters.R:256-270) with iV in
 * place of V and iSigma in place of sigma, as sampleChain keeps them
 * (R/sampleMcmc.R:161-177).  Per-level arrays are indexed [r]; Eta[r] is
 * np[r]*nf[r], Lambda/Psi[r] nf[r]*ns, Delta/Alpha[r] nf[r] (Alpha 1-based grid index). */
typedef struct hmsc_params {
  double* Gamma;          /* nc*nt */
  double* iV;             /* nc*nc */
  double* Beta;           /* nc*ns */
  double* iSigma;         /* ns    */
  double* Z;              /* ny*ns (may be NULL) */
  int32_t rho;            /* 1-based */
  int32_t nf[HMSC_MAX_LEVELS];
  double* Eta[HMSC_MAX_LEVELS];
  double* Lambda[HMSC_MAX_LEVELS];
  double* Psi[HMSC_MAX_LEVELS];
  double* Delta[HMSC_MAX_LEVELS];
  int32_t* Alpha[HMSC_MAX_LEVELS];
  /* reduced-rank regression; neither read nor written when the model's ncRRR == 0 (callers
   * built before these fields existed leave them unset) */
  double* wRRR;           /* ncRRR*ncORRR, column-major */
  double* PsiRRR;         /* ncRRR*ncORRR */
  double* DeltaRRR;       /* ncRRR */
  /* variable selection; neither read nor written when the model's ncsel == 0 */
  int32_t* BetaSel;       /* sum(selNg): 0/1, the selections one after the other */
} hmsc_params;

/* Recording buffers for hmsc_run: caller-allocated, `samples` slots each.  The
 * fields are the raw (scaled-X) state; the host applies combineParameters
 * (R/combineParameters.R:1-58) afterwards.  Eta/Lambda/Psi/Delta/Alpha slots are
 * padded to nfcap[r] (hmsc_get_nf_cap: min(nfMax[r], the K <= 64 limit)); rec_nf[r*samples+k]
 * gives the live nf of sample k. */
typedef struct hmsc_record {
  double* Beta;           /* samples*nc*ns */
  double* Gamma;          /* samples*nc*nt */
  double* iV;             /* samples*nc*nc */
  double* iSigma;         /* samples*ns    */
  int32_t* rho;           /* samples       */
  double* Eta[HMSC_MAX_LEVELS];     /* samples*np[r]*nfcap[r]  */
  double* Lambda[HMSC_MAX_LEVELS];  /* samples*nfcap[r]*ns     */
  double* Psi[HMSC_MAX_LEVELS];     /* samples*nfcap[r]*ns     */
  double* Delta[HMSC_MAX_LEVELS];   /* samples*nfcap[r]        */
  int32_t* Alpha[HMSC_MAX_LEVELS];  /* samples*nfcap[r]        */
  int32_t* rec_nf;                  /* nr*samples              */
  /* reduced-rank regression; not touched when the model's ncRRR == 0 */
  double* wRRR;                     /* samples*ncRRR*ncORRR    */
  double* PsiRRR;                   /* samples*ncRRR*ncORRR    */
  double* DeltaRRR;                 /* samples*ncRRR           */
  /* variable selection; not touched when the model's ncsel == 0 */
  int32_t* BetaSel;                 /* samples*sum(selNg)      */
} hmsc_record;

typedef struct hmsc_state hmsc_state;

/* Thread-local description of the last error. */
const char* hmsc_last_error(void);

/* Number of visible MI355X devices. */
int hmsc_device_count(int32_t* n);

/* Create one chain's device state: copies the model, allocates HBM for the state
 * at nfcap (hmsc_get_nf_cap; work buffers of the dense updaters follow the nf in use), keys Philox by `seed` (R: set.seed(initSeed[chain]), R/sampleMcmc.R:158).
 * Replaces the per-chain setup of sampleChain, R/sampleMcmc.R:155-216. */
int hmsc_create(const hmsc_model* model, uint64_t seed, int32_t device, uint32_t updater_mask,
                hmsc_state** out);

/* Species-sharded single chain: this rank owns species
 * [sp_begin, sp_end) of the model passed in full; `comm_id` is the 128-byte RCCL
 * unique id from hmsc_comm_unique_id() broadcast by rank 0 (NULL when nranks==1). */
int hmsc_create_sharded(const hmsc_model* model, uint64_t seed, int32_t device,
                        uint32_t updater_mask, int32_t rank, int32_t nranks,
                        const void* comm_id, hmsc_state** out);
int hmsc_comm_unique_id(void* out128);

/* The same species-sharded chain with a host transport in place of RCCL: every cross-shard
 * fp64 sum calls fn(buf, n, ctx), which must replace the n doubles at buf (host memory) by
 * their sum over all ranks and return 0.  For hosts without a device-to-device fabric, and
 * for exercising the sharded path on one GPU (several ranks, one device). */
typedef int (*hmsc_allreduce_fn)(double* buf, int64_t n, void* ctx);
int hmsc_create_sharded_host(const hmsc_model* model, uint64_t seed, int32_t device,
                             uint32_t updater_mask, int32_t rank, int32_t nranks,
                             hmsc_allreduce_fn fn, void* ctx, hmsc_state** out);
/* The species block [sp0, sp0 + nsl) rank `rank` of `nranks` owns in hmsc_create_sharded:
 * whole species quads (updateZ's Philox species quads), the ceil(ns/4) quads spread evenly,
 * rank r owning quads [floor(r Q/nranks), floor((r+1) Q/nranks)); an error if that block is
 * empty (fewer quads than ranks).  No reference counterpart (species sharding is new). */
int hmsc_shard_range(int32_t ns, int32_t rank, int32_t nranks, int32_t* sp0, int32_t* nsl);

void hmsc_destroy(hmsc_state* s);

/* computeInitialParameters(hM, initPar=NULL) on the device, including the initial
 * updateZ (R/computeInitialParameters.R:17-273). nf0[r] = starting nf (nfMin). */
int hmsc_init_state(hmsc_state* s, const int32_t* nf0);

/* initPar / resume: overwrite state (R/computeInitialParameters.R:82-227). */
int hmsc_set_state(hmsc_state* s, const hmsc_params* p);
int hmsc_get_state(hmsc_state* s, hmsc_params* p);
int hmsc_get_nf(hmsc_state* s, int32_t* nf);
/* nfcap[r]: the factors level r's buffers and record slots hold, min(nfMax_r, 64 - nc - the
 * other levels' nfMin) (K = nc + sum(nf) <= 64 in this build).  Below nfMax_r (R's default
 * nfMax = ns for many species) the run fails with -6 only if updateNf must grow the level
 * past it.  hmsc_record's per-level arrays are strided by nfcap, not nfMax. */
int hmsc_get_nf_cap(hmsc_state* s, int32_t* nfcap);

/* The closing step of computeInitialParameters: Z = updateZ(Y = hM$Y, Z = LFix + LRan, ...)
 * at the CURRENT state (R/computeInitialParameters.R:229-254) -- after hmsc_set_state has
 * applied an initPar (or initPar = "fixed effects", :52-79), as the reference draws Z last. */
int hmsc_init_z(hmsc_state* s);

/* One Gibbs sweep in the reference block order, R/sampleMcmc.R:219-306.
 * `iter` is the 1-based sweep number (Philox counter word 3 and updateNf's iter). */
int hmsc_sweep(hmsc_state* s, int32_t iter, int32_t adapt_nf);

/* A single updater (per-updater tests; R's tests call updaters directly,
 * tests/testthat/test-sampling.R). `which` is one hmsc_updater bit. */
int hmsc_update(hmsc_state* s, uint32_t which, int32_t iter);

/* noise_mode 1: every Gaussian innovation is zero, so Gaussian blocks return their
 * conditional means (moment-parity tests); 0: normal sampling. */
int hmsc_set_noise_mode(hmsc_state* s, int32_t mode);

/* The sweep loop with recording: for iter in 1..transient+samples*thin, record when
 * iter>transient and (iter-transient)%%thin==0 (R/sampleMcmc.R:219-315).
 * adaptNf[r] = hM adaptNf.  `rec` may be NULL (no recording). */
int hmsc_run(hmsc_state* s, int32_t transient, int32_t samples, int32_t thin,
             const int32_t* adaptNf, int32_t iter0, hmsc_record* rec);

/* hmsc_run with R's progress print every `verbose` sweeps
 * ("Chain %d, iteration %d of %d, (%s)", R/sampleMcmc.R:317-324). */
int hmsc_run_verbose(hmsc_state* s, int32_t transient, int32_t samples, int32_t thin,
                     const int32_t* adaptNf, int32_t iter0, int32_t verbose, int32_t chain,
                     hmsc_record* rec);

/* Live kernel timing with HIP events on the chain's stream (bench / roofline):
 * id 0 = fused updateZ kernel, 1 = updateEta Z-pass, 2 = batched BetaLambda solve,
 * 3 = per-unit Eta solve, 4 = whole sweep, 5 = spatial updateEta (dense system), 6 = its
 * blocked Cholesky, 7 = updateAlpha, 8 = updateGammaEta, 9 = updateRho, 10 = updatewRRR's pass
 * over Z (rrr.hip), 11 = updateBetaSel (betasel.hip).  hmsc_profile(s,1) clears and enables. */
int hmsc_profile(hmsc_state* s, int32_t enable);
int hmsc_profile_get(hmsc_state* s, int32_t id, double* total_ms, int32_t* count);

/* Live launch timing measured inside the kernels (bench.py's roofline figure): every
 * workgroup reads the constant-rate wall clock when it starts and finishes; a launch's
 * duration is its last finish minus its first start, kept per sweep (graph replays
 * included; up to 8192 sweeps per window).  id 0 = updateZ kernel, 1 = fused updateEta
 * kernel, 2 = BetaLambda wave kernel.  hmsc_kernel_timing(s,1) clears and enables (0
 * disables); _get returns the summed duration (us) and the number of timed launches.
 * No reference counterpart: instrumentation of this port. */
int hmsc_kernel_timing(hmsc_state* s, int32_t enable);
int hmsc_kernel_timing_get(hmsc_state* s, int32_t id, double* total_us, int32_t* count);

/* ---- post-sampling statistics on the device ----
 * Reductions over posterior samples that return only their summaries; every sum is in a
 * fixed order, so results repeat bit for bit. */

/* computeAssociations (R/computeAssociations.R) and getPostEstimate(hM, "Omega")
 * (R/getPostEstimate.R) for one random level: Lambda holds S samples of nfmax x ns
 * (column-major each; factors h >= nf[s] ignored).  Outputs ns x ns: the mean of
 * cov2cor(Lambda_s' Lambda_s), its support mean(> 0), and for Omega_s = Lambda_s' Lambda_s the
 * posterior mean and mean(Omega_s < 0). */
int hmsc_post_omega(int32_t device, int32_t S, int32_t ns, int32_t nfmax, const int32_t* nf,
                    const double* Lambda, double* mean_cor, double* support, double* support_neg,
                    double* mean_omega);

/* computeVariancePartitioning (R/computeVariancePartitioning.R:37-204; X a matrix): the
 * caller passes the S samples the reference loops over (its quirk: `for (i in 1:hM$samples)`
 * over the pooled list, i.e. the first chain when nChains > 1), cM = cov(hM$X), and the group
 * of every covariate (1-based).  out (nc + 1 + ns (1 + nr + ngroups) doubles):
 * R2T.Beta (nc) | R2T.Y | fixed (ns) | random (nr x ns) | fixedsplit (ngroups x ns),
 * all already averaged over the samples; vals = fixed * fixedsplit and random follow on the host. */
typedef struct hmsc_vp_args {
  int32_t device, ny, ns, nc, nt, S, ngroups, nr;
  const int32_t* group;     /* nc */
  const double* X;          /* ny x nc  hM$X */
  const double* Tr;         /* ns x nt  hM$Tr */
  const double* cM;         /* nc x nc  cov(hM$X) */
  const double* Beta;       /* S x (nc x ns) */
  const double* Gamma;      /* S x (nc x nt) */
  const int32_t* nf;        /* nr x S: factors of level r in sample s at [r S + s] */
  int32_t nfmax[HMSC_MAX_LEVELS];
  const double* Lambda[HMSC_MAX_LEVELS];  /* S x (nfmax_r x ns) */
} hmsc_vp_args;
int hmsc_variance_partitioning(const hmsc_vp_args* args, double* out);

/* coda::effectiveSize of each column of x (n x p, column-major; one chain): n var / spec0
 * with spectrum0.ar (AR order by AIC up to min(n - 1, 10 log10 n), Yule-Walker by
 * Levinson-Durbin).  ess[p]; order[p] (may be NULL) the chosen AR orders. */
int hmsc_effective_size(int32_t device, int32_t n, int32_t p, const double* x, double* ess, int32_t* order);

/* Convergence diagnostics of Omega = Lambda' Lambda for one random level, per species pair
 * (coda::effectiveSize and the moments of gelman.diag on convertToCodaObject(m)$Omega[[r]],
 * R/convertToCodaObject.r:184-188), without the ns^2 x samples matrix: the series
 * w_ij(s) = sum_{h < nf} lambda_hi lambda_hj (an fma chain in ascending h) are formed on the
 * device for the pairs i <= j and never leave it.
 *   nf, Lambda   nchains chains of n samples each, in order: nf[c n + s], and Lambda as
 *                hmsc_post_omega's (nfmax x ns column-major per sample; factors h >= nf ignored)
 *   scratch_bytes  bound of the device slab that holds the series of a run of whole species
 *                columns j (j + 1 pairs of n doubles each); 0 = 1 GiB.  It must hold the widest
 *                column (ns n doubles).  No output depends on it.
 *   ess, mean, var  nchains stacked ns x ns (column-major, symmetric): per chain the ESS of
 *                hmsc_effective_size on the pair's series, its mean and its variance (ddof = 1)
 *   order        nchains x ns x ns chosen AR orders (may be NULL)
 *   series       debug (may be NULL, at most 2^28 doubles): nchains x npairs x n, the series
 *                themselves, pair p = i + j (j + 1) / 2 (i <= j) of chain c at [(c npairs + p) n]
 * Fails by name for n < 3, nfmax > 128 (HMSC_KCAP), an nf outside 1..nfmax, a scratch_bytes
 * below one column, and a call beyond the device's free memory (bytes needed and bytes free).
 * Results repeat bit for bit.  hmsc_debug_omega_diag_timing: ms of this thread's last call --
 * the whole call (host clock), the series kernel and the ESS kernel (device events summed over
 * the slabs; -1 for a call of more than 256 slabs, which is not timed). */
int hmsc_omega_diagnostics(int32_t device, int32_t nchains, int32_t n, int32_t ns, int32_t nfmax,
                           const int32_t* nf, const double* Lambda, uint64_t scratch_bytes, double* ess,
                           double* mean, double* var, int32_t* order, double* series);
int hmsc_debug_omega_diag_timing(double out[3]);

/* evaluateModelFit (R/evaluateModelFit.R:53-169) for all species in one call.  Y, m and pO are
 * ny x ns host matrices, column-major (a species' rows contiguous): Y the data (NaN = NA), m the
 * per-cell posterior mean (the median in Poisson columns), pO the share of positive draws (read
 * in Poisson columns only; may be NULL when there is none).
 *   family         ns: 1 normal, 2 probit, 3 Poisson
 *   chunk_rows     rows ranked per LDS sort: 0 = the kernel's capacity (16384); a smaller value
 *                  forces the multi-chunk path.  No output depends on it.
 *   scratch_bytes  bound of the device slab (a run of whole species: their input columns and
 *                  3 ny doubles of rank scratch each); 0 = 1 GiB.  No output depends on it.
 *   out            10 x ns, measure k of species j at [k ns + j], k in the order RMSE, R2, AUC,
 *                  TjurR2, SR2, O.AUC, O.TjurR2, O.RMSE, C.SR2, C.RMSE; NaN where the measure
 *                  does not apply to the species' family
 * RMSE family: sqrt of the mean of (a - b)^2 over the rows where that is not NaN.  R2 / SR2 /
 * C.SR2: sign(co) co^2 of the two-pass Pearson correlation (of the average ranks for the two
 * Spearman ones) over the pairwise-complete rows, NaN below 2 rows or at zero variance.  AUC /
 * O.AUC: (R1 - n1 (n1 + 1) / 2) / (n1 n0) from the average ranks of the predictions over the
 * rows with Y not NaN, classes 1[Y > 0]; NaN unless both classes occur and no such prediction
 * is NaN.  TjurR2: mean of m where Y == 1 minus its mean where Y == 0 (O.TjurR2: pO, Y > 0
 * against the other rows with Y not NaN).  C.*: Y with 0 -> NA against m / pO.
 * Fails by name for a NULL argument, ny < 1 or ns < 1, a family outside 1..3, pO NULL while a
 * Poisson column exists, a scratch_bytes below one species' need, and a call beyond the
 * device's free memory.  Every sum runs in one fixed order: results repeat bit for bit.
 * hmsc_debug_model_fit_timing: ms of this thread's last call -- the whole call (host clock),
 * the uploads and the kernels (device events summed over the slabs; -1 beyond 256 slabs). */
typedef struct hmsc_model_fit_args {
  int32_t device, ny, ns;
  const double* Y;          /* ny x ns */
  const double* m;          /* ny x ns */
  const double* pO;         /* ny x ns, or NULL */
  const int32_t* family;    /* ns */
  int32_t chunk_rows;
  uint64_t scratch_bytes;
} hmsc_model_fit_args;
int hmsc_model_fit(const hmsc_model_fit_args* args, double* out);
int hmsc_debug_model_fit_timing(double out[3]);

/* Wait for all device work of this chain; fails (-1 not positive definite, -5 a timed-out
 * in-launch handshake) if any of it raised a device error flag. */
int hmsc_sync(hmsc_state* s);

/* Capture (without running) the steady-state sweep graphs that hmsc_run replays, so a
 * caller that times hmsc_run (bench.py) does not pay for stream capture and
 * hipGraphInstantiate inside its timed region.  `iter` is the next sweep index the caller
 * will run (the Philox counters of a replay are set per launch, so any value works).
 * *built = 1 when the graphs exist afterwards; 0 when the chain is not in a steady state
 * yet (no eager sweep since the last init / set_state / updateNf repack), is sharded, or
 * graphs are disabled (HMSC_NO_GRAPH, profiling) -- hmsc_run then captures on its own.
 * No reference counterpart: the R loop has no launch overhead to amortise. */
int hmsc_prepare_graphs(hmsc_state* s, int32_t iter, int32_t* built);

/* The blocked device Cholesky (dense.hip) on one host matrix, for tests: A (n x n,
 * column-major, lower triangle read) is overwritten by L (A = L L^T; the strict upper
 * triangle is scratch), b (may be NULL) by A^-1 b through L^-T L^-1; *info = 1 if A is not
 * positive definite.  Instrumentation of this port, no reference counterpart. */
int hmsc_dense_chol_solve(int32_t device, double* A, int32_t n, double* b, int32_t* info);

/* computeDataParameters' 'Full' grid (R/computeDataParameters.R:53-81) on the device, for
 * np units given by coordinates (np x sdim, column-major) or a distance matrix (np x np;
 * coords NULL) over the G grid values alphas: iWg, RiWg (np*np*G) and detWg (G) exactly as
 * hmsc_model takes them, RiWg = chol(W_g)^-1 lower triangular.  This is what hmsc_create
 * runs for a 'Full' level passed by sCoord / distMat. */
int hmsc_spatial_full_grid(int32_t device, int32_t np, int32_t sdim, const double* coords, const double* dist,
                           int32_t G, const double* alphas, double* iWg, double* RiWg, double* detWg);

/* Copy a named internal device buffer (fp64) for tests / profiling:
 * "Z", "E", "XEtaTZ", "Gram", "ZTr", "BL", "BL_prec" ... ; n = element count.  With variable
 * selection: "BLx" (the masked BL), "BetaSelLogRatio" (sum(selNg): lldif + pridif of the last
 * updateBetaSel, as evaluated) and "BetaSelScale" (the sum of the absolute values of the terms
 * that entered each lldif). */
int hmsc_debug_get(hmsc_state* s, const char* name, double* out, int64_t n);

/* Test hook: corrupt one in-launch handshake of this chain so the next launch that uses it
 * times out (about 1 s) and reports: "trsv_ticket" (the sync-free triangular solve's block
 * ticket) or "chol_publish" (the blocked Cholesky's fused panel flag, withheld once).  The next
 * hmsc_run / hmsc_sync / hmsc_get_state then fails with code -5 ("... handshake timed out").
 * Instrumentation of this port, no reference counterpart. */
int hmsc_debug_poison(hmsc_state* s, const char* what);

/* Test hook: the device resources this library holds in the process right now, over all chains
 * and calls: out = {device buffers, pinned host buffers, streams, events}.  After hmsc_destroy,
 * a failed hmsc_create or any one-shot call the counts are back where they were before it.
 * Instrumentation of this port, no reference counterpart. */
int hmsc_debug_live_resources(int64_t out[4]);

/* Test hook: evaluate one scalar function of the draws on the device, elementwise over n host
 * values (one plain kernel; inputs copied up, results copied back), so tests can hold the
 * device code of each function to a high-precision reference of its own:
 *   "trunc_normal"       rng.h trunc_normal_lower(alpha, u)       in0 alpha, in1 u -> out0 x
 *   "trunc_normal_tab"   the z kernel's table draw (z_kernel.h)   in0 alpha, in1 u -> out0 x
 *   "trunc_normal_poly"  the z kernel's polynomial pair draw      in0 alpha, in1 u -> out0 x
 *   "qnorm"              qnorm_fast(p)                            in0 p -> out0 q
 *   "erfc"               erfc_fast(z)                             in0 z -> out0 erfc(z)
 *   "log"                log_fast(x)                              in0 x -> out0 log x
 *   "exp_small"          exp_small(x)                             in0 x -> out0 exp x
 *   "pg_moments"         pg_moments(b, c)                         in0 b, in1 c -> out0 mean, out1 var
 *   "log_pnorm"          waic_math.h log_pnorm(x) (hmsc_waic)     in0 x -> out0 log Phi(x)
 * For the two pair draws elements 2k and 2k + 1 are drawn as one pair of cells, as the z kernel
 * draws two species of a site: e = -alpha, sd = 1, code 1 (alpha = -inf: an NA cell), x = z - e.
 * Arguments a function does not use may be NULL.  Instrumentation of this port, no reference
 * counterpart. */
int hmsc_debug_eval(int32_t device, const char* what, int64_t n, const double* in0, const double* in1,
                    double* out0, double* out1);

/* predict.Hmsc (R/predict.R:1-231) for a pooled posterior: every sample's
 * L = X Beta + sum_r Eta_r[Pi_r,] Lambda_r, then expected values (pnorm / exp(L + sigma/2) / L)
 * or draws (1[L + sqrt(sigma) e > 0] / rpois / L + sqrt(sigma) e), then the YScalePar
 * back-transform.  Replaces the per-sample loop of R/predict.R:143-229; the caller (the R
 * wrapper) keeps predictLatentFactor (R/predict.R:120-129) and passes the per-sample Eta rows
 * of the prediction units.  Arrays are sample-major stacks of R's column-major matrices. */
typedef struct hmsc_predict_args {
  int32_t ny, ns, nc, nr, nsamples;
  int32_t expected;       /* R's `expected` */
  uint64_t seed;          /* Philox key of the draws (expected = 0) */
  int32_t device;
  const double* X;        /* ny*nc  (unscaled X, as post holds un-scaled Beta) */
  const double* Beta;     /* nsamples*nc*ns */
  const double* sigma;    /* nsamples*ns */
  const int32_t* family;  /* ns: hM$distr[,1] */
  const double* YScalePar;/* 2*ns */
  const int32_t* Pi;      /* ny*nr, 1-based rows of the per-level Eta */
  const int32_t* np;      /* nr */
  const int32_t* nf;      /* nr */
  const double* Eta[HMSC_MAX_LEVELS];     /* nsamples*np[r]*nf[r] */
  const double* Lambda[HMSC_MAX_LEVELS];  /* nsamples*nf[r]*ns */
} hmsc_predict_args;

/* out: nsamples*ny*ns (pred[[s]] column-major, sample-major stack) */
int hmsc_predict(const hmsc_predict_args* args, double* out);

/* Posterior predictive summaries of hmsc_predict's values without the nsamples*ny*ns stack: per
 * cell (i, j), over the samples s = 0 .. nsamples - 1 in order,
 *   n     the number of values that are not NaN (a Poisson draw of an overflowing rate is NaN)
 *   mean  their sum / n, the sum taken by sequential fp64 adds in sample order (NaN when n = 0)
 *   occ   the share of them that is > 0 (NaN when n = 0)
 * and, for the species columns flagged in qcols, R's type-7 quantiles (quantile(x, p, na.rm = TRUE))
 * at nq probabilities: h = (n - 1) p, lo = x_(floor h), hi = x_(ceil h) (0-based order statistics of
 * the non-NaN values), result lo + (h - floor h) (hi - lo), lo itself where hi = lo.  This is what
 * evaluateModelFit (R/evaluateModelFit.R: the mean, the median of Poisson columns, the share of
 * positive draws) and credible intervals of predictions take from computePredictedValues' array.
 *
 * p is hmsc_predict's argument block, unchanged, with the same limits (nc + sum(nf) <= 128,
 * ny ns < 2^32).  Every value is formed as hmsc_predict forms it -- the same fma chain, cell
 * index and Philox counters -- so for one seed a summarised value is the double hmsc_predict
 * writes, and n, occ n and the order statistics equal those of its output exactly.
 *
 * Layouts.  mean, occ (double) and n (int32): ny x ns column-major.  quant: nq stacked ny x ns
 * column-major matrices in the order of probs, NaN in columns that are not flagged and in cells
 * with n = 0; may be NULL with nq = 0.
 *
 * Memory.  The flagged columns' values are kept for the selection in a device slab of
 * nsamples * 8 bytes per cell, at most scratch_bytes (0: 1 GiB); the sites are walked in slabs of
 * whole 64-row tiles.  No sum crosses a workgroup and selection is exact: every output is
 * bit-equal for every scratch_bytes and from call to call.
 *
 * Errors (hmsc_last_error): those of hmsc_predict; nq outside 0 .. 8; a probability outside
 * [0, 1]; nsamples < 1; one 64-row tile of the flagged columns (nsamples * 64 * columns * 8 bytes)
 * larger than scratch_bytes (the message names the bytes needed). */
typedef struct hmsc_summary_args {
  int32_t nq;               /* 0..8 */
  const double* probs;      /* nq */
  const int32_t* qcols;     /* ns: 1 = this species column gets the quantiles (NULL with nq = 0) */
  uint64_t scratch_bytes;   /* 0 = chosen by the library */
} hmsc_summary_args;

/* q may be NULL (no quantiles) */
int hmsc_predict_summary(const hmsc_predict_args* p, const hmsc_summary_args* q, double* mean, double* occ,
                         int32_t* n, double* quant /* nq*ny*ns, may be NULL */);

/* Instrumentation: host-clock milliseconds of this thread's last hmsc_predict_summary -- allocation
 * and uploads, the summary kernel(s), the quantile kernel(s) with the copy back. */
int hmsc_debug_summary_timing(double out[3]);

/* Community-level posterior summaries in one device pass: weighted sums over a sample's whole row of
 * species (species richness, the summed response, community-weighted trait means) and their
 * statistics over the samples -- plotGradient's numbers for measures "S", "Y" and "T"
 * (R/plotGradient.R:93-138) without the ny x ns x nsamples array.  The quantile of a sum is not the
 * sum of quantiles, so these cannot be had from hmsc_predict_summary.
 *
 * p is hmsc_predict's argument block, unchanged, with the same limits.  For sample s, site i and
 * column m let p_j be the double hmsc_predict writes for cell (i, j) of sample s for the same
 * block and seed (the same fma chain, cell index i + ny j and Philox counters), and g the
 * transform (0: identity; 1: exp, plotGradient's rule for an all-normal model).  Then
 *   num_m      = sum over j with W[j, m] != 0 of g(p_j) W[j, m]
 *   den        = sum over j of g(p_j)
 *   C[s, i, m] = normalise[m] ? num_m / den : num_m.
 * A zero weight leaves the species out of that column's numerator: a select, not a product, so a
 * unit-vector column returns that one species' values whatever the others hold (R's NaN * 0 is
 * NaN).  NaN and inf otherwise propagate as IEEE sums and quotients do: a NaN Poisson draw makes
 * that sample's sums NaN, as rowSums does; 0 / 0 is NaN.
 *
 * Summation order (it depends on ns alone; not on ny, the slab, the sample count or the launch):
 * four partial sums l = 0 .. 3 per site, partial l over the species j with j mod 4 = l in
 * ascending j, each from 0.0 by one fp64 add per species (for num: of the rounded product
 * g(p_j) W[j, m], skipped where W[j, m] = 0); then ((s_0 + s_1) + s_2) + s_3.
 *
 * Outputs, over the samples in order, per site and column:
 *   n      (int32, ny x nw column-major) the samples whose C is not NaN
 *   mean   (ny x nw) their sum by sequential fp64 adds in sample order, / n; NaN at n = 0
 *   quant  (nq stacked ny x nw matrices) R's type-7 quantiles of the non-NaN values, as
 *          hmsc_predict_summary defines them; NaN at n = 0; may be NULL with nq = 0
 *   pr     (npairs x nw column-major) for the 0-based site pair (a, b) = pairs[2 k], pairs[2 k + 1]
 *          the share of samples with C[s, b, m] > C[s, a, m]; NaN if either value is NaN in any
 *          sample (R's mean(x[b, ] > x[a, ]) is NA); may be NULL with npairs = 0
 *   comm   (nsamples stacked ny x nw column-major matrices) C itself; may be NULL
 *
 * Memory.  C is kept for the statistics in a device slab of nsamples * 8 bytes per site and
 * column, at most scratch_bytes (0: 1 GiB); the sites are walked in slabs of whole 64-row tiles.
 * No sum crosses a workgroup and selection is exact: every output is bit-equal for every
 * scratch_bytes and from call to call.  A pair may straddle two slabs.
 *
 * Errors (hmsc_last_error): those of hmsc_predict; NULL arguments; nw outside 1 .. 16; nq > 8; a
 * probability outside [0, 1]; npairs > 8; a pair index outside 0 .. ny - 1; nsamples < 1 or above
 * 2^23; one
 * 64-row tile (nsamples * 64 * nw * 8 bytes) larger than scratch_bytes (the message names the
 * bytes needed). */
typedef struct hmsc_community_args {
  int32_t nw;                /* 1..16 columns */
  const double* W;           /* ns x nw column-major weights */
  const int32_t* normalise;  /* nw: 1 = divide the column by the row's sum of g(p_j) */
  int32_t transform;         /* 0 identity, 1 exp */
  int32_t nq;                /* 0..8 */
  const double* probs;       /* nq */
  int32_t npairs;            /* 0..8 */
  const int32_t* pairs;      /* 2 x npairs: (a, b) per pair, 0-based sites */
  uint64_t scratch_bytes;    /* 0 = chosen by the library */
} hmsc_community_args;

int hmsc_predict_community(const hmsc_predict_args* p, const hmsc_community_args* c, int32_t* n, double* mean,
                           double* quant /* nq*ny*nw, may be NULL */, double* pr /* npairs*nw, may be NULL */,
                           double* comm /* nsamples*ny*nw, may be NULL */);

/* Instrumentation: host-clock milliseconds of this thread's last hmsc_predict_community --
 * allocation and uploads, kernel A, the statistics kernel(s) with the copy back and the pairs. */
int hmsc_debug_community_timing(double out[3]);

/* predictLatentFactor's kriging of the new units of one spatial random level
 * (R/predictLatentFactor.R:59-160) for a pooled posterior, on the device.  The caller keeps the
 * unit bookkeeping (:35-58, which units are new, their coordinates or distMat rows) and passes
 * the np fitted units followed by the nn new ones.
 *
 * Layouts.  coords: (np + nn) x sDim column-major, fitted units (in the row order of Eta) then new
 * units; or dist: the (np + nn) x (np + nn) distance matrix in that unit order (coords NULL).
 * alphas: the G values alphapw[, 1].  Eta: S stacked np x nfmax column-major matrices; a sample
 * with fewer factors is zero padded.  alpha: S x nfmax, alpha[s * nfmax + h] the 1-based grid
 * index of factor h of sample s, 0 for "no such factor" (its output stays 0).  out: S stacked
 * nn x nfmax column-major matrices, the new units in the order given.
 *
 * mode 0 predictMean (:62-77): out = K12' K11^-1 eta.
 * mode 1 predictMeanField (:78-85): ... + sqrt(1 - colSums((L^-1 K12)^2)) z, L = chol(K11)'.
 * mode 2 'Full' (:95-117): ... + chol(K22 - K12' K11^-1 K12)' z, jointly over the new units.
 * mode 3 'NNGP' (:118-160): per new unit over its nNeighbours (<= 32) nearest fitted units,
 *   ties to the lower index: w = K11^-1 K12, out = w' eta[ind] + sqrt(1 - w' K12) z.  Needs coords.
 * mode 4 'GPP' (:161-203): the predictive process over the nK knots (knots: nK x sDim column-major,
 *   its own array).  Per sample the grid value a of its LAST factor (the last non-zero entry of its
 *   alpha row; R's ag = alpha[nf]) serves every factor.  With Wss, W12, Wns = exp(-d / a) between
 *   knots, fitted units and knots, new units and knots: iWss = Wss^-1, dD = 1 - rowSums((W12 iWss) o
 *   W12), F = Wss + W12' diag(1 / dD) W12, iF = F^-1, R = chol(iF) (upper), and
 *   out[, h] = Wns (iF W12' (eta_h / dD) + R z_knot(., h)) + sqrt(max(dDn, 0)) z(., h),
 *   dDn = 1 - rowSums((Wns iWss) o Wns).  The knot innovation keeps R's literal R z_knot (covariance
 *   R R', not iF).  z_knot of knot k (0-based), factor h, sample s is normal(seed, k, h,
 *   32 + 256 * level, s).  The nn x nK matrix Wns is never stored: the call's GPP workspace beyond the
 *   plan (3 nK^2 + np nK + np (1 + c) + 2 nK c doubles) is nK^2 + nK c + nn doubles.  Needs coords and
 *   knots: refused by name with dist or nK = 0.  A fitted unit that lies on a knot (or has dD <= 0)
 *   is an error naming the unit and the grid value; a new unit on a knot has dDn = 0.  A Wss, F or
 *   iF that is not positive definite is an error naming the matrix and the grid index.
 * A factor at a grid value 0 gets out = z (:86-91, :113-115, :157-159, :199-201), 0 with mode 0.
 *
 * Counter contract: z of new unit i (0-based position among the new units), factor h (0-based)
 * and sample s is normal(key = seed, idx = i, sub = h, stream = 31 + 256 * level, iter = s) of
 * rng.h -- independent of how the (s, h) pairs are grouped by grid index, of the tiling and of the
 * other pairs of the call.  Every sum has a fixed order: equal arguments give bit-equal output.
 *
 * Errors (hmsc_last_error): a K11 or K22 - K12' K11^-1 K12 that is not positive definite (R's
 * chol stops there too), a grid index above G, nNeighbours > 32, mode 3 without coordinates, and
 * a device that cannot hold np^2 + np (nn + c) + nn^2 doubles and the workspaces (c = the
 * largest number of (s, h) pairs sharing a grid index; the message names the bytes).
 * kernel_ms (may be NULL): 8 doubles, the milliseconds spent in the kernel matrices, the K11
 * factorization, the triangular solve, the mean product, the W product, the W factorization, the
 * L_W Z product and the NNGP kernel, summed over the grid indices (instrumentation).  Mode 4 fills
 * slot 0 (Wss and W12), 1 (iWss), 2 (the dDn pass over the new units), 3 (the slab product with the
 * output), 4 (dD and F), 5 (iF and chol(iF)) and 6 (C = mu + eps); slot 7 stays 0. */
typedef struct hmsc_krige_args {
  int32_t device, np, nn, sDim, G, S, nfmax;
  int32_t mode;           /* 0 predictMean, 1 predictMeanField, 2 'Full', 3 'NNGP', 4 'GPP' */
  int32_t nNeighbours;    /* mode 3 */
  int32_t level;          /* index r of the random level: offsets the Philox stream */
  uint64_t seed;          /* Philox key of the draws */
  const double* coords;   /* (np + nn) * sDim, or NULL */
  const double* dist;     /* (np + nn)^2, or NULL */
  const double* alphas;   /* G */
  const double* Eta;      /* S * np * nfmax */
  const int32_t* alpha;   /* S * nfmax */
  double* kernel_ms;      /* 8, or NULL */
  const double* knots;    /* mode 4: nK * sDim, column-major; else NULL */
  int32_t nK;             /* mode 4: the number of knots; else 0 */
} hmsc_krige_args;

/* out: S * nn * nfmax */
int hmsc_krige(const hmsc_krige_args* args, double* out);

/* Prediction maps: a pooled posterior mapped onto ny new rows (a raster of 10^5 - 10^6 cells) in
 * one call -- predictLatentFactor for the rows' units (hmsc_krige's arithmetic), predict's values
 * and their per-cell (hmsc_predict_summary) and community-level (hmsc_predict_community) summaries
 * -- walked in slabs of prediction rows.  The latent factors of a slab's units are produced on the
 * device and consumed there; they never exist on the host.  In the reference this is
 * prepareGradient -> predict(Gradient =, predictEtaMean = TRUE) -> row sums and means.
 *
 * Per random level r (hmsc_map_level): the np fitted units with their posterior Eta (S stacked
 * np x nf column-major matrices, zero padded to nf factors) and nn new units.  unit[i] in
 * 1 .. np + nn names the unit of prediction row i: 1 .. np a fitted unit (its row of Eta),
 * np + 1 + k the k-th new unit, which is row np + k of coords / dist and index k of hmsc_krige's
 * counter contract for the whole call.  coords, dist, alphas (G), alpha (S x nf, 1-based grid
 * indices, 0: no such factor), mode and nNeighbours are hmsc_krige_args' fields.  A non-spatial
 * level is the one-point grid alphas = {0} without coords and dist: its new units get z of the
 * counter contract, 0 with mode 0.
 *
 * Slabs.  The rows are walked in slabs of slab_rows rows (0: the largest multiple of 64 whose
 * scratch -- nsamples * 8 bytes per row for every flagged summary column, every community column
 * and every factor -- fits scratch_bytes, 0 meaning 1 GiB).  Per slab and level the distinct units
 * the slab's rows refer to, in ascending order (fitted units first), form the slab's Eta table: S
 * stacked units x nf column-major matrices, filled from the posterior Eta (fitted units), z or 0
 * (new units at a grid value 0) and the kriging of the slab's new units (grid values > 0, modes 0,
 * 1 and 3), with a slab-local Pi.  What depends on the fitted units alone -- per distinct grid
 * value in use K11, its Cholesky factor and Y = L^-1 E -- is built once per call and stays
 * resident.  A unit that several slabs refer to is recomputed in each; every value is a sum in a
 * fixed order with counters of (unit, factor, level, sample), so it is the same double each time,
 * and every output is bit-equal to that of hmsc_krige followed by hmsc_predict_summary /
 * hmsc_predict_community for the same seed, for every slab_rows.  Mode 2 ('Full') draws the new
 * units jointly and is served when every slab that holds new units of the level holds all of them.
 * Mode 4 ('GPP') keeps iWss and C = mu + eps per grid value in use (nK^2 + nK c doubles) and serves
 * any slab: given the knot draw the new units are conditionally independent, so there is no
 * condition on how they fall across slabs, and a slab's GPP workspace is one double per new unit.
 *
 * Cell (i, j) of the map has the counters of cell i + ny j of hmsc_predict; ny * ns < 2^32.
 *
 * Outputs (hmsc_map_out; each may be NULL when its block is absent): mean, occ, n and quant as
 * hmsc_predict_summary's (cells = 1); per community block b < ncomm its n, mean and quant as
 * hmsc_predict_community's.  pairs and comm are not served on maps (npairs must be 0).
 *
 * Memory.  factor_bytes bounds the resident factors, Y, the posterior Eta, the geometry and one
 * slab's kriging workspace and Eta tables (0: what the device reports free, less the summaries'
 * scratch and outputs); a call that needs more is refused with both byte counts in the message.
 *
 * Errors (hmsc_last_error): those of hmsc_predict_summary, hmsc_predict_community and hmsc_krige;
 * a unit outside 1 .. np + nn; a 'Full' level whose new units are spread over slabs; the budget. */
typedef struct hmsc_map_level {
  int32_t np, nn, nf;
  int32_t sDim, G;
  int32_t mode;            /* hmsc_krige's: 0 predictMean, 1 predictMeanField, 2 'Full', 3 'NNGP', 4 'GPP' */
  int32_t nNeighbours;     /* mode 3 */
  const int32_t* unit;     /* ny, 1-based */
  const double* coords;    /* (np + nn) * sDim, or NULL */
  const double* dist;      /* (np + nn)^2, or NULL */
  const double* alphas;    /* G */
  const int32_t* alpha;    /* nsamples * nf */
  const double* Eta;       /* nsamples * np * nf */
  const double* Lambda;    /* nsamples * nf * ns */
  const double* knots;     /* mode 4: nK * sDim, column-major; else NULL */
  int32_t nK;              /* mode 4 */
} hmsc_map_level;

typedef struct hmsc_map_args {
  int32_t ny, ns, nc, nr, nsamples;
  int32_t expected;
  uint64_t seed;           /* Philox key of predict's draws and of the new units' */
  int32_t device;
  const double* X;         /* ny*nc */
  const double* Beta;      /* nsamples*nc*ns */
  const double* sigma;     /* nsamples*ns */
  const int32_t* family;   /* ns */
  const double* YScalePar; /* 2*ns */
  hmsc_map_level level[HMSC_MAX_LEVELS];
  int32_t cells;           /* 1: the per-cell summaries (ny x ns outputs) */
  hmsc_summary_args summary;        /* its scratch_bytes is not used */
  int32_t ncomm;           /* 0..2 community blocks (one per transform) */
  hmsc_community_args community[2]; /* npairs = 0; scratch_bytes not used */
  int32_t slab_rows;       /* 0 = derived from scratch_bytes */
  uint64_t scratch_bytes;  /* 0 = 1 GiB */
  uint64_t factor_bytes;   /* 0 = what the device has free */
} hmsc_map_args;

typedef struct hmsc_map_out {
  double* mean;            /* ny*ns */
  double* occ;             /* ny*ns */
  int32_t* n;              /* ny*ns */
  double* quant;           /* nq*ny*ns */
  int32_t* cn[2];          /* ny*nw */
  double* cmean[2];        /* ny*nw */
  double* cquant[2];       /* nq*ny*nw */
} hmsc_map_out;

int hmsc_predict_map(const hmsc_map_args* args, const hmsc_map_out* out);

/* Instrumentation: milliseconds of this thread's last hmsc_predict_map, summed over the slabs:
 * the plan (uploads, K11, its factor, Y), the K12 slabs, the triangular solves, the mean products
 * (with the NNGP kernel and a 'Full' level's whole group), the Eta tables' assembly, the summary
 * kernel, the community kernel, the quantile / statistics kernels, the copy back.  K12, trsm and
 * mean are device times between events, the others host-clock times around a synchronisation.  A
 * mode-4 level adds its plan (iWss, F, iF, chol(iF), C) to slot 0, its dDn pass to slot 1 (K12) and
 * its slab product to slot 3 (mean); it adds nothing to slot 2. */
int hmsc_debug_map_timing(double out[9]);

/* computeWAIC (R/computeWAIC.R:25-131) for a pooled posterior, in one pass on the device:
 *   val[s, i] = sum_j log p(y_ij | sample s), with E = X Beta + sum_r Eta_r[Pi_r,] Lambda_r and
 *     normal   dnorm(y, E, sigma^(-1/2), log = TRUE)
 *     probit   y log Phi(E) + (1 - y) log Phi(-E)
 *     Poisson  log(pi^(-1/2) sum_g w_g dpois(y, exp(E + sqrt(2) x_g sigma^(-1/2))))
 *   (NA cells 0), then per site Bl_i = -log mean_s exp(val[s, i]), V_i = var_s val[s, i] (ddof 1)
 *   and WAIC = mean_i (Bl_i + V_i).
 * Arrays as in hmsc_predict_args: sample-major stacks of R's column-major matrices, 1-based Pi; a
 * covariate-dependent level is one level per column of rL$x with Eta * x[, k] formed by the
 * caller.  K = nc + sum(nf) <= 128 (HMSC_KCAP), nsamples >= 2.
 *
 * Unlike the reference, which exponentiates val and the Poisson cell likelihoods as they are
 * (:111-112, :124: Inf / -Inf once a site's log-likelihood passes -745), both sums are taken
 * max-shifted; they equal the literal form to rounding wherever that is finite.  log Phi keeps
 * its relative accuracy on the whole line.
 *
 * For a Poisson column the y of node g is read at the recycled index (i + ny c + ny cN g) mod
 * (ny ns), c the column's rank among the cN Poisson columns, as R's dpois(Y, exp(gX)) recycles Y
 * (the cell's own y when every column is Poisson); dpois is 0 off the non-negative integers.
 *
 * The per-sample stacks are uploaded sample_chunk samples at a time (0: chosen by the library);
 * val (nsamples x ny) stays on the device.  Every sum has a fixed order that does not depend on
 * the chunking: equal arguments give bit-equal output for every sample_chunk. */
typedef struct hmsc_waic_args {
  int32_t ny, ns, nc, nr, nsamples, ghN, device;
  int32_t sample_chunk;      /* samples resident at once; 0 = chosen by the library */
  const double* Y;           /* ny*ns  hM$Y, NaN = NA */
  const double* X;           /* ny*nc  hM$X */
  const double* Beta;        /* nsamples*nc*ns */
  const double* sigma;       /* nsamples*ns */
  const int32_t* family;     /* ns: hM$distr[,1] */
  const double *gx, *gw;     /* ghN Gauss-Hermite nodes / weights (the caller computes them) */
  const int32_t *Pi, *np, *nf;
  const double* Eta[HMSC_MAX_LEVELS];     /* nsamples*np[r]*nf[r] */
  const double* Lambda[HMSC_MAX_LEVELS];  /* nsamples*nf[r]*ns */
} hmsc_waic_args;

/* waic: the scalar.  site (may be NULL): 2*ny, Bl then V.  val (may be NULL): nsamples*ny. */
int hmsc_waic(const hmsc_waic_args* args, double* waic, double* site, double* val);

/* Instrumentation: host-clock milliseconds of this thread's last hmsc_waic -- allocation and
 * uploads, the val kernel, the per-site kernel with the mean and the copy back. */
int hmsc_debug_waic_timing(double out[3]);

/* Conditional prediction (R/predict.R:181-198) for a pooled posterior in one call: the latent
 * factors of every sample are updated given the observed part of Yc.  Per sample s this is what the
 * per-sample path computes (hmsc_set_state, then hmsc_update Z / Eta): Z = L; Z = updateZ(Yc);
 * then mcmcStep x (updateEta, updateZ) with the sample's Beta, sigma and Lambda fixed; updateEta
 * takes the levels in order and level r sees the already updated earlier levels.  The output is
 * the conditioned Eta stacks in the layout of the input stacks; the caller runs hmsc_predict on
 * them (R forms L from the conditioned Eta and discards Z, R/predict.R:188-197).
 *
 * Arrays as in hmsc_predict_args (sample-major stacks of R's column-major matrices, 1-based Pi),
 * sigma the residual variances.  Scope: non-spatial levels without unit covariates; any mix of
 * np == ny and grouped units; any NA pattern in Yc; families 1 (normal), 2 (probit) and 3 (Poisson,
 * lognormal Poisson); K = nc + sum(nf) <= 128 and nf <= 32 per level.
 *
 * Classes.  The precision of unit q of level r, Q = I + sum_j c_qj lambda_j lambda_j' / sigma_j with
 * c_qj the number of rows of q in which species j is observed, depends on q only through its count
 * vector.  The caller passes the ncls[r] distinct count vectors, cnt[r][c * ns + j], and each
 * unit's class unit_class[r][q] (0-based); Q is formed and Cholesky-factored once per (sample,
 * class) and call, and every updateEta step is two triangular solves.  The call checks cnt
 * against (Yc, Pi).
 *
 * Counter contract.  The Philox key is `seed`, as a chain's.  Sample s (0-based in the call) uses
 * the iterations it0 = 1 + s (2 mcmcStep + 1): Z at it0, then for step t = 0 .. mcmcStep - 1 Eta at
 * it0 + 1 + 2 t and Z at it0 + 2 + 2 t.  Streams and element indices are the sweep's: Z one block
 * per (site, species quad), word k the 32-bit uniform of species 4 q + k, block (i + ny q, 0, 12,
 * it); a Poisson cell the two uniforms of block (i + ny j, 0, 13, it); Eta xi = normal(unit, factor,
 * 22 + 256 r, it).  For the same key the call therefore draws what hmsc_update draws sample by
 * sample, whatever sample_chunk and the tiling are; every sum has a fixed order, so equal
 * arguments give bit-equal output for every sample_chunk.
 *
 * NA cells of Yc are neither drawn nor stored: no step in scope reads them.  A unit with no
 * observed cell gets a fresh N(0, I) draw, as in R.  nsamples == 0 returns at once; an all-NA Yc
 * returns the input Eta unchanged.
 *
 * Memory.  sample_chunk samples are resident at once (0: chosen by the library: what fits in 3/4
 * of the free device memory, the Z slab at most 16 GiB, at most 65535); one sample takes
 *   8 (ny ns + (nc + 1) ns + (K + 1) ns + sum_r nf_r (np_r + ns) + sum_r ncls_r nf_r^2) bytes
 * (the Z slab, Beta and sigma, the species-contiguous copy of the coefficients, Eta and Lambda,
 * the factors).  Launches per chunk: nr + 1 of preparation (the factors, the coefficient copy),
 * then 1 + mcmcStep (nr + 1) on one stream without a host synchronisation between them.
 *
 * Errors (hmsc_last_error): Pi out of range; nc + sum(nf) > 128; nf > 32; ny ns >= 2^32; a sigma
 * that is not finite and positive; a family outside 1 .. 3; cnt / unit_class that do not match
 * (Yc, Pi); a precision that is not positive definite; a device too small for one sample (the
 * message names the bytes). */
typedef struct hmsc_cond_args {
  int32_t ny, ns, nc, nr, nsamples;
  int32_t mcmcStep;          /* R's mcmcStep */
  int32_t device;
  int32_t sample_chunk;      /* samples resident at once; 0 = chosen by the library */
  uint64_t seed;             /* Philox key */
  const double* X;           /* ny*nc */
  const double* Beta;        /* nsamples*nc*ns */
  const double* sigma;       /* nsamples*ns */
  const int32_t* family;     /* ns: hM$distr[,1] */
  const double* Yc;          /* ny*ns, NaN = NA */
  const int32_t *Pi, *np, *nf;
  const double* Eta[HMSC_MAX_LEVELS];         /* nsamples*np[r]*nf[r]: the starting Eta */
  const double* Lambda[HMSC_MAX_LEVELS];      /* nsamples*nf[r]*ns */
  const int32_t* ncls;                        /* nr */
  const int32_t* cnt[HMSC_MAX_LEVELS];        /* ncls[r]*ns */
  const int32_t* unit_class[HMSC_MAX_LEVELS]; /* np[r], 0-based */
} hmsc_cond_args;

/* EtaOut: nr pointers, EtaOut[r] nsamples*np[r]*nf[r] (may be the input stack itself) */
int hmsc_predict_conditional(const hmsc_cond_args* args, double* const* EtaOut);

/* The same call for models with spatial 'Full' and 'GPP' levels (R/updateEta.R:110-196).  `levels`
 * is NULL (then the call is hmsc_predict_conditional) or nr entries; an entry with method 0 is a
 * level as above.  For an entry with method 1 ('Full') or 3 ('GPP'), cnt / unit_class / ncls[r] are
 * not read.
 *
 * 'Full'.
 * Per sample s and such a level r, with N = np nf unknowns in the unit-fastest order, n_q the number
 * of rows of unit q and LDL = Lambda diag(1 / sigma) Lambda':
 *   iUEta = bdiag_h(iW[AlphaIdx[s, h]]) + kron(LDL, diag(n_q)),   L L' = iUEta
 *   fS[q, h] = sum_{rows i of q} sum_j (Z_ij - L(-r)_ij) lambda_hj / sigma_j   over all species
 *   eta = L^-T (L^-1 vec(fS) + xi),   xi(q, h) = normal(q, h, 22 + 256 r, it)
 * iW[g] = W_g^-1, W_g = exp(-d / alphas[g]) (the identity for alphas[g] = 0) from the prediction
 * units' coordinates or distances, is built on the device once per call for the nalpha grid values
 * in use.  iUEta is assembled and factored once per (sample, level) and resident chunk; an Eta step
 * is the rhs, two triangular solves and the noise.  Up to N = 1024 one workgroup per sample factors
 * and solves, the samples as the grid; above, the blocked routines run sample by sample.
 *
 * 'GPP' (one row per unit, nf <= 16, nK nf <= 1024, as the chain).  idDg (np x nalpha), idDW12g (np x
 * nK x nalpha) and Fg (nK x nK x nalpha) are computeDataParameters' arrays of the conditioning model
 * for the grid values in use, column-major as hmsc_model takes them.  Once per (sample, level) and
 * chunk: B1_i = (LDL + diag_h(idD[i, g(s, h)]))^-1 and LB1_i = chol(B1_i) per unit, iAW = bdiag(B1_i)
 * bdiag_h(idDW12g[,, g(s, h)]), H = bdiag_h(Fg[,, g(s, h)]) - W' iAW and its factor L_H.  A step is
 *   eta = iA fS + iAW L_H^-T (L_H^-1 iAW' fS + xi2) + LiA xi1
 * (R's T (T' fS + xi2) with T = iAW L_H^-T), xi1(i, h) = normal(i, h, 22 + 256 r, it) and
 * xi2(k, h) = normal(k, 1024 + h, 22 + 256 r, it).
 *
 * R's spatial branch sums over all cells, so in a call with a spatial level the NA cells of Yc are
 * drawn and stored as well: Z = E + sd Phi^-1(u), u the cell's word of its (site, species quad)
 * block of stream 12 (R/updateZ.R:92), whatever the family.  The other levels of the model keep
 * their sums over the observed cells and their classes.  The counter contract is unchanged, so the
 * call draws what the per-sample path draws; output is bit-equal for every sample_chunk.
 *
 * A sample with fewer factors than nf[r] is zero-padded in Eta and Lambda; its padded factors take
 * any valid AlphaIdx (0).  Their blocks are decoupled (zero rows of LDL) and last in the order, so
 * the other factors do not depend on them.
 *
 * Memory.  Per 'Full' level 8 nalpha np^2 bytes for iW (and as much again while it is built), and per
 * resident sample 8 (N^2 + nf^2) bytes, plus 8 (64^2 ceil(N / 64) + N + 64) above N = 1024.  Per
 * 'GPP' level the uploaded arrays, and per resident sample 8 (np nf (nK nf + 2 nf) + (nK nf)^2 + nK nf
 * + nf^2) bytes.  sample_chunk = 0 sizes the chunk from the memory that is free once the grid
 * arrays are resident.  Launches per chunk: per 'Full' level 3 of preparation up to N = 1024, then
 * 2 per Eta step; per 'GPP' level 5 of preparation, then 4 per Eta step.
 *
 * Errors: method 2 ('NNGP') is refused by name; a 'GPP' level with np != ny or a unit without
 * exactly one row, nf > 16 or nK nf > 1024; an AlphaIdx outside 0 .. nalpha - 1; nalpha outside
 * 1 .. 101; a grid value that is negative or not finite; np nf > 65535 for a 'Full' level; a grid
 * matrix or a sample's system that is not positive definite (the message names sample and level);
 * a handshake timeout of the blocked routines. */
typedef struct hmsc_cond_spatial {
  int32_t method;            /* 0: not spatial, 1: 'Full', 3: 'GPP' (hmsc_model's spatialMethod codes) */
  int32_t sDim;              /* 'Full': columns of coords */
  int32_t nalpha;            /* grid values in use */
  int32_t nK;                /* 'GPP': knots */
  const double* alphas;      /* 'Full': nalpha values (alphapw[, 1] of the indices the posterior uses) */
  const double* coords;      /* 'Full': np*sDim, column-major, the level's units in Eta's order; or NULL */
  const double* dist;        /* 'Full': np*np distance matrix; or NULL (exactly one of the two is given) */
  const double *idDg, *idDW12g, *Fg; /* 'GPP': np*nalpha, np*nK*nalpha, nK*nK*nalpha */
  const int32_t* AlphaIdx;   /* nsamples*nf[r], factor fastest, 0-based into alphas */
} hmsc_cond_spatial;

int hmsc_predict_conditional_spatial(const hmsc_cond_args* args, const hmsc_cond_spatial* levels, double* const* EtaOut);

/* Instrumentation: milliseconds of this thread's last hmsc_predict_conditional -- uploads,
 * allocation and the factor launches (host clock), the Z launches and the Eta launches (device
 * events at the launch boundaries), and the copy back (host clock). */
int hmsc_debug_cond_timing(double out[4]);

#ifdef __cplusplus
}
#endif
#endif /* HMSC_AMD_H */
