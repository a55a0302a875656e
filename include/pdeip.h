/*
 * pdeip.h -- C-ABI of libpdeip.so: the MI355X (gfx950) implementation of the MEX-side
 * stencil hot path of JediZ/PDE-based-image-processing.
 *
 * Boundary.  The reference's FFI for this path is MATLAB's MEX gateway,
 *     void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]),
 * one shared object per gateway source in mex/source/ (mex/buildAll.m:5-25).  Each
 * `pdeip_<name>` host entry point below is what the body of one gateway forwards to
 * after unpacking its mxArrays; it reproduces the gateway's semantics (copy-in,
 * iter<=0 handling, residuals from the INPUT iterate, zero-initialised outputs) so the
 * MEX stub is pure unpacking.  INTEGRATION.md shows the stubs.
 *
 * Data.  Every array is MATLAB column-major float32: element (row i, col j, frame k) at
 * k*nrows*ncols + j*nrows + i.  Scalars that MATLAB passes as 1x1 singles (iter, omega,
 * solver, eps) are plain int/float here; the stub does the cast the gateway did
 * (e.g. Oflow_sor_elin4_2d.c:263-283).
 *
 * Two families of entry points:
 *   pdeip_<name>(...)      host pointers, synchronous, stateless: H2D, solve, D2H.
 *   pdeip_<name>_dev(...)  device pointers (resident in HBM), asynchronous on `stream`
 *                          (a hipStream_t passed as void*; NULL = default stream), in
 *                          place where the reference solves in place.
 *
 * All functions return PDEIP_OK or an error code; pdeip_last_error() gives the message
 * (the text a stub hands to mexErrMsgTxt).  No exceptions cross the boundary.  The
 * library keeps one lazily created context per process (device workspace cache); it is
 * thread-compatible: one call at a time.
 *
 * Sweep ordering (pdeip_set_mode):
 *   PDEIP_MODE_EXACT_ORDER  the reference's lexicographic Gauss-Seidel order, evaluated
 *                           as a pipelined tile wavefront; results are bit-identical to
 *                           the CPU restatement of the reference (default).
 *   PDEIP_MODE_RED_BLACK    red-black (5-point) / four-colour (9-point) ordering with the
 *                           same per-pixel arithmetic: the throughput and multi-GPU mode.
 *                           Converges to the same fixed point; differs at finite `iter`.
 *   PDEIP_MODE_LINE_SCAN    line relaxation (solver = 2) in the reference's line order and with
 *                           its per-line coefficients, both Thomas recurrences of a line
 *                           evaluated as a parallel scan over the workgroup.  Not bit-identical:
 *                           within 1e-4 RMS per output plane of PDEIP_MODE_EXACT_ORDER from the
 *                           first call on diagonally dominant lines, which is all the drivers
 *                           produce (NaN in the coefficient planes Cu / TRACE is handled as in the
 *                           other modes and is inside that contract).  A line that is not
 *                           diagonally dominant, or that holds non-finite iterates, is outside
 *                           it: the call returns and does not fault, its values are unspecified.
 *                           Every entry point other than line relaxation behaves exactly as in
 *                           PDEIP_MODE_EXACT_ORDER, bit for bit; no multi-GPU split.
 */
#ifndef PDEIP_H
#define PDEIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PDEIP_OK 0
#define PDEIP_ERR_ARG 1         /* null pointer, nrows/ncols < 3, nframes < 1 */
#define PDEIP_ERR_SOLVER 2      /* "no such solver" (gateway default: branch) */
#define PDEIP_ERR_UNSUPPORTED 3 /* valid request outside what the device path covers */
#define PDEIP_ERR_DEVICE 4      /* HIP runtime error / no gfx950 device */
#define PDEIP_ERR_NOMEM 5

#define PDEIP_MODE_EXACT_ORDER 0
#define PDEIP_MODE_RED_BLACK 1
#define PDEIP_MODE_LINE_SCAN 2

/* `solver` argument of the solver gateways (e.g. Oflow_sor_elin4_2d.c:328-338).  Both are device paths:
 *   1 -> GS_SOR_*      point Gauss-Seidel SOR
 *   2 -> GS_ALR_SOR_*  alternating line relaxation (the MATLAB drivers' default); in PDEIP_MODE_EXACT_ORDER the
 *        reference's line order (bit-identical, serial by construction), in PDEIP_MODE_RED_BLACK zebra order, in
 *        PDEIP_MODE_LINE_SCAN the reference's line order with each line's recurrences as a parallel scan. */
#define PDEIP_SOLVER_SOR 1
#define PDEIP_SOLVER_ALR 2

/* ---- library state ------------------------------------------------------------------ */
const char *pdeip_version(void);
const char *pdeip_last_error(void);
int pdeip_set_mode(int mode);
int pdeip_get_mode(void);
/* Select the HIP device used by the host-pointer entry points (default 0) = pdeip_set_devices(1, &device_id). */
int pdeip_set_device(int device_id);
/* Device group of the host-pointer entry points.  With n > 1, red-black (PDEIP_MODE_RED_BLACK) point-SOR solver calls
 * are cut into n slabs of consecutive MATLAB columns, one per device.  Every device uploads its slab plus a halo of
 * 2 x iter columns per cut side straight from the caller's host planes and relaxes it for the whole call: nothing is
 * exchanged between devices (for a host-pointer call the upload is the halo refresh; csrc/pdeip_multi.hip).  Results are
 * bit-identical to the single-device red-black call.  Exact-order calls and line relaxation do not decompose (their
 * dependency front crosses the frame) and run on ids[0].  Workspace is cached per device. */
int pdeip_set_devices(int n, const int *ids);
/* Writes up to `capacity` ids of the current group to ids (may be NULL) and returns the group size. */
int pdeip_get_devices(int *ids, int capacity);
/* Environment knobs, read once before the first call that needs them, so that an unchanged MATLAB session can opt in
 * without touching a signature (explicit pdeip_set_mode / pdeip_set_device(s) calls made before that win):
 *   PDEIP_MODE     exact | red_black        sweep ordering of the host entry points (default exact)
 *   PDEIP_DEVICE   n                        = pdeip_set_device(n)
 *   PDEIP_DEVICES  a,b,c,...                = pdeip_set_devices */
/* Release the cached device workspace of every device (optional; the process exit also releases it). */
int pdeip_release(void);
/* Number of kernel launches the last *_dev solver call enqueued (diagnostic). */
int pdeip_last_launch_count(void);
/* Diagnostic: the direction of every launch of the calling thread's last red-black point-SOR *_dev call that ran the launch chain
 * (families 3 and 4 of pdeip_debug_plan_sor), in order: the mirror mode the launch ran with -- 0 every strip marched west -> east,
 * 2 every strip east -> west, 1 the odd strips east -> west; 0 for the chain's kernels that have no mirrored march.  Writes the
 * first `cap` of them to out (may be NULL with cap 0) and returns their number; 0 after any other point-SOR call.  With
 * PDEIP_RBP_SERPENTINE=3, and with the variable absent on frames whose planes exceed the Infinity Cache (13 * pixels * frames * 4
 * bytes > 256 MiB), the k_sor_rbp launches on a device alternate 0, 2, 0, 2, ... across launches AND calls (each starts where the
 * one before ended, on lines the cache still holds); every direction gives the same bits. */
int pdeip_debug_last_directions(int *out, int cap);
/* Changes whenever the library frees or regrows a cached workspace buffer (a larger frame, pdeip_release, pdeip_set_device).
 * A caller that captured *_dev calls into a HIP graph must re-capture when the value differs from the one at capture time:
 * the graph's kernel arguments point into those buffers.  Replaying a captured graph between eager calls is supported: nothing
 * the library keeps on the host describes the content of a buffer that a replay rewrites (every exact-order call builds its own
 * schedule table on its stream).  The *_dev calls share ONE set of scratch buffers per device: calls on different streams must
 * be ordered by the caller. */
int pdeip_workspace_generation(void);
/* Waits for the device and reports PDEIP_ERR_DEVICE if a bounded dependency wait of the persistent
 * exact-order kernel (PDEIP_EXACT_PERSIST=1) timed out during the preceding calls. */
int pdeip_persist_error(void);
/* Diagnostic: sets the sticky abort word as a timed-out dependency wait of an exact-order walker would (calls made while it is set
 * drain at once, their results are invalid), to exercise the reporting path: pdeip_persist_error() must return PDEIP_ERR_DEVICE
 * once and clear it. */
int pdeip_debug_raise_abort(void);
/* Diagnostic: the schedule table the exact-order walkers would use for B strips x T sweeps (affine: the XCD-affine lists of
 * PDEIP_PERSIST_XCD=1), built on the device as a call builds it and copied to `table` (16 + B*T ints: list offsets 0..8, items
 * b | t << 16 from int 16 on). */
int pdeip_debug_persist_order(int B, int T, int affine, int *table);
/* Diagnostic: what a point-SOR *_dev call of this shape would launch, decided as the call decides it (csrc/pdeip_sor_plan.hpp) and
 * under the PDEIP_* knobs of the environment, without launching anything.
 *   model       PDEIP_PLAN_*; aligned16: every plane of the caller's is 16-byte aligned; has_dst: a *_dev_to call whose destination
 *               is not the iterate (ignored for the 9-point model, which has none)
 *   num_cus, rb2_slots, rbp_slots   compute units, resident waves of the two-sweep march, resident workgroups of k_sor_rbp.  A
 *               value of 0 is asked from the current device as a call asks it; with all three positive the entry makes no HIP
 *               call and works on a machine without a GPU.
 *   info        PDEIP_PLAN_INFO ints: family (0 nothing to relax, 1 exact order, 2 k_sor_small, 3 k_sor_rb, 4 k_sor_rbp with its 2 / 1
 *               tail, 5 the 9-point four-colour chain), exact-order form (1 persistent, 2 walker, 3 one launch per front), whether a
 *               closing device-to-device copy follows, whether the iterate is copied to the destination first, whether
 *               k_persist_setup runs (these three are not counted by pdeip_last_launch_count()), A, B, NC, W, last_m of the
 *               exact-order forms, and the number of launch records.
 *   records     the launches pdeip_last_launch_count() counts, in order (the first `capacity` of them; may be NULL with capacity 0),
 *               PDEIP_PLAN_RECORD ints each: kind (1 k_sor_rbp, 2 / 3 k_sor_rb two- / one-sweep, 4 k_sor_small, 5 / 6 k_pde8_colour2 /
 *               k_pde8_colour, 7 pack, 8 persistent walk, 9 walker, 10 derive, 11 a front, 12 border fill), sweeps, first launch of a
 *               red-black call, strip width, row tiles, units, grid x, buffer read and buffer written (0 the caller's iterate, 1 the
 *               scratch copy, 2 the destination).  pdeip_disp_sor_llin_sym4_dev runs its plan twice; so do the records. */
enum { PDEIP_PLAN_ELIN4 = 0, PDEIP_PLAN_LLIN4, PDEIP_PLAN_DISP4, PDEIP_PLAN_PDE4, PDEIP_PLAN_PDE8, PDEIP_PLAN_DISPSYM4 };
enum { PDEIP_PLAN_INFO = 11, PDEIP_PLAN_RECORD = 9 };
int pdeip_debug_plan_sor(int model, int nrows, int ncols, int nframes, int iter, int mode, int aligned16, int has_dst, int num_cus,
                         int rb2_slots, int rbp_slots, int *info, int *records, int capacity);
/* Diagnostic: what a line-relaxation *_dev call (solver = 2) of this shape would launch, decided as the call decides it
 * (csrc/pdeip_alr_plan.hpp) and under the PDEIP_ALR_* knobs of the environment, without launching anything and without a HIP call:
 * it works on a machine without a GPU.  The caller's planes are taken to be distinct, as the gateways pass them; nframes is that of
 * the PDE models (the others have one frame); the 9-point PDE model plans one iteration whatever `iter` says, as its call runs.
 *   info        PDEIP_PLAN_ALR_INFO ints: family (0 nothing to do, 1 k_alr_small, 2 zebra, 3 exact order, 4 scan), the launches
 *               pdeip_last_launch_count() reports, the coefficient-transpose launches, the factor launches, whether those take both
 *               fields at once, the iterate transposes per iteration, dynamic LDS bytes of k_alr_small and whether it needs the
 *               opt-in, and the floats of WS_ALR, WS_ALR_T, WS_AUX1 and WS_LEX the call fetches (INT_MAX: more than that).
 *   passes      two records of PDEIP_PLAN_ALR_PASS ints, along the columns and along the rows: kernel (1 k_alr_zebra3, 2
 *               k_alr_zebra3_pair, 3 k_alr_lex, 4 k_alr_lex on the global line buffer, 5 k_alr_scan), first line, last line, line
 *               length, grid x of the factor launch, colours that have a line, {first line, last line, grid x} of up to two
 *               colours, chains per launch, launches per pass, G, dynamic LDS bytes, LDS opt-in, grid x of an exact-order or scan
 *               launch, and the two fields in the order the pass takes them. */
enum { PDEIP_PLAN_ALR_ELIN4 = 0, PDEIP_PLAN_ALR_LLIN4, PDEIP_PLAN_ALR_LLIN8, PDEIP_PLAN_ALR_DISP4, PDEIP_PLAN_ALR_PDE4, PDEIP_PLAN_ALR_PDE8 };
enum { PDEIP_PLAN_ALR_INFO = 12, PDEIP_PLAN_ALR_PASS = 20 };
int pdeip_debug_plan_alr(int model, int nrows, int ncols, int nframes, int iter, int mode, int *info, int *passes);
/* Diagnostic: compares the fused pipeline's fast reciprocal (v_rcp_f32 + one Newton step, taken by the divisor planes of
 * opticalflowSolvers.c:111-127 when every denominator is a normal number with a normal reciprocal) with the IEEE quotient
 * 1.0f / d for EVERY such float (exponent field 1..252, both signs); counts[0] = inputs compared, counts[1] = results that differ
 * in any bit (must be 0). */
int pdeip_debug_rcp_check(unsigned long long *counts);
/* Sweep-kernel timing for bench.py's roofline figure.  While enabled, every *_dev solver call
 * brackets its back-to-back sweep launches (not its prologue) with a pair of HIP events on the
 * call's stream.  pdeip_profile_read() waits for the recorded events, returns the summed elapsed
 * milliseconds and the number of sweep launches they cover, and clears the record. */
int pdeip_profile_enable(int on);
int pdeip_profile_read(double *elapsed_ms, int *sweep_launches);

/* ---- host-pointer drop-in entry points -------------------------------------------------
 * Output pointers marked "optional" may be NULL (the corresponding MATLAB output was not
 * requested, nlhs too small). */

/* [U,V(,RU,RV)] = Oflow_sor_elin4_2d(U,V,M,Cu,Cv,Du,Dv,wW,wN,wE,wS,iter,omega,solver)
 * replaces mexFunction of mex/source/Oflow_sor_elin4_2d.c:64-352 -> GS_SOR_elin4_2d
 * (library/opticalflowSolvers.c:41) + Residuals_elin4_2d (:269).
 * M,Cu,Cv,Du,Dv are [nrows x ncols x nframes_coef]; the solver reads frame 0, the
 * residuals every frame; RU,RV (optional, both or neither) are [.. x nframes_coef].
 * iter<=0: U_out,V_out are all zero (Oflow_sor_elin4_2d.c:341-346). */
int pdeip_oflow_sor_elin4(const float *U, const float *V, const float *M, const float *Cu,
                          const float *Cv, const float *Du, const float *Dv, const float *wW,
                          const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                          int nframes_coef, int iter, float omega, int solver, float *U_out,
                          float *V_out, float *RU, float *RV);

/* [dU,dV(,RU,RV)] = Oflow_sor_llin4_2d(U,V,dU,dV,M,Cu,Cv,Du,Dv,wW,wN,wE,wS,iter,omega,solver)
 * replaces mex/source/Oflow_sor_llin4_2d.c:66-386 -> GS_SOR_llin4_2d
 * (opticalflowSolvers.c:504) + Residuals_llin4_2d (:766). */
int pdeip_oflow_sor_llin4(const float *U, const float *V, const float *dU, const float *dV,
                          const float *M, const float *Cu, const float *Cv, const float *Du,
                          const float *Dv, const float *wW, const float *wN, const float *wE,
                          const float *wS, int nrows, int ncols, int nframes_coef, int iter,
                          float omega, int solver, float *dU_out, float *dV_out, float *RU,
                          float *RV);

/* [dU,dV(,RU,RV)] = Oflow_sor_llin8_2d(U,V,dU,dV,M,Cu,Cv,Du,Dv,wW,wNW,wN,wNE,wE,wSE,wS,wSW,
 *                                      iter,omega,solver)
 * replaces mex/source/Oflow_sor_llin8_2d.c:71-489 -> GS_SOR_llin8_2d (opticalflowSolvers.c:1487),
 * whose point solver never reads the diagonal weights (:1550-1591); they are accepted and
 * ignored here too.  The gateway allocates RU,RV but never fills them (:466-488): zeros. */
int pdeip_oflow_sor_llin8(const float *U, const float *V, const float *dU, const float *dV,
                          const float *M, const float *Cu, const float *Cv, const float *Du,
                          const float *Dv, const float *wW, const float *wNW, const float *wN,
                          const float *wNE, const float *wE, const float *wSE, const float *wS,
                          const float *wSW, int nrows, int ncols, int nframes_coef, int iter,
                          float omega, int solver, float *dU_out, float *dV_out, float *RU,
                          float *RV);

/* [AU,AV] = Oflow_lhs_elin4_2d(U,V,M,Du,Dv,wW,wN,wE,wS)
 * replaces mex/source/Oflow_lhs_elin4_2d.c:56-231 -> LHS_elin4_2d (opticalflowSolvers.c:387). */
int pdeip_oflow_lhs_elin4(const float *U, const float *V, const float *M, const float *Du,
                          const float *Dv, const float *wW, const float *wN, const float *wE,
                          const float *wS, int nrows, int ncols, int nframes_coef, float *AU,
                          float *AV);

/* [AU,AV] = Oflow_lhs_llin4_2d(U,V,dU,dV,M,Du,Dv,wW,wN,wE,wS)
 * replaces mex/source/Oflow_lhs_llin4_2d.c:59-260 -> LHS_llin4_2d (opticalflowSolvers.c:923),
 * including its top-border quirk (:1056). */
int pdeip_oflow_lhs_llin4(const float *U, const float *V, const float *dU, const float *dV,
                          const float *M, const float *Du, const float *Dv, const float *wW,
                          const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                          int nframes_coef, float *AU, float *AV);

/* [dU(,RU)] = Disp_sor_llin4_2d(U,dU,Cu,Du,wW,wN,wE,wS,iter,omega,solver)
 * replaces mex/source/Disp_sor_llin4_2d.c:59-282 -> GS_SOR_llin4_2d (disparitySolvers.c:41).
 * The gateway allocates RU but never computes it (:251-281): zeros. */
int pdeip_disp_sor_llin4(const float *U, const float *dU, const float *Cu, const float *Du,
                         const float *wW, const float *wN, const float *wE, const float *wS,
                         int nrows, int ncols, int iter, float omega, int solver, float *dU_out,
                         float *RU);

/* [dU0 dU1] = Disp_sor_llin_sym4_2d(U0,dU0,Cu0,Du0,wW0,wN0,wE0,wS0, U1,dU1,Cu1,Du1,wW1,wN1,wE1,wS1, iter,omega,solver)
 * replaces mex/source/Disp_sor_llin_sym4_2d.c:82-440 -> GS_SOR_llinsym4_2d / GS_ALR_SOR_llinsym4_2d
 * (disparitySolvers.c:301,462): two disparity fields relaxed side by side that never read each other (the
 * symmetry constraint lives in the MATLAB driver).  The gateway solves unconditionally: iter<=0 returns copies. */
int pdeip_disp_sor_llin_sym4(const float *U0, const float *dU0, const float *Cu0, const float *Du0, const float *wW0,
                             const float *wN0, const float *wE0, const float *wS0, const float *U1, const float *dU1,
                             const float *Cu1, const float *Du1, const float *wW1, const float *wN1, const float *wE1,
                             const float *wS1, int nrows, int ncols, int iter, float omega, int solver,
                             float *dU_out0, float *dU_out1);

/* X = PDEsolver4(X,TRACE,B,wW,wN,wE,wS,iter,omega,solver)
 * replaces mex/source/PDEsolver4.c:54-249 -> GS_SOR_4_2d (pdeSolvers.c:44).  Every plane is
 * [nrows x ncols x nframes].  iter<=0 returns a copy (PDEsolver4.c:239).  solver 3 (unbound
 * function pointer in the reference, PDEsolver4.c:228) is rejected with PDEIP_ERR_SOLVER. */
int pdeip_pde_sor4(const float *X, const float *TRACE, const float *B, const float *wW,
                   const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                   int nframes, int iter, float omega, int solver, float *X_out);

/* X = PDEsolver8(X,TRACE,B,wW,wNW,wN,wNE,wE,wSE,wS,wSW,iter,omega,solver)
 * replaces mex/source/PDEsolver8.c:54-309 -> GS_SOR_8_2d (pdeSolvers.c:153). */
int pdeip_pde_sor8(const float *X, const float *TRACE, const float *B, const float *wW,
                   const float *wNW, const float *wN, const float *wNE, const float *wE,
                   const float *wSE, const float *wS, const float *wSW, int nrows, int ncols,
                   int nframes, int iter, float omega, int solver, float *X_out);

/* [wW,wN,wE,wS] = DdiffWeights(D,eps)
 * replaces mex/source/DdiffWeights.c:50-140 -> diffWeights6_2D_c (imageDiffusionWeights.c:341).
 * D and the four outputs are [nrows x ncols x nframes]; frame 0 of each output holds the
 * weights (max over frames), frames >= 1 stay zero as in the gateway. */
int pdeip_diffweights6(const float *D, int nrows, int ncols, int nframes, float eps, float *wW,
                       float *wN, float *wE, float *wS);

/* Iout = BilinInterp_2d(Iin,X,Y)
 * replaces mex/source/BilinInterp_2d.c:41-124 -> bilinInterp2 (imageInterpolation.c:44).
 * Iin,Iout are [nrows x ncols x nframes]; X,Y are [nrows x ncols] 1-based coordinates
 * (X = column, Y = row).  Out-of-range samples are NaN. */
int pdeip_warp_bilinear(const float *Iin, const float *X, const float *Y, int nrows, int ncols,
                        int nframes, float *Iout);

/* [Idt,Idx,Idy] = FstDerivatives5(It0,It1)
 * replaces mex/source/FstDerivatives5.c:50-145 -> fstSimoncelli_c (library/imageDerivatives.c:309).
 * Every plane is [nrows x ncols x nframes] (frames independent); nrows, ncols >= 4. */
int pdeip_fst_derivatives5(const float *It0, const float *It1, int nrows, int ncols, int nframes,
                           float *Idt, float *Idx, float *Idy);

/* [Idxt,Idyt,Idxx,Idyy,Idxy] = SndDerivatives5(It0,It1)
 * replaces mex/source/SndDerivatives5.c:51-174 -> sndSimoncelli_c (imageDerivatives.c:391). */
int pdeip_snd_derivatives5(const float *It0, const float *It1, int nrows, int ncols, int nframes,
                           float *Idxt, float *Idyt, float *Idxx, float *Idyy, float *Idxy);

/* ---- device-pointer entry points ---------------------------------------------------------
 * Same arithmetic on buffers already resident in HBM; asynchronous on `stream`.  Solvers work
 * in place on the iterate and take the ordering `mode` explicitly.  iter<=0 is a no-op here
 * (the gateway's zero/copy semantics belong to the host entry points).  `col0` is the
 * global column index of local column 0 when the buffers are one slab of a column-slab
 * decomposition (only its parity matters, for the colour of a pixel); 0 for a whole image. */
int pdeip_oflow_sor_elin4_dev(void *stream, float *U, float *V, const float *M, const float *Cu,
                              const float *Cv, const float *Du, const float *Dv, const float *wW,
                              const float *wN, const float *wE, const float *wS, int nrows,
                              int ncols, int iter, float omega, int mode, int col0);
int pdeip_oflow_sor_llin4_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                              const float *M, const float *Cu, const float *Cv, const float *Du,
                              const float *Dv, const float *wW, const float *wN, const float *wE,
                              const float *wS, int nrows, int ncols, int iter, float omega,
                              int mode, int col0);
int pdeip_disp_sor_llin4_dev(void *stream, const float *U, float *dU, const float *Cu,
                             const float *Du, const float *wW, const float *wN, const float *wE,
                             const float *wS, int nrows, int ncols, int iter, float omega,
                             int mode, int col0);
int pdeip_disp_sor_llin_sym4_dev(void *stream, const float *U0, float *dU0, const float *Cu0, const float *Du0,
                                 const float *wW0, const float *wN0, const float *wE0, const float *wS0,
                                 const float *U1, float *dU1, const float *Cu1, const float *Du1,
                                 const float *wW1, const float *wN1, const float *wE1, const float *wS1,
                                 int nrows, int ncols, int iter, float omega, int solver, int mode, int col0);
int pdeip_pde_sor4_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                       const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                       int nframes, int iter, float omega, int mode, int col0);
/* Out-of-place forms of the four 5-point point solvers: the iterate planes are only READ and the relaxed iterate is written to
 * the `_out` planes (iter <= 0: a copy) -- the shape of the gateways themselves (copy the input in, solve on the output:
 * Oflow_sor_elin4_2d.c:341-346).  The red-black launches ping-pong between buffers, so this form never needs the
 * device-to-device copy that an in-place call with an odd number of launches ends with; `_out` == the inputs is the in-place
 * call.  Callers that relax the same planes again and again alternate between two sets. */
int pdeip_oflow_sor_elin4_dev_to(void *stream, const float *U, const float *V, float *U_out, float *V_out, const float *M,
                                 const float *Cu, const float *Cv, const float *Du, const float *Dv, const float *wW,
                                 const float *wN, const float *wE, const float *wS, int nrows, int ncols, int iter,
                                 float omega, int mode, int col0);
int pdeip_oflow_sor_llin4_dev_to(void *stream, const float *U, const float *V, const float *dU, const float *dV,
                                 float *dU_out, float *dV_out, const float *M, const float *Cu, const float *Cv,
                                 const float *Du, const float *Dv, const float *wW, const float *wN, const float *wE,
                                 const float *wS, int nrows, int ncols, int iter, float omega, int mode, int col0);
int pdeip_disp_sor_llin4_dev_to(void *stream, const float *U, const float *dU, float *dU_out, const float *Cu,
                                const float *Du, const float *wW, const float *wN, const float *wE, const float *wS,
                                int nrows, int ncols, int iter, float omega, int mode, int col0);
int pdeip_pde_sor4_dev_to(void *stream, const float *X, float *X_out, const float *TRACE, const float *B, const float *wW,
                          const float *wN, const float *wE, const float *wS, int nrows, int ncols, int nframes, int iter,
                          float omega, int mode, int col0);
int pdeip_pde_sor8_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                       const float *wNW, const float *wN, const float *wNE, const float *wE,
                       const float *wSE, const float *wS, const float *wSW, int nrows, int ncols,
                       int nframes, int iter, float omega, int mode, int col0);
/* Alternating line relaxation, solver = 2 of the gateways (GS_ALR_SOR_*: opticalflowSolvers.c:196,690,1677;
 * disparitySolvers.c:154; pdeSolvers.c:277,344).  Iterate planes in place.
 *   mode PDEIP_MODE_EXACT_ORDER: the reference's line order, bit-identical, inherently serial (one
 *        workgroup per frame; a line of more than 10240 pixels is held in global memory instead of LDS: slow).
 *   mode PDEIP_MODE_RED_BLACK:   zebra order (even lines, then odd lines), lines solved concurrently.
 *   mode PDEIP_MODE_LINE_SCAN:   the reference's line order; the two recurrences of a line are scans over one workgroup
 *        (1e-4 RMS of EXACT_ORDER on diagonally dominant lines, values unspecified otherwise; see the top of this file).
 *        Where the exact-order walker cannot hold its chains in LDS together (two coupled fields with lines of more than
 *        5120 pixels, any line of more than 10240), and with PDEIP_ALR_SCAN=0, the call takes the EXACT_ORDER kernels.
 * pdeip_pde_alr8_dev runs ONE iteration whatever `iter` is, like the reference (pdeSolvers.c:362). */
int pdeip_oflow_alr_elin4_dev(void *stream, float *U, float *V, const float *M, const float *Cu,
                              const float *Cv, const float *Du, const float *Dv, const float *wW,
                              const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                              int iter, float omega, int mode);
int pdeip_oflow_alr_llin4_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                              const float *M, const float *Cu, const float *Cv, const float *Du,
                              const float *Dv, const float *wW, const float *wN, const float *wE,
                              const float *wS, int nrows, int ncols, int iter, float omega, int mode);
int pdeip_oflow_alr_llin8_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                              const float *M, const float *Cu, const float *Cv, const float *Du,
                              const float *Dv, const float *wW, const float *wNW, const float *wN,
                              const float *wNE, const float *wE, const float *wSE, const float *wS,
                              const float *wSW, int nrows, int ncols, int iter, float omega, int mode);
int pdeip_disp_alr_llin4_dev(void *stream, const float *U, float *dU, const float *Cu, const float *Du,
                             const float *wW, const float *wN, const float *wE, const float *wS,
                             int nrows, int ncols, int iter, float omega, int mode);
int pdeip_pde_alr4_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                       const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                       int nframes, int iter, float omega, int mode);
int pdeip_pde_alr8_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                       const float *wNW, const float *wN, const float *wNE, const float *wE,
                       const float *wSE, const float *wS, const float *wSW, int nrows, int ncols,
                       int nframes, int iter, float omega, int mode);
int pdeip_oflow_res_elin4_dev(void *stream, float *RU, float *RV, const float *U, const float *V,
                              const float *M, const float *Cu, const float *Cv, const float *Du,
                              const float *Dv, const float *wW, const float *wN, const float *wE,
                              const float *wS, int nrows, int ncols, int nframes_coef);
int pdeip_oflow_lhs_elin4_dev(void *stream, float *AU, float *AV, const float *U, const float *V,
                              const float *M, const float *Du, const float *Dv, const float *wW,
                              const float *wN, const float *wE, const float *wS, int nrows,
                              int ncols, int nframes_coef);
int pdeip_oflow_res_llin4_dev(void *stream, float *RU, float *RV, const float *U, const float *V,
                              const float *dU, const float *dV, const float *M, const float *Cu,
                              const float *Cv, const float *Du, const float *Dv, const float *wW,
                              const float *wN, const float *wE, const float *wS, int nrows,
                              int ncols, int nframes_coef);
int pdeip_oflow_lhs_llin4_dev(void *stream, float *AU, float *AV, const float *U, const float *V,
                              const float *dU, const float *dV, const float *M, const float *Du,
                              const float *Dv, const float *wW, const float *wN, const float *wE,
                              const float *wS, int nrows, int ncols, int nframes_coef);
int pdeip_diffweights6_dev(void *stream, const float *D, int nrows, int ncols, int nframes,
                           float eps, float *wW, float *wN, float *wE, float *wS);
int pdeip_warp_bilinear_dev(void *stream, const float *Iin, const float *X, const float *Y,
                            int nrows, int ncols, int nframes, float *Iout);
int pdeip_fst_derivatives5_dev(void *stream, const float *It0, const float *It1, int nrows, int ncols,
                               int nframes, float *Idt, float *Idx, float *Idy);
int pdeip_snd_derivatives5_dev(void *stream, const float *It0, const float *It1, int nrows, int ncols,
                               int nframes, float *Idxt, float *Idyt, float *Idxx, float *Idyy,
                               float *Idxy);

/* ---- MATLAB-side stages of one late-linearisation pyramid level, device-resident ("next row" f2) --------
 * What matlab/optical_flow/FlowEminND_llin_2D_v10.m runs between its MEX calls inside firstLoop/secondLoop
 * (:208-356), so that a level can stay in HBM (pde-based-image-processing_amd/flow_level.py drives them).
 * Restatements of MATLAB array code: single/double typing and expression order as written there;
 * checked against oracle/matlab_side.py, not against MATLAB ("parity unpinned"). */
/* X = single((1:cols) + U), Y = single((1:rows)' + V): the warp coordinates (:223) */
int pdeip_flow_coords_dev(void *stream, const float *U, const float *V, int nrows, int ncols, float *X, float *Y);
/* The warp step of one firstLoop iteration in one launch (:223-231): W1 = bilinInterp2(I1, X+U, Y+V) and, with C2 > 0,
 * W2 = bilinInterp2(I2, X+U, Y+V), X,Y = meshgrid(1:cols,1:rows), the sums rounded to single as pdeip_flow_coords_dev stores
 * them.  V may be NULL (warp along x only). */
int pdeip_flow_warp_dev(void *stream, const float *U, const float *V, const float *I1, int C1, const float *I2, int C2, int nrows,
                        int ncols, float *W1, float *W2);
/* robust data-term assembly (:283-327): gD = b./(alpha*sqrt((It - Ix.*dU - Iy.*dV).^2 + 1e-5)) per channel of one or
 * two data terms ([nrows x ncols x C] derivative arrays; C2 = 0: no second term), then nansum over all channels of
 * (Iy.*Ix).*gD -> MGd, (It.*Ix).*gD -> CuGd, (It.*Iy).*gD -> CvGd, (Ix.*Ix).*gD -> DuGd, (Iy.*Iy).*gD -> DvGd. */
int pdeip_flow_assemble_dev(void *stream, const float *It1, const float *Ix1, const float *Iy1, int C1, float b1,
                            const float *It2, const float *Ix2, const float *Iy2, int C2, float b2, const float *dU,
                            const float *dV, float alpha, int nrows, int ncols, float *MGd, float *CuGd, float *CvGd,
                            float *DuGd, float *DvGd);
/* disparity twin (matlab/disparity/DispEminND_llin_2D.m:258-293): CuGd = sum_c (It.*Ix).*gD, DuGd = sum_c (Ix.*Ix).*gD with
 * gD = b./(alpha.*realsqrt((It - Ix.*dU).^2 + 1e-5)); plain sum: NaN propagates to the solver's isnan(Cu) test */
int pdeip_disp_assemble_dev(void *stream, const float *It1, const float *Ix1, int C1, float b1, const float *It2,
                            const float *Ix2, int C2, float b2, const float *dU, float alpha, int nrows, int ncols,
                            float *CuGd, float *DuGd);
/* The same with a gradient-magnitude second term (sndTerm 'gradmag', :253-258, :291-293 -- what runme.m configures): the five
 * planes of SndDerivatives5(I2t0, I2t1w) [.. x C2] take the place of the first-order derivatives. */
int pdeip_flow_assemble_gradmag_dev(void *stream, const float *It1, const float *Ix1, const float *Iy1, int C1, float b1,
                                    const float *Ixt, const float *Iyt, const float *Ixx, const float *Iyy, const float *Ixy, int C2,
                                    float b2, const float *dU, const float *dV, float alpha, int nrows, int ncols, float *MGd,
                                    float *CuGd, float *CvGd, float *DuGd, float *DvGd);
/* One inner iteration's nine coefficient planes in one pass: the assembly above (second term: three first-order planes with
 * Iyy = Ixy = NULL, or the five gradient-magnitude planes Ixt, Iyt, Ixx, Iyy, Ixy) and OPdiffWeights(U+dU, V+dV) (:389-433,
 * pdeip_flow_opdiffweights_dev) of the same iterate -- both only read dU, dV, so the drivers' two calls fuse into one launch. */
int pdeip_flow_assemble_weights_dev(void *stream, const float *It1, const float *Ix1, const float *Iy1, int C1, float b1,
                                    const float *A2, const float *B2, const float *C2p, const float *Iyy, const float *Ixy, int C2,
                                    float b2, const float *U, const float *V, const float *dU, const float *dV, float alpha, int nrows,
                                    int ncols, float *MGd, float *CuGd, float *CvGd, float *DuGd, float *DvGd, float *wW, float *wN,
                                    float *wS, float *wE);
/* disparity twin (matlab/disparity/DispEminND_llin_2D.m:236-238, :271) */
int pdeip_disp_assemble_gradmag_dev(void *stream, const float *It1, const float *Ix1, int C1, float b1, const float *Ixt,
                                    const float *Iyt, const float *Ixx, const float *Ixy, int C2, float b2, const float *dU, float alpha,
                                    int nrows, int ncols, float *CuGd, float *DuGd);
/* The spatial a-priori slice of that assembly (:262-270, :301-318; param.Us / param.Vs, gammaS): appends ASCu.*gSu to CGd and
 * 1.*gSu to DGd (nansum).  Us: the constraint field of the scale, a MATLAB double array; as_diff = 2*(1/scl_factor)^-(scl-1);
 * u_double: U is still the double array of the coarsest scale's first firstLoop; du_double: first inner iteration (dU = zeros). */
int pdeip_flow_apriori_dev(void *stream, const double *Us, const float *U, const float *dU, double gammaS, double alpha,
                           double as_diff, int u_double, int du_double, int nrows, int ncols, float *CGd, float *DGd);
/* The disparity driver's variant (DispEminND_llin_2D.m:246-248, :277-284, :291-292; param.Us, gammaS): ASCu = Us - U, ASDu = 1,
 * gS = gammaS/alpha * exp(-(Us - U - dU)^2 / as_diff^2) with as_diff = 1.75*(1/scl_factor)^-(scl-1); the slices are added to
 * CGd / DGd by a plain sum (NaN propagates).  exp() is the library's own fixed double algorithm (csrc/pdeip_flow.hpp det_exp),
 * shared with the numpy statement of the driver, so results are reproducible bit for bit; not MATLAB's exp to the last ulp. */
int pdeip_disp_apriori_dev(void *stream, const double *Us, const float *U, const float *dU, double gammaS, double alpha,
                           double as_diff, int u_double, int du_double, int nrows, int ncols, float *CGd, float *DGd);
/* rgb2grad (FlowEminND_llin_2D_v10.m:368-381; fstTerm 'grad'): out [.. x 2*nframes], frames 2f-1 / 2f (1-based) = the [1 0 -1]
 * differences of input frame f along x / y, replicate borders */
int pdeip_rgb2grad_dev(void *stream, const float *in, int nrows, int ncols, int nframes, float *out);
/* out = A + B (single); e.g. the argument of DdiffWeights(single(U+dU), eps) (:283) */
int pdeip_add_dev(void *stream, const float *A, const float *B, int nrows, int ncols, float *out);
/* Horn-Schunck, early linearisation: the data terms of one scale (matlab/optical_flow/FlowEminHS_elin_2D_v10.m:133-164) from the
 * two frames [nrows x ncols x C]: separable 5-tap derivative filters and the b1/b2-weighted motion tensor, summed over channels. */
int pdeip_hs_assemble_dev(void *stream, const float *It0, const float *It1, int C, float b1, float b2, int nrows, int ncols,
                          float *MGd, float *CuGd, float *CvGd, float *DuGd, float *DvGd);
/* [wW wN wS wE] = OPdiffWeights(U+dU, V+dV) (:389-433), evaluated in double, returned as single */
int pdeip_flow_opdiffweights_dev(void *stream, const float *U, const float *V, const float *dU, const float *dV, int nrows,
                                 int ncols, float *wW, float *wN, float *wS, float *wE);
/* dU, dV may both be NULL: OPdiffWeights(U, V) of the early-linearisation drivers (FlowEminNDFASFMG_elin_2D_v10.m:392). */
/* Diagnostic: the weights' single(1 ./ sqrt(x)) takes a short sequence that is proven against the exact one (double sqrt,
 * double divide, one rounding) value by value; this runs n arguments (random ones and ones aimed at rounding boundaries)
 * through both and returns how many differ (0 expected), or -1 on a device error. */
int pdeip_selftest_inv_sqrt(int n, unsigned seed);

/* ---- the drivers' image pyramid.  IPT semantics have nothing to be checked against here: pyramid.py states our definition
 * (tap lists at MATLAB's pixel-centre convention, antialiased when shrinking, replicate borders, double accumulation) and
 * these entry points compute exactly that. ---- */
/* imresize(in, [nrows_out ncols_out], 'bilinear' (cubic = 0) or 'bicubic' (1)) */
int pdeip_pyr_resize_dev(void *stream, const float *in, int nrows, int ncols, int nframes, int nrows_out, int ncols_out, int cubic,
                         float *out);
/* imfilter(in, G, 'replicate'), G an odd size x size mask (row-major doubles in host memory, size <= 7) */
int pdeip_pyr_smooth_dev(void *stream, const float *in, int nrows, int ncols, int nframes, const double *G, int size, float *out);

/* ---- symmetric stereo (matlab/disparity/DispEminND_llin_sym_2D.m): the stages the other drivers do not have.  Planes marked
 * double are MATLAB doubles there (U, the warped disparities and what is derived from them). ---- */
/* out = interp2(X, Y, U, X+Uq, Y) (:140-141): linear along x, NaN outside the grid */
int pdeip_sym_warp_flow_dev(void *stream, const float *U, const float *Uq, int nrows, int ncols, double *out);
/* Udt = (U+Uw)*0.5, Udx = prefiltered x-derivative of Uw, CuS = Udt.*(1+Udx), DuS = 1+Udx+Udx+Udx.*Udx (:156-175) */
int pdeip_sym_flow_terms_dev(void *stream, const float *U, const double *Uw, int nrows, int ncols, double *Udt, double *Udx,
                             double *CuS, double *DuS);
/* CuG, DuG of one view (:189-222): robust data term over the C channels plus the symmetry term with
 * gSYM = kS./(1 + Snorm/sr2), kS = channels*beta/alpha, sr2 = srDiff^2; first != 0 in the first inner iteration (dU still
 * MATLAB's double zeros: symmetry weights in double), 0 afterwards (single) */
int pdeip_sym_assemble_dev(void *stream, const float *Idt, const float *Idx, const float *Idxt, const float *Idyt, const float *Idxx,
                           const float *Idxy, int C, const double *Udt, const double *Udx, const double *CuS, const double *DuS,
                           const float *dU, float b1, float b2, float alpha, double kS, double sr2, int first, int nrows, int ncols,
                           float *CuG, float *DuG);

/* TVdenoise4's work between two PDEsolver4 calls (matlab/denoising/TVdenoise4.m:84-98 with DiffWeights :116-156), all single:
 * the four weights (maximum over the frames, outer column/row zeroed) scaled by alpha, PsiData, TRACE, B; [.. x nframes] each.
 * The maximum over the frames is MATLAB's max: NaN is skipped, the result is NaN only where every frame is NaN. */
int pdeip_tv4_assemble_dev(void *stream, const float *Iout, const float *Iin, int nrows, int ncols, int nframes, float alpha,
                           float *TRACE, float *B, float *aW, float *aN, float *aE, float *aS);
/* [W NW N NE E SE S SW] = ADdiffWeights(D, quantile) of the anisotropic flow driver (matlab/optical_flow/
 * FlowEminAD_llin_2D_v10.m:416-487): Alvarez derivative in double, strongest frame per pixel, lambda = the quantile of the
 * non-zero squared gradient norms, tensor weights with circshift wrap-around; returned as single (the solver's arguments).
 * NaN in the frame maximum follows MATLAB's max: a frame whose squared norm is NaN is skipped, the first of the maximal numeric
 * frames wins, and a pixel whose norm is NaN in every frame (or in the only one) takes frame 1, i.e. keeps NaN derivatives and a
 * NaN norm.  In the selection of lambda a NaN norm is a non-zero one and the largest value (sort places NaN last): it moves
 * the rank but becomes lambda only if the rank reaches it.  The same holds for pdeip_tv_assemble_dev. */
int pdeip_ad_weights_dev(void *stream, const float *D, int nrows, int ncols, int nframes, double quantile, float *wW, float *wNW,
                         float *wN, float *wNE, float *wE, float *wSE, float *wS, float *wSW);

/* ---- FAS full-multigrid flow (matlab/optical_flow/FlowEminNDFASFMG_elin_2D_v10.m): the stages between its MEX calls ----
 * Planes are [nrows x ncols x frames], column-major, as everywhere.  Output dimensions of the two halving stages are
 * ceil(nrows/2) x ceil(ncols/2) (MATLAB's 1:2:end). */
/* imfilter(I, G, 'replicate', 'conv') with a 5x5 kernel (:104-105); g25 = the kernel G itself, column-major (host memory) */
int pdeip_fas_gauss5_dev(void *stream, const float *in, int nrows, int ncols, int frames, const float *g25, float *out);
/* one pyramid step (:108-111): [1 4 6 4 1]/16 along both axes, then (1:2:end, 1:2:end, :); out == in: PDEIP_ERR_ARG */
int pdeip_fas_down_dev(void *stream, const float *in, int nrows, int ncols, int frames, float *out);
/* the per-scale constants (:125-153) from the frames (0..255 range): planes = [13][frames][ncols][nrows] in the order
 * Idt, Idx, Idy, Idxx, Idyy, Idxy, Idxt, Idyt, M, Cu, Cv, Du, Dv */
int pdeip_fas_prepare_dev(void *stream, const float *It0, const float *It1, int nrows, int ncols, int frames, float b1, float b2,
                          float *planes);
/* gd = 1./(k*sqrt(OPnorm+0.00001)) at (U,V) and the solver's planes (:377-397 summed over the frames when per_frame = 0,
 * one plane each; :425-445 / :228-237 per frame when per_frame = 1, [.. x frames] each, plus gd).  Cu/Cv: the right-hand
 * side [.. x frames] (the scale's own or the cycle's fu/fv); they, their outputs and gd may be NULL. */
int pdeip_fas_assemble_dev(void *stream, const float *planes, const float *Cu, const float *Cv, const float *U, const float *V,
                           int nrows, int ncols, int frames, float b1, float b2, float k, int per_frame, float *MGd, float *CuGd,
                           float *CvGd, float *DuGd, float *DvGd, float *gd);
/* The smoother's two calls of one firstLoop iteration in one launch: pdeip_fas_assemble_dev with per_frame = 0 and
 * OPdiffWeights(U, V) (:392). */
int pdeip_fas_assemble_weights_dev(void *stream, const float *planes, const float *Cu, const float *Cv, const float *U, const float *V,
                                   int nrows, int ncols, int frames, float b1, float b2, float k, float *MGd, float *CuGd, float *CvGd,
                                   float *DuGd, float *DvGd, float *wW, float *wN, float *wS, float *wE);
/* imfilter(in*scale, [1 2 1;2 4 2;1 2 1]/16, 'replicate', 'conv')(1:2:end, 1:2:end, :) (:200, :212-217); out == in: PDEIP_ERR_ARG */
int pdeip_fas_restrict_dev(void *stream, const float *in, int nrows, int ncols, int frames, float scale, float *out);
/* out = (R + A)./gd (:250-251); elementwise, so out may be R, A or gd */
int pdeip_fas_rhs_dev(void *stream, const float *R, const float *A, const float *gd, int nrows, int ncols, int frames, float *out);
/* U = U + imresize((Uc-Ures)*inv_scale, size(U), 'bilinear') (:256-257); Uc, Ures are [nrows_c x ncols_c]; both
 * sizes at least 2x2 (what a side of 3 halves to) */
int pdeip_fas_prolong_add_dev(void *stream, float *U, int nrows, int ncols, const float *Uc, const float *Ures, int nrows_c,
                              int ncols_c, float inv_scale);
/* out = imresize(in.*mul, [nrows_out ncols_out]) with imresize's default bicubic kernel, enlarging (:177-180); both sizes
 * at least 2x2; out == in: PDEIP_ERR_ARG */
int pdeip_fas_upscale_dev(void *stream, const float *in, int nrows, int ncols, float mul, int nrows_out, int ncols_out, float *out);
/* TVdenoise8's work between two PDEsolver8 calls (matlab/denoising/TVdenoise8.m:80-86 with ADdiffWeights :119-231):
 * the anisotropic weights of Iout (double; Alvarez derivative, strongest frame per pixel, lambda = median of the
 * non-zero squared gradient norms), then TRACE = PsiData + alpha*sum(w), B = PsiData.*Iin with
 * PsiData = 1./sqrt((Iout-Iin).^2 + eps), and single(alpha*w) for the eight weights; all [nrows x ncols x nframes]. */
int pdeip_tv_assemble_dev(void *stream, const float *Iout, const float *Iin, int nrows, int ncols, int nframes,
                          float alpha, float *TRACE, float *B, float *aW, float *aNW, float *aN, float *aNE,
                          float *aE, float *aSE, float *aS, float *aSW);
/* out = medfilt2(A + B, [3 3], 'symmetric') (:352); B may be NULL (out = medfilt2(A)); out must not alias A or B.
 * Our definition where medfilt2's is not documented: the 5th of the nine window values (the edge pixel mirrored) in ascending
 * order with NaN as the LARGEST value, above +Inf, as sort places it.  A window with up to four NaN yields its 5th smallest
 * number, one with five or more yields NaN.  Sign of zero: -0 and +0 are equal in that order; where a window holds zeros of both
 * signs and the median is a zero, only its value is defined, not its sign.  Everywhere else the result is defined to the bit. */
int pdeip_median3_dev(void *stream, const float *A, const float *B, int nrows, int ncols, float *out);
/* Two fields in one launch: out0 = medfilt2(A0 + B0), out1 = medfilt2(A1 + B1) (:352-353 filters U+dU and V+dV). */
int pdeip_median3_pair_dev(void *stream, const float *A0, const float *B0, const float *A1, const float *B1, int nrows, int ncols,
                           float *out0, float *out1);

/* ---- whole drivers, resident on the device (csrc/pdeip_drivers.hip) --------------------------------------------------------
 * What `runme.m` calls -- its eight drivers, FlowEminND_llin_2D_v10 (runme.m:44) and DispEminND_llin_2D (runme.m:20) first -- as ONE
 * host-pointer call each: the frames go up once, the coarse-to-fine loop (pyramid, warps, derivatives, robust assembly, diffusion weights,
 * solver calls, medians, up-scaling) runs on device planes, the result comes down once.  A MATLAB session reaches them through
 * the stubs mex/FlowEminND_llin_2D_v10_gpu.c and mex/DispEminND_llin_2D_gpu.c.  The pyramid's IPT calls
 * (imresize, imfilter, fspecial) are OUR definitions of them (pyramid.py); everything between them is the arithmetic the
 * per-stage entry points above are tested for. */
#define PDEIP_TERM_NONE 0
#define PDEIP_TERM_RGB 1
#define PDEIP_TERM_GRAD 2     /* first term only: rgb2grad */
#define PDEIP_TERM_GRADMAG 3  /* second term only: gradient magnitude through SndDerivatives5 */
/* param struct of both drivers (FlowEminND_llin_2D_v10.m:52-67, DispEminND_llin_2D.m:51-66); a member that is <= 0 (or NaN)
 * keeps the driver's own default; `scales` limits the number of pyramid scales (param.scales).  NULL: all defaults. */
typedef struct pdeip_driver_params {
    double alpha, omega, gammaS, b1, b2, scl_factor;
    int firstLoop, secondLoop, iter, solver, scales;
} pdeip_driver_params;
/* [U V] = FlowEminAD_llin_2D_v10(Iin, channels, fstTerm, sndTerm, param) (matlab/optical_flow/FlowEminAD_llin_2D_v10.m,
 * runme.m:54,64): the anisotropic-diffusion flow driver; arguments as pdeip_flow_nd_llin plus param.quantile (<= 0: 0.9) and
 * param.diffusion (flow_diffusion 0: 'image', the default -- eight weights from frame 0 of a scale, once per scale; 1: 'flow' --
 * from U+dU+V+dV in every inner iteration). */
int pdeip_flow_ad_llin(const float *Iin, int nrows, int ncols, int channels, int fst_term, int snd_term, const pdeip_driver_params *prm,
                       double quantile, int flow_diffusion, const double *Us, const double *Vs, float *U, float *V);
/* [U V] = FlowEminNDFASFMG_elin_2D_v10(Iin, channels, param) (matlab/optical_flow/FlowEminNDFASFMG_elin_2D_v10.m, runme.m:90): the FAS
 * full-multigrid flow driver in one call; Iin as for pdeip_flow_nd_llin (0..255, not rescaled by this driver).  A member that is
 * <= 0 (or NaN) keeps the driver's default (alpha 0.035, omega 1.9, firstLoop 4, iter 4, b1 0.03, b2 0.97, scl_factor 0.5,
 * solver 2, cycle_index 1 = V-cycle, scales = until a side is <= 10 pixels); NULL: all defaults. */
typedef struct pdeip_fas_params {
    double alpha, omega, b1, b2, scl_factor;
    int firstLoop, iter, solver, cycle_index, scales;
} pdeip_fas_params;
int pdeip_flow_fas_fmg_elin(const float *Iin, int nrows, int ncols, int channels, const pdeip_fas_params *prm, float *U, float *V);
/* [U V] = FlowEminHS_elin_2D_v10(Iin, channels, param) (matlab/optical_flow/FlowEminHS_elin_2D_v10.m, runme.m:74): Horn-Schunck
 * with early linearisation, the whole coarse-to-fine run in one call; Iin as for pdeip_flow_nd_llin.  Of the parameter struct
 * alpha (0.2), omega (1.9), iter (20), b1 (0.25), b2 (0.75), scl_factor (0.75) and solver (2) are this driver's. */
int pdeip_flow_hs_elin(const float *Iin, int nrows, int ncols, int channels, const pdeip_driver_params *prm, float *U, float *V);
/* U = DispEminND_llin_sym_2D(Il, Ir, param) (matlab/disparity/DispEminND_llin_sym_2D.m, runme.m:28): symmetric stereo, both
 * views' disparities; Il, Ir single [nrows x ncols x channels] (this driver does not divide by 255); U: [nrows x ncols x 2].
 * A member that is <= 0 (or NaN) keeps the driver's default (alpha 0.035, beta 0.4, omega 1.9, firstLoop 3, secondLoop 4, iter 4,
 * b1 0.25, b2 0.72, scl_factor 0.75, solver 2); NULL: all defaults. */
typedef struct pdeip_sym_params {
    double alpha, beta, omega, b1, b2, scl_factor;
    int firstLoop, secondLoop, iter, solver;
} pdeip_sym_params;
int pdeip_disp_nd_llin_sym(const float *Il, const float *Ir, int nrows, int ncols, int channels, const pdeip_sym_params *prm, float *U);
/* Iout = TVdenoise8(I_in, param) (matlab/denoising/TVdenoise8.m, runme.m:144) and Iout = TVdenoise4(I_in, param)
 * (TVdenoise4.m, runme.m:143) as one host-pointer call each: I_in single, 0..1, [nrows x ncols x frames] column-major; the short
 * pyramid, the lagged-diffusivity loop (weights, PsiData / TRACE / B, PDEsolver8 | PDEsolver4) and the up-scaling stay on the
 * device.  A member of the parameter struct that is <= 0 (or NaN) keeps the driver's own default; NULL: all defaults
 * (TVdenoise8: alpha 500, omega 1.75, outer_iter 20, inner_iter 4, solver 2, scl 0.75, scl_factor 0.75; TVdenoise4: alpha 5,
 * omega 1.75, outer_iter 10, inner_iter 5, solver 2, scl 0.5, scl_factor 0.75). */
typedef struct pdeip_tv_params {
    double alpha, omega, scl, scl_factor;
    int outer_iter, inner_iter, solver;
} pdeip_tv_params;
int pdeip_tvdenoise8(const float *Iin, int nrows, int ncols, int frames, const pdeip_tv_params *prm, float *Iout);
int pdeip_tvdenoise4(const float *Iin, int nrows, int ncols, int frames, const pdeip_tv_params *prm, float *Iout);
/* [U V] = FlowEminND_llin_2D_v10(Iin, channels, fstTerm, sndTerm, param): Iin = cat(3, frame0, frame1), single, 0..255,
 * [nrows x ncols x 2*channels] column-major; fst_term PDEIP_TERM_RGB | _GRAD, snd_term _NONE | _RGB | _GRADMAG; Us, Vs:
 * param.Us / param.Vs, double [nrows x ncols] or NULL; U, V: [nrows x ncols].  Ordering: pdeip_set_mode / PDEIP_MODE. */
int pdeip_flow_nd_llin(const float *Iin, int nrows, int ncols, int channels, int fst_term, int snd_term, const pdeip_driver_params *prm,
                       const double *Us, const double *Vs, float *U, float *V);
/* U = DispEminND_llin_2D(Il, Ir, fstTerm, sndTerm, param): Il, Ir single 0..255 [nrows x ncols x channels]; Us: param.Us or NULL. */
int pdeip_disp_nd_llin(const float *Il, const float *Ir, int nrows, int ncols, int channels, int fst_term, int snd_term,
                       const pdeip_driver_params *prm, const double *Us, float *U);

/* ---- level sets: the active-contour section of runme.m (csrc/pdeip_levelset.hip) ------------------------------------------
 * Arrays as everywhere: column-major float32 [nrows x ncols x nframes]; frames are planes solved independently.  nrows, ncols
 * >= 2 (PDEIP_ERR_ARG otherwise, before any HIP call); lines of any length (the reference stops at MAX_BUF_SIZE = 2048).
 * AOS has one order: pdeip_set_mode does not apply.  PHI_out must not alias an input.
 *
 * PHI_out = AC_solver_2d(PHI, D, GradNorm, Diff, tau, nu) (mex/source/AC_solver_2d.c -> AC_AOS_4_2d, levelsetSolvers.c:145-181):
 * one AOS step of the geodesic active contour -- a Thomas solve along every column, one along every row, their sum with both
 * passes' Diff == 0 rules, then one re-initialisation step (T = 0.25).  Bit-identical to the reference's column and row passes;
 * the re-initialisation step follows the sign-function contract below. */
int pdeip_ac_solver(const float *PHI, const float *D, const float *GradNorm, const float *Diff, int nrows, int ncols, int nframes,
                    float tau, float nu, float *PHI_out);
/* PHI_out = Reinit(PHI, T) (mex/source/Reinit.c -> reinit, levelsetSolvers.c:969-1118): as many re-initialisation steps as the
 * reference's loop for (t = 0; t < T; t += 0.25f) runs (T <= 0 or NaN: none, PHI_out = PHI; a T at which t stops growing is
 * refused).  Unlike the reference gateway, PHI is not modified.  Sign-function contract: the reference's SSE path uses
 * rsqrtps (a 12-bit estimate); this library computes S = PHI * (1.0f / sqrtf(PHI*PHI + sqrtf((PHIx*PHIx + PHIy*PHIy) +
 * FLT_EPSILON))) with correctly rounded sqrtf and division -- the same operation order, not bit-identical at that step. */
int pdeip_reinit(const float *PHI, int nrows, int ncols, int nframes, float T, float *PHI_out);
/* Device-pointer forms of the two, asynchronous on `stream`; workspace from the library's cache. */
int pdeip_ac_solver_dev(void *stream, const float *PHI, const float *D, const float *GradNorm, const float *Diff, int nrows,
                        int ncols, int nframes, float tau, float nu, float *PHI_out);
int pdeip_reinit_dev(void *stream, const float *PHI, int nrows, int ncols, int nframes, float T, float *PHI_out);
/* PHI_out = CV_solver_2d(PHI, D, DH, GradNorm, tau, nu) (mex/source/CV_solver_2d.c -> CV_AOSOMP_4_2d, levelsetSolvers.c:103,
 * GRADNORM_ZERO_CHECK defined): one AOS step of the Chan-Vese model, bit-identical to the reference.  The gateway hands DH to
 * the library's GradNorm_in slot and GradNorm to its Diff_in slot, so with g = GradNorm, delta = DH and q a line neighbour of p:
 * w(p,q) = (g_p + g_q > 0) ? ((2*tau)*delta_p) / (g_p + g_q) : 0 (a NaN sum gives 0), right-hand side PHI + (tau*delta)*D, and
 * a Thomas solve along every column (xc) and every row (xr), each chain running on its own solved x.  With i the row, j the
 * column index and clamp(v) = "if (v > 5) v = 5; if (v < -5) v = -5;" (a NaN passes through):
 *   col = (i >= 1 && g == 0) ? clamp(PHI) : clamp(0.0f + xc),   PHI_out = (j >= 1 && g == 0) ? clamp(PHI) : clamp(col + xr)
 * (g == -0.0 counts as zero, a NaN g does not).  PHI_out must not alias an input. */
int pdeip_cv_solver(const float *PHI, const float *D, const float *DH, const float *GradNorm, int nrows, int ncols, int nframes,
                    float tau, float nu, float *PHI_out);
/* The terms the segmentation drivers build for each CV_solver_2d call (DispSegmentation.m:380-387, DispSegmentationSparse.m:
 * 388-396), this library's definition for single PHI (parity with MATLAB unpinned): DH = 1.0f / ((float)M_PI * (c0 + (PHI*PHI)
 * / c1)), then if (DH < dh_floor) DH = dh_floor (a NaN dh_floor: no floor; a NaN DH stays NaN); GradNorm = sqrtf(dx*dx + dy*dy)
 * with dx, dy = imfilter(PHI, [-1 0 1]*0.5, 'replicate') and its transpose, as the GAC drivers define them.  The drivers' forms:
 * (c0, c1, dh_floor) = (1, 1, NaN) (generateSeeds), (1, 1, 0.06) (DispSegmentation), (2, 4, 0.04) (DispSegmentationSparse).
 * nrows, ncols, nframes >= 1; the outputs must not alias PHI or each other. */
int pdeip_cv_terms(const float *PHI, int nrows, int ncols, int nframes, float c0, float c1, float dh_floor, float *DH_out,
                   float *GradNorm_out);
/* Device-pointer forms, asynchronous on `stream`, workspace from the library's cache; no host read-back (graph-capturable). */
int pdeip_cv_solver_dev(void *stream, const float *PHI, const float *D, const float *DH, const float *GradNorm, int nrows,
                        int ncols, int nframes, float tau, float nu, float *PHI_out);
int pdeip_cv_terms_dev(void *stream, const float *PHI, int nrows, int ncols, int nframes, float c0, float c1, float dh_floor,
                       float *DH_out, float *GradNorm_out);
/* PHIout = GAC_v10a(Iin, PHIin, param) / GAC_v10b(Iin, PHIin, param) (matlab/active_contour/GAC_v10a.m, GAC_v10b.m; runme.m:128-131):
 * the whole geodesic-active-contour driver in one call, resident on the device.  Iin: single [nrows x ncols x channels] (runme.m
 * divides by 255); PHIin: single [nrows x ncols]; PHIout: [nrows x ncols]; nrows, ncols >= 3.  model: PDEIP_GAC_A (balloon
 * force c, upwind gradient) or PDEIP_GAC_B (convection along grad g, circshift wrapping at the borders).  Reinit(PHIin, 10),
 * the 7x7 Gaussian (sigma 2.5) and the [-1 0 1]*0.5 derivatives are this library's definitions of the IPT calls (pyramid.py);
 * lambda < 0 selects sort(Igrad(:))(round(0.7*N)) on the device.  Every member of the parameter struct that is NaN keeps the
 * driver's default (tau 0.25, c -0.1 (model a only), lambda -1 = automatic, iter = ITER 100, smooth = SMOOTH 100): a NaN, not
 * <= 0, because c is negative by default and a negative lambda means "automatic".  NULL: all defaults. */
#define PDEIP_GAC_A 0
#define PDEIP_GAC_B 1
typedef struct pdeip_gac_params {
    double tau, c, lambda, iter, smooth;
} pdeip_gac_params;
int pdeip_gac(const float *Iin, int nrows, int ncols, int channels, const float *PHIin, int model, const pdeip_gac_params *prm,
              float *PHIout);
/* The same on device pointers, asynchronous on `stream` (no host read-back inside: graph-capturable). */
int pdeip_gac_dev(void *stream, const float *Iin, int nrows, int ncols, int channels, const float *PHIin, int model,
                  const pdeip_gac_params *prm, float *PHIout);
/* The stages of the driver that come before its loop, on device pointers, asynchronous on `stream`, no host read-back (graph-
 * capturable); pdeip_gac_dev runs through these two, so a caller of either runs the driver's own code.
 * pdeip_select_kth_dev: *out = the k-th smallest (1-based) of x[0..n), what MATLAB's Y = sort(x); Y(k) gives: NaN sort last (k may
 * point into them: the result is then a NaN), -Inf and +Inf are ordinary values.  The key orders -0.0 below +0.0, which sort()
 * leaves in the order they came: where the k-th element is a zero, only its value is defined, not its sign.  By four passes over
 * x, one per 8-bit digit of an order-preserving key (a 256-bin histogram on at most 1024 workgroups, then the digit that holds
 * the rank); the state is cleared at the start of every call, so nothing survives from one call to the next.  Nine launches.
 * Refused with PDEIP_ERR_ARG before any HIP call: a NULL pointer, n < 1 or > 2^31-1, k < 1, k > n.
 * pdeip_gac_stopping_dev (GAC_v10a.m:57-75): Igrad_out = max_c(Idx).^2 + max_c(Idy).^2 of the channels of I smoothed with the 7x7
 * Gaussian (sigma 2.5), the derivatives [-1 0 1]*0.5 with a replicated border and max() over the channels ignoring NaN (the first of
 * equal values kept); *lambda_out = the element of rank round(0.7*N) of Igrad_out when lambda < 0, N = nrows*ncols and round() taken
 * of the double product as MATLAB does (N = 45: 0.7*45 = 31.499999999999996, rank 31, not 32), otherwise lambda rounded to single
 * (a NaN included); g_out = 1 ./ (1 + Igrad_out ./ *lambda_out) in single with true divisions.  I: [nrows x ncols x channels];
 * Igrad_out, g_out: [nrows x ncols], not aliasing I or each other; lambda_out: one device float.  Refusals as pdeip_gac_dev's. */
int pdeip_select_kth_dev(void *stream, const float *x, long long n, long long k, float *out);
int pdeip_gac_stopping_dev(void *stream, const float *I, int nrows, int ncols, int channels, double lambda, float *Igrad_out,
                           float *g_out, float *lambda_out);

/* ---- nonlinear diffusion (csrc/pdeip_diffusion.hip) -----------------------------------------------------------------------
 * Iout = Diffusion4_v10(I_in, 'alpha', alpha, 'outer_iter', outer_iter) (matlab/diffusion/Diffusion4_v10.m) before its uint8
 * cast: the lagged-diffusivity filter as one call, resident on the device.  Iin, Iout: single [nrows x ncols x channels]; Iin is
 * never modified and Iout == Iin is allowed.  `for iter = 0:outer_iter` runs floor(outer_iter) + 1 iterations (none when
 * outer_iter < 0), each: the weights wW wN wE wS = DdiffWeights(Iout, 1e-5f) with the maximum over the channels as the .m's
 * max(w, [], 3) takes it (a NaN of any channel is omitted, where the gateway keeps one of its first frame), then for every channel
 * a Thomas solve along every column with a = -alpha*wN, b = 2 + alpha*(wN + wS), c = -alpha*wS, one along every row with
 * a = -alpha*wW, b = 2 + alpha*(wW + wE), c = -alpha*wE, both with d = Iout(:,:,k), and Iout(:,:,k) = ver + hor; every operation
 * in single, alpha rounded to single, in the order of the .m.  A NaN member (or prm == NULL) keeps the driver's default (alpha
 * 25, outer_iter 5).  Refused with PDEIP_ERR_ARG before any HIP call: nrows or ncols < 2, channels < 1, a non-finite alpha, an
 * infinite outer_iter; with PDEIP_ERR_UNSUPPORTED: more than 65535 columns or channels.  pdeip_set_mode does not apply (a Thomas
 * solve has one order). */
typedef struct pdeip_diffusion4_params {
    double alpha, outer_iter;
} pdeip_diffusion4_params;
int pdeip_diffusion4(const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion4_params *prm, float *Iout);
/* The same on device pointers, asynchronous on `stream`: one stream, no host read-back, no graph branches (graph-capturable). */
int pdeip_diffusion4_dev(void *stream, const float *Iin, int nrows, int ncols, int channels,
                         const pdeip_diffusion4_params *prm, float *Iout);

/* ---- RANSAC surface fit (csrc/pdeip_ransac.hip) ---------------------------------------------------------------------------
 * [M_out, Err] = SurfaceEquation(A, B, M_in, err_thr, min_set_size, iter) (mex/source/SurfaceEquation.c + library/ransac.c): the
 * RANSAC fit of A * M = B, A single [ndata x ncoef] column-major with ncoef = 3 ([X Y 1]) or 6 ([X^2 Y^2 XY X Y 1]), B [ndata];
 * n = ncoef + 1 samples per hypothesis.  The control flow is RANSAC()'s (ransac.c:31-220): err_thr2 = err_thr*err_thr in single;
 * abs_min = (unsigned)(min_set_size*(float)ndata + 0.5f) (a value below 1, negative included, gives 0); a row is an inlier iff
 * e <= err_thr2 (a NaN error never is).  A given model M_in (NULL: none) is scored first: it seeds the best error sum and is licit
 * iff its inliers >= abs_min.  Then hypotheses 0..iter-1 IN ORDER: one becomes the best model iff inliers >= abs_min && sum <
 * best sum (strict: the earliest wins a tie); otherwise, while no licit model exists yet, it replaces the best-inlier model iff
 * inliers >= the best-inlier count (not strict: the latest wins).  M_out is the best licit model, else the best-inlier model;
 * err_out [ndata] holds its errors.  Where the reference is undefined or not deterministic, this library's definitions:
 *   samples      sets [iter x n] 0-based row indices, hypothesis-major (duplicates allowed), or, with sets == NULL, drawn from
 *                seed: sample k of hypothesis i is (uint32)(((splitmix64(seed + i*n + k) >> 32) * (uint64)ndata) >> 32), where
 *                splitmix64(x) is { z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *                0x94D049BB133111EB; return z ^ (z >> 31); } in 64-bit wrapping arithmetic (the reference: rand() % ndata).
 *   fit          (the reference: sgels) Householder QR in float64 on the samples widened from single, no pivoting, every sum in
 *                ascending index, no FMA, correctly rounded sqrt and division; for column k: s = sum_{i>=k} R[i][k]^2, norm =
 *                sqrt(s), alpha = R[k][k] > 0 ? -norm : norm, v_k = R[k][k] - alpha, v_i = R[i][k], vtv = sum v_i^2, then for
 *                every later column c and at last the right-hand side f = (2*sum v_i*c_i)/vtv, c_i = c_i - f*v_i, and R[k][k] =
 *                alpha; back-substitution t = b[k], t = t - R[k][j]*x[j] for j = k+1.., x[k] = t/R[k][k]; x rounded to single.  An
 *                exactly zero norm marks the hypothesis singular: its model is zero and all its errors are FLT_MAX
 *                (SurfaceEquation.c:417-421).
 *   error        of row j for model m, in single without FMA: t = A[j,0]*m[0]; t = t + A[j,1]*m[1]; ...; d = t - B[j]; e = d*d
 *                (the reference: sgemm, whose order is unspecified).
 *   score        the inlier count is exact; the error sum over the inliers is float64, reduced in a fixed order that does not
 *                depend on the hypothesis (no floating-point atomics): equal models get equal sums, two calls the same bits.
 *   no model     iter <= 0 and no licit given model: the given model and its errors; with M_in == NULL: PDEIP_ERR_ARG (the
 *                reference returns uninitialised memory).
 * inliers_out (NULL ok) [iter + 1]: [0] the given model's count (-1 if none), [1 + i] hypothesis i's; errsum_out (NULL ok)
 * [iter + 1] the float64 sums likewise ([0] = 0 if none).  Refused with PDEIP_ERR_ARG before any HIP call: a NULL A, B, M_out or
 * err_out, ncoef not 3 or 6, ndata < 1, a non-finite err_thr or min_set_size, and in the host form a sets entry >= ndata.
 * pdeip_set_mode does not apply.  Parity with the reference's compiled gateway is unpinned (it needs MATLAB's BLAS and LAPACK). */
int pdeip_surface_equation(const float *A, const float *B, int ndata, int ncoef, const float *M_in, float err_thr,
                           float min_set_size, int iter, const unsigned *sets, unsigned long long seed, float *M_out, float *err_out,
                           int *inliers_out, double *errsum_out);
/* The same on device pointers (sets, inliers_out and errsum_out too), asynchronous on `stream`: workspace from the library's
 * cache, one stream, no host read-back, no graph branches (graph-capturable).  A sets entry >= ndata cannot be refused here: it
 * makes its hypothesis singular and nothing is read through it. */
int pdeip_surface_equation_dev(void *stream, const float *A, const float *B, int ndata, int ncoef, const float *M_in, float err_thr,
                               float min_set_size, int iter, const unsigned *sets, unsigned long long seed, float *M_out,
                               float *err_out, int *inliers_out, double *errsum_out);
/* The fit as the segmentation drivers use it (DispSegmentation.m:329-360), resident: the data are the pixels with PHI >= 0 (a NaN
 * PHI is false) of the [nrows x ncols] planes PHI and D, ranked in column-major order; pixel (i, j) (0-based) has X = j + 1, Y =
 * i + 1, the row [X Y 1] (order 1) or [X^2 Y^2 XY X Y 1] (order 2) with each product formed in double and rounded to single, and
 * B = D(i, j).  The result equals pdeip_surface_equation_dev on that A, B bit for bit; ndata, abs_min and the seeded draws are
 * formed on the device.  M_out [3 | 6]; dist_out (NULL ok) [nrows x ncols]: the error formula on EVERY pixel's row against D
 * (distD of :349/:360, in single; FLT_MAX everywhere when the chosen hypothesis is singular); ndata_out (device, NULL ok): the number of pixels taken.  A mask without pixels sets *ndata_out
 * = 0 and M_out = M_in (NaN when none was given).  Same refusals, with `order` not 1 or 2 in place of ncoef. */
int pdeip_surface_fit_masked_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int order, const float *M_in,
                                 float err_thr, float min_set_size, int iter, const unsigned *sets, unsigned long long seed,
                                 float *M_out, float *dist_out, int *ndata_out);
/* The masked fit of S level-set planes PHI [nrows x ncols x S] over ONE data plane D [nrows x ncols] in one chain of launches:
 * for every s in 0..S-1, column s of M_out [ncoef x S], plane s of dist_out (NULL ok) [nrows x ncols x S] and ndata_out[s] (device,
 * NULL ok, [S]) equal, bit for bit, what
 *   pdeip_surface_fit_masked_dev(stream, PHI + s*nrows*ncols, D, nrows, ncols, order, M_in ? M_in + s*ncoef : NULL, err_thr,
 *                                min_set_size, iter, NULL, seed + seed_stride*s, ...)
 * writes, the seed formed in 64-bit wrapping arithmetic; all that call defines holds per segment (a mask without pixels gives
 * M_out = M_in, NaN when none was given; a singular winner gives FLT_MAX in dist; a NaN PHI is false).  M_in (NULL: no segment has
 * a given model) is [ncoef x S].  There is no sets argument: the draws are seeded.  M_out may be M_in (models updated in place);
 * dist_out must not alias PHI or D.  Asynchronous on `stream`: workspace from the library's cache (S*nrows*ncols ints, not the
 * single call's data rows), one stream, no host read-back, no atomics, no graph branches (graph-capturable); at most 7 launches, 6
 * without dist_out, whatever S is (pdeip_last_launch_count()).  Refused with PDEIP_ERR_ARG before any HIP call: a NULL PHI, D or
 * M_out, S < 1 or S > 65535, order not 1 or 2, nrows or ncols < 1, a non-finite err_thr or min_set_size, iter <= 0 with M_in ==
 * NULL, an iter the single call refuses, a workspace of more than 2^31-1 elements (S*nrows*ncols too large), dist_out == PHI or D.
 * pdeip_set_mode does not apply. */
int pdeip_surface_fit_masked_batch_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order,
                                       const float *M_in, float err_thr, float min_set_size, int iter, unsigned long long seed,
                                       unsigned long long seed_stride, float *M_out, float *dist_out, int *ndata_out);

/* ---- region competition: the inner loop of the segmentation drivers (csrc/pdeip_segmentation.hip) ---------------------------
 * What regionCompetition() does between its MEX calls (matlab/segmentation/DispSegmentation.m:497-646, DispSegmentationSparse.m:
 * 511-666), defined here because MATLAB's evaluation of the data term cancels catastrophically.  S level-set planes PHI [nrows x
 * ncols x S], one data plane D [nrows x ncols], column-major float32; eps = 2^-52.  One COMPETITION ITERATION `iter` (1-based):
 *  1. sizes     size_s = #{PHI_s >= 0} (a NaN is false).  Segments with (double)size_s < srem_thr*nrows*ncols (the product formed
 *               in double, left to right) are removed, the survivors compacted in order, ALL surface models reset to zero and
 *               `recalc` set.  No segment left: the call returns at once with S_out = 0 and PDEIP_OK.
 *  2. terms     when iter is odd or recalc is set, (a)-(e), then recalc is cleared:
 *     (a) DH, gradPHI = pdeip_cv_terms(PHI, c0, c1, dh_floor).
 *     (b) all live segments in one pdeip_surface_fit_masked_batch_dev call, which is, per segment in order,
 *         pdeip_surface_fit_masked_dev with M_in = the segment's current model (a zero model IS a given model), err_thr,
 *         min_set_size = ransac_cset, 10 hypotheses, dist_out = the segment's dist plane.  The k-th fit a call performs (0-based,
 *         every fit counted, across iterations and scales) draws from seed + 65536*k in 64-bit wrapping arithmetic: the batch
 *         call's seed is that of its first segment, its seed_stride 65536.  With nan_fill not NaN the fit and dist see D with every NaN replaced by nan_fill; D is not modified.
 *     (c) n_s = the number of pixels with PHI_s >= 0 and, when dist_cap is finite, (double)dist < dist_cap (a NaN dist fails);
 *         cov_s = (sum of (double)dist over them) / n_s, the sum in float64 in a fixed order that depends neither on S nor on s
 *         (no floating-point atomics; with dist_cap = +Inf a NaN propagates); then if (cov_s < minCOV) cov_s = minCOV (a NaN
 *         stays; n_s == 0 gives NaN).
 *     (d) in float64, correctly rounded sqrt and division: c_s = 1/sqrt((2*pi)*cov_s), t = (double)dist/(2*cov_s), P_s =
 *         c_s*exp(-t).
 *     (e) WC_s by strategy; max ignores NaN as MATLAB's does (all NaN: NaN); over the empty set of S == 1 it is 0:
 *           PDEIP_SEG_SURFACE  WC_s = max_{r != s} P_r
 *           PDEIP_SEG_GREEDY   as SURFACE, then WC_s = 0 where no segment has PHI >= 0 and DH_s > 0.02f
 *           PDEIP_SEG_INVERSE  WC_s = max(Q_s, max_{r != s} [PHI_r >= 0 ? P_r : 0]) with Q_s = -(c_s*expm1(-t)) (S == 1: Q_s)
 *         DATA_s = (float) log((P_s + eps)/(WC_s + eps)).  Q_s is the one deliberate departure from the .m, which forms c_s - P_s:
 *         equal in exact arithmetic, but quantised at c_s*2^-53 -- the size of the eps it is added to -- so that one ulp in exp
 *         moves DATA by 0.17 where dist -> 0.  Q_s is accurate there and the same elsewhere after rounding to single.
 *  3. step      PHI = CV_solver_2d(PHI, DATA, DH, gradPHI, tau = 1, nu), nu = (float)(gamma_coef*(nrows*ncols)^0.7) formed in
 *               double, all live planes in one call.  On an even iteration without removal DATA, DH and gradPHI are the previous
 *               iteration's.
 * The drivers' two forms are parameters; a NaN member (or prm == NULL) keeps the dense driver's value:
 *               c0  c1  dh_floor  err_thr  gamma_coef  dist_cap  nan_fill
 *   dense        1   1   0.06      1.0      0.001       +Inf      NaN (D is used as it is)
 *   sparse       2   4   0.04      1.2      0.005       100       1000
 * Refused with PDEIP_ERR_ARG before any HIP call: nrows or ncols < 2, S < 1, an order other than 1 or 2, an unknown strategy, a
 * non-finite minCOV, srem_thr, err_thr or ransac_cset, minCOV <= 0, iterations < 0.  pdeip_set_mode does not apply. */
#define PDEIP_SEG_SURFACE 0
#define PDEIP_SEG_GREEDY 1
#define PDEIP_SEG_INVERSE 2
typedef struct pdeip_seg_params {
    double c0, c1, dh_floor, err_thr, gamma_coef, dist_cap, nan_fill;
} pdeip_seg_params;
/* The stages on device pointers, asynchronous on `stream`, no host read-back (graph-capturable); partials in the library's cache.
 * sizes_out int [S]: step 1's counts.  cov_out double [S], n_out int [S] (NULL ok): step 2c (a NaN dist_cap means +Inf).
 * pdeip_seg_data_dev: steps 2d-e from dist [S planes], PHI, DH, cov [S] (device, double); DATA_out [S planes] must not alias an
 * input; P_out (NULL ok) receives P as float64 planes.  P_s is formed twice (once per pass over the segments) by the same
 * operations; every plane is read once per pass. */
int pdeip_seg_sizes_dev(void *stream, const float *PHI, int nrows, int ncols, int S, int *sizes_out);
int pdeip_seg_variance_dev(void *stream, const float *PHI, const float *dist, int nrows, int ncols, int S, double minCOV, double dist_cap,
                           double *cov_out, int *n_out);
int pdeip_seg_data_dev(void *stream, const float *dist, const float *PHI, const float *DH, const double *cov, int nrows, int ncols, int S,
                       int strategy, float *DATA_out, double *P_out);
/* `iterations` competition iterations on one scale, resident.  PHI, D, PHI_out [nrows x ncols x S], surf_out [ncoef x S] (ncoef =
 * 3 | 6) and cov_out (double [S], NULL ok: the last variances, zero if none was formed) are device pointers in the _dev form and
 * host pointers in the other; S_out, kept_out (int [S]: the 0-based input index of each survivor) and fit_counter are host
 * pointers in both.  S_out planes / columns / entries are written.  fit_counter (NULL: starts at 0, not returned) holds k of step
 * 2b on entry and on return, so that a caller can run one count across calls.  The _dev form reads the S sizes back once per
 * iteration (pinned memory, one stream synchronisation) to decide removal and recalc on the host: it is NOT graph-capturable, and
 * it has returned from its last synchronisation, not from its last kernel, when it returns.  Compaction is device-to-device plane
 * copies; workspace from the library's cache.  PHI_out must not alias PHI.  These two calls and pdeip_region_competition clear the
 * thread's error text on entry: after one that returned PDEIP_OK, pdeip_last_error() is empty. */
int pdeip_seg_competition_level_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order, int strategy,
                                    double minCOV, float ransac_cset, int iterations, double srem_thr, unsigned long long seed,
                                    unsigned long long *fit_counter, const pdeip_seg_params *prm, int *S_out, float *PHI_out,
                                    float *surf_out, int *kept_out, double *cov_out);
int pdeip_seg_competition_level(const float *PHI, const float *D, int nrows, int ncols, int S, int order, int strategy, double minCOV,
                                float ransac_cset, int iterations, double srem_thr, unsigned long long seed, unsigned long long *fit_counter,
                                const pdeip_seg_params *prm, int *S_out, float *PHI_out, float *surf_out, int *kept_out, double *cov_out);
/* [PHIout SParam] = regionCompetition(D, pyramid, polyorder, sigmaLim, ransac_cset, iterations, srem_thr, PHIin, competition)
 * (DispSegmentation.m:448-654) in one call, host pointers.  The D pyramid is built here: scale k+1 = imresize(scale k, scl_factor)
 * through pdeip_pyr_resize_dev(cubic = 1) at ceil(size*scl_factor), K the last scale with both sides >= rc_scl x the original (and
 * >= 3, and still shrinking); the visits are [1..K, K..1], each one level call with minCOV = sigmaLim on the PHI of the visit
 * before, resized (cubic) to the visit's size (:648-650; the .m's initial PHI pyramid of :471-473 only fixes these sizes).  The
 * fit counter runs across the visits.  PHI_out [nrows x ncols x S_out], surf_out: the last visit's models, kept_out as above.
 * Also refused: scl_factor outside (0, 1), rc_scl not finite or <= 0, nrows or ncols < 3. */
int pdeip_region_competition(const float *D, const float *PHI, int nrows, int ncols, int S, int order, int strategy, double sigmaLim,
                             float ransac_cset, int iterations, double srem_thr, double scl_factor, double rc_scl, unsigned long long seed,
                             const pdeip_seg_params *prm, int *S_out, float *PHI_out, float *surf_out, int *kept_out);
/* The numbered map of DispSegmentation.m:190-198: SEG = sum over 1-based s of s*[PHI_s > 0], 0 where two or more segments hold the
 * pixel (after which the .m's SEG(SEG > segments) = segments + 1 cannot fire).  SEG_out int32 [nrows x ncols]. */
int pdeip_seg_label_dev(void *stream, const float *PHI, int nrows, int ncols, int S, int *SEG_out);
int pdeip_seg_label(const float *PHI, int nrows, int ncols, int S, int *SEG_out);

/* ---- connected components (csrc/pdeip_ccl.hip) ------------------------------------------------------------------------------
 * [L, num] = bwlabel(A > 0, conn) and regionprops(.., 'Area') as generateSeeds() calls them (matlab/segmentation/
 * DispSegmentation.m:282-298).  A [nrows x ncols] column-major float32; a pixel is foreground iff A > 0: a NaN, +0.0, -0.0 and
 * every negative value are background, a positive subnormal and +Inf are foreground.  conn is 8 (bwlabel's default, what the
 * drivers use: diagonal contacts join) or 4.  The numbering is MATLAB's: components are numbered 1..num in the order of their
 * first pixel in column-major (memory) order, background is 0.  L_out int32 [nrows x ncols] (must not alias A); num_out int [1];
 * areas_out (NULL ok) int [areas_cap]: areas_out[l-1] = the pixel count of component l for l <= min(num, areas_cap), 0 for the
 * entries from num on; areas beyond areas_cap are not written.  The result is a pure function of the mask: the implementation
 * uses integer atomics only (min on labels, adds on areas), whose outcome is unique, and no floating-point atomics; two calls give
 * the same bits.
 *   Two forms, chosen by the plane's size: planes of up to 16384 pixels (the coarse pyramid scales the drivers label) are done by
 * one workgroup in LDS in one launch; larger ones tile by tile in LDS, then the tile seams, then a prefix sum over the roots.
 * PDEIP_CCL_SMALL=0 forces the tiled form, =1 the one-workgroup form wherever it admits the plane.
 *   Refused with PDEIP_ERR_ARG before any HIP call: a NULL A, L_out / out or (bwlabel) num_out, nrows or ncols < 1, nrows*ncols >
 * INT_MAX, conn not 4 or 8, areas_cap < 0.  pdeip_set_mode does not apply.
 *   The _dev forms take device pointers (num_out and areas_out too), are asynchronous on `stream`, take their workspace from the
 * library's cache, run a number of launches that depends on the plane's size only and read nothing back: graph-capturable.
 * The tiled form keeps its tree, labels, areas and scalars in ONE workspace of that cache, as the other units do: two _dev calls
 * on different streams, or a captured graph replayed while another call of this section runs, would share it and race.  Order
 * such calls on one stream. */
int pdeip_bwlabel_dev(void *stream, const float *A, int nrows, int ncols, int conn, int *L_out, int *num_out, int *areas_out,
                      int areas_cap);
int pdeip_bwlabel(const float *A, int nrows, int ncols, int conn, int *L_out, int *num_out, int *areas_out, int areas_cap);
/* out = lo everywhere and hi on the component with the largest area (DispSegmentation.m:284-290; [CCY CCI] = max(...): the LOWEST
 * label wins a tie).  No foreground at all: all lo, *area_out = 0, *num_out = 0 (this library's definition; the .m indexes with an
 * empty CCI there).  out float32 [nrows x ncols] may alias A.  num_out, area_out (NULL ok): the number of components and the
 * largest area; device pointers in the _dev form.  Same forms, refusals and capturability as above. */
int pdeip_largest_component_dev(void *stream, const float *A, int nrows, int ncols, int conn, float hi, float lo, float *out,
                                int *num_out, int *area_out);
int pdeip_largest_component(const float *A, int nrows, int ncols, int conn, float hi, float lo, float *out, int *num_out,
                            int *area_out);

/* ---- generateSeeds() and the dense driver (csrc/pdeip_segmentation.hip) --------------------------------------------------------
 * [PHIout SParam] = generateSeeds(Din, pyramid, polyorder, sigmaLim, ransac_cset_vect, iterations, srem_thr, AAin, seeds)
 * (matlab/segmentation/DispSegmentation.m:203-443) in one call, host pointers, resident on the device for the whole call, with
 * the definitions fixed above for regionCompetition().  D [nrows x ncols]; AA [nrows x ncols] float or NULL for all ones, a NaN
 * counts as 0; cset_vect double [n_cset].
 *   Scales: the sizes follow the rule of pdeip_region_competition with pyr_scl in place of rc_scl; the D pyramid is built through
 * pdeip_pyr_resize_dev(cubic); the visits are [1..K, K..1], numbered v = 0..2K-1.  gamma starts at 0.01 per call.
 *   Per seed: the AA pyramid is formed by cubic resize to each scale's size; minCOV = sigmaLim; PHI_1 = -1 everywhere and +1 at the
 * 0-based rows 1, 6, 11, .. <= nrows-2 and columns 1, 6, .. <= ncols-2.
 *   Per visit: include = AA_scl > 0.05f; at v = 0 PHI(~include) = -1; the model is reset to "none"; at v = K (the second visit of
 * the coarsest scale) PHI = pdeip_largest_component_dev(PHI, 8, +5, -5); nu = (float)(gamma*(rows*cols)^0.7) in double.
 *   Per iteration it = 1..iterations: RITER = (it == 1 && v == 0) ? 2000 : 100; RCONS = v == 0 ? cset_vect[min(it, n_cset) - 1] :
 * cset_vect[n_cset - 1]; the count #{PHI >= 0} is read back, fewer than 20 marks the seed EMPTY and leaves both loops; the fit is
 * pdeip_surface_fit_masked_dev with the current model (none on a visit's first iteration), err_thr 0.7, RCONS, RITER, the dist
 * plane and seed + 65536*k, k the running count of all fits (starting at *fit_counter, 0 if NULL; the end value is returned there
 * so that a caller can chain counts); cov as pdeip_seg_variance_dev with S = 1, floored at minCOV; DATA as pdeip_seg_data_dev
 * with S = 1 and PDEIP_SEG_INVERSE (the -c*expm1(-t) form of c - P); DATA(~include) = -2; DH, gradPHI = pdeip_cv_terms_dev(1, 1,
 * NaN); PHI = pdeip_cv_solver_dev(PHI, DATA, DH, gradPHI, 1, nu).
 *   After a visit: EMPTY: gamma *= 0.8 (this persists over the remaining seeds) and the seed ends without output.  At v = K with
 * iterations > 0: minCOV becomes the UNFLOORED variance of the visit's last iteration (its mask, its dist plane) if that exceeds
 * mincov_gate (a NaN never does).  Otherwise PHI is resized (cubic) to the next visit's size.
 *   After a seed that is not empty its PHI_1 and model are appended to PHI_out [nrows x ncols x seeds] (S_out planes written) and
 * surf_out [ncoef x seeds] (NaN with iterations == 0: no fit was made); then AA_1 = (PHI_1 < 0) && (AA_1 != 0).
 *   The .m's final "remove small segments" block (:435-443) operates on PHI{1}, which by then is PHIinitial, never on PHIout: it
 * removes nothing.  This call removes nothing and takes no srem_thr.
 *   pdeip_seeds_params: what the two drivers' generateSeeds() differ in; a NaN member (or prm == NULL) keeps the dense value:
 * dist_cap +Inf (sparse 100), nan_fill NaN (sparse 1000: the fit and dist see D with its NaNs replaced), mincov_gate -Inf (sparse
 * 0.5, DispSegmentationSparse.m:417-424).  err_thr is 0.7 in both.
 *   trace (NULL ok) records what a checker needs: counts[0..min(n_counts, counts_cap)) every count read back, in order (n_counts is
 * the number there were); largest (NULL ok) [rK x cK x seeds] the v = K largest-component planes, n_largest of them.
 *   The count needs one pinned read-back per iteration, as the level call does: NOT graph-capturable.  Refused with PDEIP_ERR_ARG
 * before any HIP call: a NULL D or output, nrows or ncols < 3, seeds outside 1..65535, planes too large, iterations < 0, order not
 * 1 or 2, a non-finite or non-positive sigmaLim, n_cset < 1 or a non-finite entry, scl_factor outside (0, 1), pyr_scl not finite
 * or <= 0.  pdeip_set_mode does not apply. */
typedef struct pdeip_seeds_params {
    double dist_cap, nan_fill, mincov_gate;
} pdeip_seeds_params;
typedef struct pdeip_seeds_trace {
    int *counts;
    int counts_cap, n_counts;
    float *largest;
    int n_largest;
} pdeip_seeds_trace;
int pdeip_generate_seeds(const float *D, const float *AA, int nrows, int ncols, int order, double sigmaLim, const double *cset_vect,
                         int n_cset, int iterations, int seeds, double scl_factor, double pyr_scl, unsigned long long seed,
                         unsigned long long *fit_counter, const pdeip_seeds_params *prm, pdeip_seeds_trace *trace, int *S_out,
                         float *PHI_out, float *surf_out);
/* [PHI SEG SParam] = DispSegmentation(Din, param) (DispSegmentation.m:31-198), host pointers.  NaNs of Din are set to 0;
 * cset_vect = ransac_min_cset + (ransac_max_cset - ransac_min_cset)/ransac_cset_cycles * [0..cycles] (:56); strategy inverse.
 *   PHIin == NULL (param.PHI empty): seeds (sigmaLim 0.7, 20 iterations, AA == 1 allowed or everything with AA == NULL, gen_scl);
 * unless seeds == 1: competition (1.5, 30), seeds again (1.2, 20, rc_scl) on sum(PHI > 0, 3) == 0, concatenated, competition
 * (1.5, 20).  PHIin [nrows x ncols x S_in] given: competition (1.0, 20), one more seed (1.2, 20, rc_scl) on the uncovered
 * pixels, competition (2.0, 20).  The stages are pdeip_generate_seeds and pdeip_region_competition; stage j (0-based, in call
 * order) draws from seed + j*2^32; PHI crosses the host between stages.  A stage after which no segment is left ends the call
 * with *S_out = 0 and nothing else written (a seeding stage that only adds nothing to existing segments goes on, as cat(3, PHI,
 * []) does).  PHI_out and surf_out must hold 2*seeds (PHIin == NULL) or S_in + 1 planes / models; *S_out of them are written;
 * SEG_out int32 [nrows x ncols] through pdeip_seg_label.  A NaN (double) or 0 (int) member of prm, or prm == NULL, keeps the
 * .m's default: srem_thr 0.002, polyorder 1, seeds 15, scl_factor 0.7, gen_scl 0.2, rc_scl 0.4, ransac_min_cset 0.1,
 * ransac_max_cset 0.7, ransac_cset_cycles 10.  Refusals: those of the two stage calls, before any HIP call.  Not graph-capturable. */
typedef struct pdeip_dispseg_params {
    double srem_thr, scl_factor, gen_scl, rc_scl, ransac_min_cset, ransac_max_cset;
    int polyorder, seeds, ransac_cset_cycles;
} pdeip_dispseg_params;
int pdeip_disp_segmentation(const float *Din, int nrows, int ncols, const float *PHIin, int S_in, const float *AA,
                            const pdeip_dispseg_params *prm, unsigned long long seed, int *S_out, float *PHI_out, int *SEG_out,
                            float *surf_out);

/* ---- the sparse driver (csrc/pdeip_sparse.hip, csrc/pdeip_segmentation.hip) ----------------------------------------------------
 * DispSegmentationSparse.m takes disparity maps whose NaNs mean "no estimate".  It differs from the dense driver in nanmedfilt2(),
 * in its D pyramid, in generateSeeds()'s starting gamma and in constants that are parameters of the stage calls above.
 *
 * out = nanmedfilt2(A) (DispSegmentationSparse.m:679-685: colfilt(A, [3 3], 'sliding', @nanmedian); the .m ignores its fsize
 * argument).  This library's definition.  A, out column-major float32 [nrows x ncols x nframes], every plane filtered on its own.
 *   The window of pixel (i, j) is its 3x3 neighbourhood; a position outside the plane contributes the VALUE 0.0f (colfilt's zero
 * padding is a value, not a missing one).  NaNs in the window are ignored.  With n the number of non-NaN values among the nine:
 *     n == 0   NaN (an edge pixel always sees at least three zeros and a corner five: this happens at interior pixels only)
 *     n odd    the (n+1)/2-th smallest value
 *     n even   (float)(((double)a + (double)b) * 0.5) of the n/2-th and (n/2+1)-th smallest: the correctly rounded mean, no overflow
 *   +Inf and -Inf in the middle of an even window give NaN, two equal infinities that infinity.  -0 and +0 compare equal; which
 * zero comes out of a window holding both is not part of the contract (compare by value), as for pdeip_median3_dev.  Everywhere
 * else the result is defined to the bit.  out must not alias A.
 *   Refused with PDEIP_ERR_ARG before any HIP call: a NULL pointer, nrows, ncols or nframes < 1, a plane of more than INT_MAX
 * pixels, out == A; with PDEIP_ERR_UNSUPPORTED: more than 65535 columns or frames (the launch geometry).  The _dev form takes
 * device pointers, is asynchronous on `stream`, one launch, reads nothing back: graph-capturable.  The host form copies A up and
 * out down.  pdeip_set_mode does not apply. */
int pdeip_nanmedfilt2_dev(void *stream, const float *A, int nrows, int ncols, int nframes, float *out);
int pdeip_nanmedfilt2(const float *A, int nrows, int ncols, int nframes, float *out);
/* The sparse driver's D pyramid (:63-64, :76-79), host pointers: P_1 = nanmedfilt2(D), P_{k+1} = nanmedfilt2(imresize(nanmedfilt2(
 * P_k), scl_factor)), imresize being pdeip_pyr_resize_dev(cubic = 1) at ceil(size*scl_factor).  The sizes follow the rule of
 * pdeip_region_competition with pyr_scl in place of rc_scl.  Where NaNs go in a resize is that call's definition: a NaN reaches
 * every output pixel whose tap list touches it, zero-weight taps included.  3K - 2 launches, all on the device.
 *   *K_out = K; sizes_out int [2*scales_cap] receives rows, cols per scale (2K entries); out receives the K planes packed in scale
 * order without padding.  out == NULL: the sizes only, no HIP call, D is not read.  Refused with PDEIP_ERR_ARG before any HIP
 * call: a NULL K_out or sizes_out, a NULL D with out given, nrows or ncols < 3, a plane of more than INT_MAX pixels, scl_factor
 * outside (0, 1), pyr_scl not finite or <= 0, scales_cap < 1 or smaller than K (nothing is written then); PDEIP_ERR_UNSUPPORTED:
 * more than 65535 columns. */
int pdeip_sparse_pyramid(const float *D, int nrows, int ncols, double scl_factor, double pyr_scl, int scales_cap, int *K_out,
                         int *sizes_out, float *out);
/* generateSeeds() and regionCompetition() of DispSegmentationSparse.m (:207-447, :452-674): pdeip_generate_seeds and
 * pdeip_region_competition, argument for argument, with three things different:
 *   - D is the raw map with its NaNs; its pyramid is pdeip_sparse_pyramid's, built inside the call.  The filled copy of each scale
 *     (nan_fill) is made from that pyramid (:287, :500).  The AA and PHI pyramids stay plain cubic resizes.
 *   - a NaN member of prm, or prm == NULL, resolves to the SPARSE driver's value: seeds dist_cap 100, nan_fill 1000, mincov_gate
 *     0.5; competition c0 2, c1 4, dh_floor 0.04, err_thr 1.2, gamma_coef 0.005, dist_cap 100, nan_fill 1000.  (A struct cannot ask
 *     for "no fill" or "no gate" here: that is what the dense calls are for.)
 *   - generateSeeds()'s gamma starts at 0.005 per call (:226).
 * Everything else, the refusals included, is as stated for the dense calls. */
int pdeip_generate_seeds_sparse(const float *D, const float *AA, int nrows, int ncols, int order, double sigmaLim, const double *cset_vect,
                                int n_cset, int iterations, int seeds, double scl_factor, double pyr_scl, unsigned long long seed,
                                unsigned long long *fit_counter, const pdeip_seeds_params *prm, pdeip_seeds_trace *trace, int *S_out,
                                float *PHI_out, float *surf_out);
int pdeip_region_competition_sparse(const float *D, const float *PHI, int nrows, int ncols, int S, int order, int strategy, double sigmaLim,
                                    float ransac_cset, int iterations, double srem_thr, double scl_factor, double rc_scl,
                                    unsigned long long seed, const pdeip_seg_params *prm, int *S_out, float *PHI_out, float *surf_out,
                                    int *kept_out);
/* [PHI SEG SParam] = DispSegmentationSparse(Din, param) (DispSegmentationSparse.m:42-202), host pointers: pdeip_disp_segmentation
 * with Din's NaNs left in place (the stages filter them), the two sparse stage calls above, and the sparse .m's defaults for a NaN
 * / 0 member of prm or prm == NULL: srem_thr 0.002, polyorder 2, seeds 15, scl_factor 0.75, gen_scl 0.55, rc_scl 0.55,
 * ransac_min_cset 0.1, ransac_max_cset 0.7, ransac_cset_cycles 10.  The stage constants (0.7/20, 1.5/30, 1.2/20, 1.5/20; with
 * PHIin 1.0/20, 1.2/20 with one seed, 2.0/20), the strategy (inverse), AA == 1 as the allowed area, the stage seeds, PHI crossing
 * the host between stages, SEG through pdeip_seg_label, *S_out = 0 after a stage that leaves no segment, the sizes of the outputs
 * and the refusals are those of pdeip_disp_segmentation.  The .m's param.varLim is never read and its `keyboard` block (:544-547)
 * is a debugging stop.  Not graph-capturable. */
int pdeip_disp_segmentation_sparse(const float *Din, int nrows, int ncols, const float *PHIin, int S_in, const float *AA,
                                   const pdeip_dispseg_params *prm, unsigned long long seed, int *S_out, float *PHI_out, int *SEG_out,
                                   float *surf_out);

/* ---- flow colour coding and error measures (csrc/pdeip_flowviz.hip) -------------------------------------------------------------
 *
 * img = flow2color(cat(3, U, V), 'maxvalue', maxvalue, 'border', border) (matlab/optical_flow/flow2color.m), the whole function:
 *   dir   = atan2(-V, -U), negative angles + 2 pi, / (2 pi): the hue in turns
 *   mag   = sqrt(U^2 + V^2) / maxvalue, values above 1 set to 1
 *   valid = isfinite(U) & (mag <= 1)   (a NaN in V makes mag NaN; an Inf in V alone leaves the pixel valid, as in the .m)
 *   hsv   = valid ? (dir, 1, mag) : (1, 0, 1), i.e. white; rgb = hsv2rgb(hsv)
 * maxvalue NaN stands for the .m's empty default: the maximum magnitude of the field by MATLAB's max (NaN magnitudes ignored, Inf
 * counts, an all-NaN field gives NaN and an all-white picture; a zero field gives 0/0 and an all-white picture).  *maxvalue_out (may
 * be NULL) receives the value used, in place of the .m's disp().
 * border > 0: the picture is (nrows + 2 border) x (ncols + 2 border); its frame is the colour coding of X = (j / bcols - 0.5) * 10,
 * Y = (i / brows - 0.5) * 10 (1-based i, j) normalised by its own maximum sqrt(50), and the flow's picture is pasted at 1-based
 * index `border`, i.e. 0-based offset border - 1 (flow2color.m:66; the .m's off-by-one, kept).
 * U, V: column-major float32 [nrows x ncols].  rgb_out: float32 [brows x bcols x 3] in MATLAB layout, or NULL.  rgb8_out: the same
 * picture as uint8(round(255 x)), interleaved RGB in row-major order [brows][bcols][3], or NULL.  One of the two must be given.
 * Arithmetic (this library's definition; MATLAB's hsv2rgb is not pinned): inputs promoted to float64, every step in float64 without
 * FMA, hsv2rgb the six-sector formula (k = floor(6 h), k = 6 as 0, f = 6 h - k, p = v (1 - s), q = v (1 - s f), t = v (1 - s (1 - f))),
 * one rounding to float32; rgb8 is computed from the float32 value.
 * _dev: device pointers (maxvalue_out a device double), launches on `stream`, nothing read back, graph-capturable once the
 * workspace exists; 1 launch with maxvalue given, 3 with maxvalue NaN, whatever the data (pdeip_last_launch_count()).
 * Refused with PDEIP_ERR_ARG before any HIP call: U or V NULL, both outputs NULL, nrows or ncols < 1, border < 0, a picture of more
 * than 2^31-1 elements; PDEIP_ERR_UNSUPPORTED: more than 1048560 columns. */
int pdeip_flow2color_dev(void *stream, const float *U, const float *V, int nrows, int ncols, double maxvalue, int border, float *rgb_out,
                         unsigned char *rgb8_out, double *maxvalue_out);
int pdeip_flow2color(const float *U, const float *V, int nrows, int ncols, double maxvalue, int border, float *rgb_out,
                     unsigned char *rgb8_out, double *maxvalue_out);
/* The flow (U, V) against a ground truth (Ut, Vt).  A pixel counts when all four values are finite there and mask (float32
 * [nrows x ncols], or NULL for every pixel) is nonzero.  Per counted pixel, in float64 on the promoted inputs, without FMA:
 *   endpoint error   sqrt((U - Ut)^2 + (V - Vt)^2)
 *   angular error    acos(clamp((U Ut + V Vt + 1) / (sqrt(U^2 + V^2 + 1) sqrt(Ut^2 + Vt^2 + 1)), -1, 1)) * (180 / pi)   (Barron et al.)
 * epe_out, ang_out: float32 [nrows x ncols] or NULL; pixels that do not count hold NaN.  stats_out: double[4] = {count, mean
 * endpoint error, mean angular error, largest endpoint error}; with count 0 the last three are NaN.  The sums are the library's
 * fixed-order float64 tree (thread, wave butterfly, waves ascending, tiles ascending), so a call is reproducible to the bit.
 * _dev: device pointers, 2 launches on `stream`, nothing read back, graph-capturable once the workspace exists.
 * Refused with PDEIP_ERR_ARG before any HIP call: U, V, Ut, Vt or stats_out NULL, nrows or ncols < 1, more than 2^31-1 pixels. */
int pdeip_flow_errors_dev(void *stream, const float *U, const float *V, const float *Ut, const float *Vt, const float *mask, int nrows,
                          int ncols, float *epe_out, float *ang_out, double *stats_out);
int pdeip_flow_errors(const float *U, const float *V, const float *Ut, const float *Vt, const float *mask, int nrows, int ncols,
                      float *epe_out, float *ang_out, double *stats_out);

/* ---- cross-checks: where a disparity or a flow can be trusted (csrc/pdeip_crosscheck.hip) ----------------------------------------
 *
 * This library's own definitions (the reference has no such function).  All arithmetic is float64 on the promoted float32 inputs,
 * every product and sum rounded, no FMA; results are rounded once to float32.
 *
 * The left-right check of two disparities.  D0 is the view being checked, D1 the other view, both column-major float32
 * [nrows x ncols] in the sign convention of the symmetric driver (pdeip_disp_nd_llin_sym): view 0's pixel x matches view 1 at
 * x + D0(x).  Per pixel:
 *   w    = the value pdeip_sym_warp_flow_dev(U = D1, Uq = D0) defines, bit for bit (one device function serves both): linear along
 *          x, NaN outside 1 <= xq <= ncols, xq == ncols the last column itself; a tap with weight 0 still propagates its NaN (0 * NaN)
 *   r    = D0 + w
 *   kept = isfinite(r) && |r| <= tol
 * sparse_out: kept ? D0 : NaN, D0's own bits (-0.0 included); may be D0 itself, since a thread reads only its own pixel of D0.
 * mask_out: 1.0f or 0.0f.  diff_out: (float)r.  stats_out: double[4] = {kept, defined (pixels with finite r), mean |r| over the
 * defined pixels, largest |r| over them}; with nothing defined the last two are NaN.  Each output may be NULL, but not all of them.
 *
 * The forward-backward check of two flows.  (Uf, Vf) is the flow of frame 0 -> 1, (Ub, Vb) that of frame 1 -> 0, in the flow drivers'
 * convention (BilinInterp_2d(I1, X+U, Y+V)).  Per pixel (i, j), 0-based:
 *   xq = (j+1) + Uf, yq = (i+1) + Vf; in range iff 1 <= xq <= ncols and 1 <= yq <= nrows, otherwise ub = vb = NaN
 *   j0 = min(floor(xq), ncols-1), s = xq - j0; i0 = min(floor(yq), nrows-1), t = yq - i0; the +1 taps clamped to the last column / row
 *   B(A) = (A[i0,j0] (1-s) + A[i0,j0+1] s) (1-t) + (A[i0+1,j0] (1-s) + A[i0+1,j0+1] s) t, evaluated in exactly this order
 *   ub = B(Ub), vb = B(Vb), ru = Uf + ub, rv = Vf + vb
 *   e    = ru ru + rv rv
 *   lim  = a ((Uf Uf + Vf Vf) + (ub ub + vb vb)) + b
 *   kept = isfinite(e) && e <= lim
 * the criterion of Sundaram, Brox and Keutzer (ECCV 2010), who use a = 0.01, b = 0.5; a = 0 makes it an absolute threshold.
 * mask_out: 1.0f or 0.0f.  err_out: (float)sqrt(e).  stats_out as above with sqrt(e) in place of |r| (defined: finite e).
 *
 * The statistics are the library's fixed-order float64 tree (thread, wave butterfly, waves ascending, workgroups by a strided
 * fold and the same tree), so a call is reproducible to the bit; the counts are integers held in doubles, exact for any plane.
 * _dev: device pointers (stats_out a device double[4]), launches on `stream`, nothing read back, graph-capturable once the
 * workspace exists; 2 launches with stats_out, 1 without, whatever the data (pdeip_last_launch_count()).  The inputs are never
 * written.  Planes may start at any 4-byte offset.
 * Refused with PDEIP_ERR_ARG before any HIP call: a NULL input, every output NULL, ncols < 2 (the flow call: nrows < 2 as well),
 * nrows < 1, more than 2^31-1 pixels, tol, a or b NaN or negative (+Inf is allowed), an output pointer equal to a gathered plane
 * (D1, Ub, Vb); PDEIP_ERR_UNSUPPORTED: more than 65535 columns. */
int pdeip_disp_crosscheck_dev(void *stream, const float *D0, const float *D1, int nrows, int ncols, double tol, float *sparse_out,
                              float *mask_out, float *diff_out, double *stats_out);
int pdeip_disp_crosscheck(const float *D0, const float *D1, int nrows, int ncols, double tol, float *sparse_out, float *mask_out,
                          float *diff_out, double *stats_out);
int pdeip_flow_crosscheck_dev(void *stream, const float *Uf, const float *Vf, const float *Ub, const float *Vb, int nrows, int ncols,
                              double a, double b, float *mask_out, float *err_out, double *stats_out);
int pdeip_flow_crosscheck(const float *Uf, const float *Vf, const float *Ub, const float *Vb, int nrows, int ncols, double a, double b,
                          float *mask_out, float *err_out, double *stats_out);

/* ---- hole filling: total-variation inpainting of a sparse map (csrc/pdeip_inpaint.hip) ---------------------------------------------
 *
 * This library's own definitions (the reference has no such driver; its solvers carry the mechanism: a pixel whose TRACE is NaN has
 * "no data", pdeSolvers.c:101-114).  Planes are column-major float32 [nrows x ncols (x frames)].  A pixel of D is a hole if it is
 * NaN, per frame; every other value (Inf included) is known.  Single arithmetic without FMA unless stated otherwise.
 *
 * pdeip_nan_resize_dev: with resize = pdeip_pyr_resize_dev(cubic = 0) kept in double,
 *   num = resize(known ? D : 0), den = resize(known ? 1 : 0), out = den >= cover ? (float)(num / den) : NaN.
 * One thread per output pixel walks the tap lists once and accumulates both sums in that order.  cover in (0, 1]; the size limits
 * of pdeip_pyr_resize_dev apply.
 *
 * pdeip_inpaint_meanfill_dev: per frame the known values are summed in double, each column top to bottom starting from 0, the column
 * sums then left to right starting from 0; mean = (float)(sum / count), 0 for a frame without a known pixel.  out = D where known
 * (its bits), the mean on holes.  out may be D.
 *
 * pdeip_tv4_inpaint_assemble_dev: the weights are TVdenoise4.m's DiffWeights (pdeip_tv4_assemble_dev), their maximum over the frames
 * taken over the `nframes` frames of X followed by the guide_channels planes of (float)guide_scale * guide (guide NULL with 0
 * channels).  On a known pixel psi = 1/sqrt((X-D)^2 + eps), TRACE = psi + alpha*(wW+wN+wE+wS), B = psi*D; on a hole TRACE = NaN,
 * B = 0, and D's NaN enters no arithmetic.  The weight planes hold alpha*w, repeated per frame.  With no hole and no guide the
 * outputs are pdeip_tv4_assemble_dev's, bit for bit.
 *
 * pdeip_inpaint_merge_dev: out = D where known (its own bits, -0.0 included), X elsewhere; filled_out (NULL allowed) = 1 on holes,
 * 0 elsewhere.  out may be X or D.
 *
 * Each of the four is one launch on `stream`, whatever the data (pdeip_last_launch_count()).
 *
 * pdeip_tv_inpaint4 (host pointers) / pdeip_tv_inpaint4_dev (resident planes): D [nrows x ncols x frames], guide
 * [nrows x ncols x guide_channels] or NULL with 0 channels, out like D, filled_out like D or NULL.
 *   pyramid   level k+1 has ceil(size*scl_factor) rows and columns, D through pdeip_nan_resize_dev(cover), the guide through
 *             pdeip_pyr_resize_dev, no smoothing; it continues while the smaller side of the next level is >= max(min_size, 3) and
 *             the frame still shrinks
 *   start     X = pdeip_inpaint_meanfill_dev of the coarsest D
 *   level     outer_iter + 1 times [pdeip_tv4_inpaint_assemble_dev; pdeip_pde_sor4_dev | pdeip_pde_alr4_dev(inner_iter, omega)] in
 *             the library's current mode (pdeip_set_mode), coarse to fine; X goes up through pdeip_pyr_resize_dev
 *   end       keep: pdeip_inpaint_merge_dev; otherwise out = X (filled_out is written either way)
 * A flow is filled by handing U, V as two frames: the weights are then joint, as in TVdenoise4.
 * A member of the parameter struct that is <= 0 or NaN keeps its default (alpha 5, omega 1.75, outer_iter 10, inner_iter 5,
 * solver 2, scl_factor 0.75, min_size 16, cover 0.25, guide_scale 20); keep: 0 = no merge, > 0 = merge, < 0 = the default (merge).
 * NULL: all defaults.
 * _dev: launches on `stream`, nothing read back, no control flow on the data (the launch count depends on shape and parameters
 * alone); graph-capturable once an eager call has created the workspace.
 * Refused with PDEIP_ERR_ARG before any HIP call: NULL D or out, a frame below 3x3, frames < 1, more than 2^31-1 elements,
 * scl_factor not below 1, cover above 1, an unknown solver, guide_channels < 0, a guide pointer that disagrees with its channel
 * count; PDEIP_ERR_UNSUPPORTED: more than 65535 columns, a scl_factor that needs more taps than pdeip_pyr_resize_dev has. */
typedef struct pdeip_inpaint_params {
    double alpha, omega, scl_factor, cover, guide_scale;
    int outer_iter, inner_iter, solver, min_size, keep;
} pdeip_inpaint_params;
int pdeip_nan_resize_dev(void *stream, const float *in, int nrows, int ncols, int nframes, int nrows_out, int ncols_out, double cover,
                         float *out);
int pdeip_inpaint_meanfill_dev(void *stream, const float *D, int nrows, int ncols, int nframes, float *out);
int pdeip_tv4_inpaint_assemble_dev(void *stream, const float *X, const float *D, const float *guide, int guide_channels,
                                   double guide_scale, int nrows, int ncols, int nframes, float alpha, float *TRACE, float *B,
                                   float *wW, float *wN, float *wE, float *wS);
int pdeip_inpaint_merge_dev(void *stream, const float *X, const float *D, int nrows, int ncols, int nframes, float *out,
                            float *filled_out);
int pdeip_tv_inpaint4_dev(void *stream, const float *D, int nrows, int ncols, int frames, const float *guide, int guide_channels,
                          const pdeip_inpaint_params *prm, float *out, float *filled_out);
int pdeip_tv_inpaint4(const float *D, int nrows, int ncols, int frames, const float *guide, int guide_channels,
                      const pdeip_inpaint_params *prm, float *out, float *filled_out);

/* ---- frame interpolation: the picture between two frames, from a computed flow (csrc/pdeip_interp.hip) ------------------------------
 *
 * This library's own definitions (the reference has no such function); the algorithm is the baseline of Baker et al., "A Database and
 * Evaluation Methodology for Optical Flow", IJCV 2011, section 3.3.  Planes are column-major float32 [nrows x ncols (x channels)],
 * coordinates 1-based (x = j+1, y = i+1 for the 0-based pixel (i, j)) as in pdeip_flow_crosscheck.  All arithmetic is float64 on the
 * promoted inputs, every product and sum rounded, no FMA, one rounding to float32 on the way out.  0 < t < 1; tq = 1 - t is formed
 * once on the host.  B(A) at (xq, yq) is the bilinear sample of pdeip_flow_crosscheck, one device function for all: in range iff
 * 1 <= xq <= ncols and 1 <= yq <= nrows, the same clamps, the same order of operations.
 *
 * pdeip_flow_splat_dev: the flow (Uf, Vf) of frame 0 -> 1 carried forward to time t.
 *   source   a pixel p = (i, j) with Uf[p], Vf[p] finite; any other pixel splats nothing
 *   cost     with I0, I1 [nrows x ncols x channels] given: c = (float) sum over ch ascending of |I0[p,ch] - B(I1[:,:,ch])| at
 *            (x + Uf, y + Vf), the sum started at 0; out of range, or a NaN sum: c = +Inf.  With I0 == I1 == NULL: c = 0.
 *            c >= +0, so its bit pattern orders as an unsigned integer.
 *   landing  xq = x + t Uf, yq = y + t Vf
 *   targets  columns floor(xq) and, only if xq is not an integer, floor(xq)+1; rows alike: one, two or four pixels, those outside
 *            the frame dropped
 *   winner   per target the smallest 64-bit key (bits(c) << 32) | p, p the 0-based linear index j nrows + i: the lowest cost, ties
 *            to the lowest index.  Keys meet in an integer atomicMin on a plane cleared to all ones, so the order of arrival does
 *            not matter and a call is reproducible to the bit.
 *   resolve  a target no key reached is a hole: Ut = Vt = NaN, cost = NaN.  Otherwise Ut, Vt are the winner's Uf, Vf with their own
 *            bits (-0.0 stays -0.0) and cost_out (NULL allowed) its c.
 * 3 launches (clear, splat, resolve), whatever the data.  Workspace: the key plane, 8 bytes per pixel.
 * Refused with PDEIP_ERR_ARG before any HIP call: NULL Uf, Vf, Ut_out or Vt_out; only one of I0, I1; channels < 1 with images; t not
 * in (0, 1) or NaN; a plane below 3x3; more than 2^31-1 pixels; an output pointer equal to an input pointer.
 * PDEIP_ERR_UNSUPPORTED: more than 65535 columns.
 *
 * pdeip_interp_blend_dev: the picture at time t along a dense flow (Ut, Vt) given at time t.  Per pixel, (u, v) = (Ut, Vt) there:
 *   q0 = (x - t u, y - t v) in frame 0, q1 = (x + tq u, y + tq v) in frame 1
 *   r0, r1   u and v finite and the point in range
 *   a0 = B(I0) at q0, a1 = B(I1) at q1, per channel
 *   p0 = (M0 == NULL) || M0[nearest(q0)] != 0, p1 alike with M1 at q1; nearest: column min(floor(xq + 0.5), ncols), row alike.
 *        M0, M1 (both or neither) are the masks pdeip_flow_crosscheck writes, 1 = consistent: M0 for the forward flow in frame 0,
 *        M1 for the backward flow in frame 1.
 *   case                 It_out                    source_out
 *   neither in range     NaN on every channel      0
 *   only r0              a0                        1
 *   only r1              a1                        2
 *   both, p0 == p1       (float)(tq a0 + t a1)     3
 *   both, p0 && !p1      a1                        2
 *   both, !p0 && p1      a0                        1
 * The last two rows are Baker's occlusion reasoning: a sample that fails its own view's check shows what only that view sees (a
 * background pixel about to be covered exists in frame 0 alone, one just revealed in frame 1 alone), so it is the one taken; the
 * sample that passes its check at that place is the occluder.
 * 1 launch; source_out may be NULL.  Refused as above, and: NULL I0, I1, Ut, Vt or It_out; channels < 1; only one of M0, M1.
 *
 * pdeip_flow_interpolate (host pointers) / pdeip_flow_interpolate_dev (resident planes), in this order:
 *   1  with Ub, Vb (both or neither), the flow of frame 1 -> 0: M0 = mask of pdeip_flow_crosscheck_dev(Uf, Vf | Ub, Vb; a, b) and
 *      M1 = mask of pdeip_flow_crosscheck_dev(Ub, Vb | Uf, Vf; a, b), no statistics
 *   2  pdeip_flow_splat_dev, with the costs of I0, I1 unless use_costs == 0
 *   3  pdeip_tv_inpaint4_dev on (Ut, Vt) as two frames, no guide, parameters `fill` (NULL: its defaults), in the library's current mode
 *   4  pdeip_interp_blend_dev along the filled flow, with M0, M1 if step 1 ran
 * Ut_out, Vt_out (each may be NULL) receive the filled flow at t; source_out may be NULL.  A parameter struct is taken as it stands
 * (a = 0 is an absolute threshold); NULL: a = 0.01, b = 0.5, use_costs = 1, fill = NULL.
 * A field without any finite source is an all-hole plane to step 3, which fills it with zeros: the result is the zero-flow blend.
 * _dev: launches on `stream`, nothing read back, graph-capturable once an eager call has created the workspaces.  The launch count
 * depends on shape and parameters alone and is the sum of its parts: [2] + 3 + pdeip_tv_inpaint4_dev's + 1, plus one copy per
 * Ut_out / Vt_out given (pdeip_last_launch_count()).
 * Refused before any HIP call: what the parts refuse (a, b NaN or negative; the hole filling's parameters), NULL I0, I1, Uf, Vf or
 * It_out, only one of Ub, Vb, an output pointer equal to an input pointer. */
typedef struct pdeip_interp_params {
    double a, b;
    int use_costs;
    const pdeip_inpaint_params *fill;
} pdeip_interp_params;
int pdeip_flow_splat_dev(void *stream, const float *Uf, const float *Vf, const float *I0, const float *I1, int channels, int nrows,
                         int ncols, double t, float *Ut_out, float *Vt_out, float *cost_out);
int pdeip_interp_blend_dev(void *stream, const float *I0, const float *I1, int channels, const float *Ut, const float *Vt,
                           const float *M0, const float *M1, int nrows, int ncols, double t, float *It_out, float *source_out);
int pdeip_flow_interpolate_dev(void *stream, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf,
                               const float *Ub, const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm,
                               float *It_out, float *Ut_out, float *Vt_out, float *source_out);
int pdeip_flow_interpolate(const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub,
                           const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm, float *It_out,
                           float *Ut_out, float *Vt_out, float *source_out);

/* ---- exact Euclidean distance transform: bwdist, signed distance, nearest fill (csrc/pdeip_edt.hip) ----------------------------------
 *
 * This library's own definitions (the reference has no such function; MATLAB's bwdist is the model); tests/edt_ref.py restates them.
 * Planes are column-major float32 [nrows x ncols x frames]; each frame is transformed on its own.
 *
 * pdeip_edt / pdeip_edt_dev.  A pixel is a FEATURE according to `mode`:
 *   PDEIP_EDT_POSITIVE   A > 0    the predicate of bwdist(A > 0) and of pdeip_bwlabel; NaN is not a feature
 *   PDEIP_EDT_NONNEG     A >= 0   the library's "inside" of a level set; -0.0 is inside, NaN is not
 *   PDEIP_EDT_NOT_NAN    A == A   the known pixels of a sparse map; +-Inf is known, as in pdeip_tv_inpaint4
 *   PDEIP_EDT_*_NOT      the complement of each (a NaN is then a feature of the first two)
 * Per pixel (every output may be NULL, but not all three):
 *   d2_out    int32: the exact squared Euclidean distance, in pixels, to the nearest feature
 *   idx_out   int32: the 0-based column-major linear index j nrows + i, within the frame, of that feature
 *   dist_out  float32: (float)sqrt((double)d2), both operations correctly rounded
 * A frame without a feature, or a pixel beyond max_dist: d2 = INT32_MAX, idx = -1, dist = +Inf.
 * Ties: among equidistant features the one with the LOWEST LINEAR INDEX wins -- the smallest column, then the smallest row.  The
 * result therefore does not depend on scheduling and is reproducible to the bit.
 * max_dist <= 0: unbounded.  max_dist = R > 0: features farther than R pixels along either axis are not looked at, and a pixel whose
 * nearest feature has d2 > R^2 reports "none"; this bounds the work per pixel by 2 R + 1 columns.
 * The transform is separable and all integer: a column pass finds every pixel's nearest feature within its own column (the upper of
 * two equidistant ones), a row pass minimises (d^2 + g^2, idx) over the columns j -+ d outward and stops once d^2 exceeds the best
 * squared distance.  Its work per pixel is proportional to the distance found, so it depends on the content: near one pass over the
 * plane for masks and sparse maps, O(ncols) per pixel for a single feature in a large frame.
 * _dev: device pointers, launches on `stream`, nothing read back, graph-capturable once an eager call has created the workspace (one
 * int32 per element); 2 launches (columns, rows), whatever the data (pdeip_last_launch_count()).  A is never written; planes may start
 * at any 4-byte offset.
 * Refused with PDEIP_ERR_ARG before any HIP call: NULL A, all outputs NULL, frames < 1, a side < 1, an unknown mode, more than 2^31-1
 * elements; PDEIP_ERR_UNSUPPORTED: a side above 32767 (d2 must fit an int32).  A 1 x 1 plane is accepted.
 *
 * pdeip_bwdist / pdeip_bwdist_dev: [D, IDX] = bwdist(BW) with the Euclidean metric: the transform in mode PDEIP_EDT_POSITIVE, unbounded;
 * D_out = dist, idx_out = the 0-based idx (either may be NULL, not both).  2 launches.  Refusals as above.
 *
 * pdeip_signed_distance / pdeip_signed_distance_dev: the signed distance of the level set whose inside is A >= 0,
 *   out = dist_to_outside - 0.5   on an inside pixel    (dist of the transform in mode PDEIP_EDT_NONNEG_NOT)
 *   out = -(dist_to_inside - 0.5) on an outside pixel   (dist of the transform in mode PDEIP_EDT_NONNEG)
 * the subtraction a single float32 operation.  The interface lies half-way between an inside pixel and its outside neighbour: |out| is
 * never below 0.5 and the sign of out is the input's side.  A plane that is all inside is +Inf, one that is all outside -Inf.  With
 * max_dist = R > 0 a distance "none" counts as (float)(R + 1), so values beyond the band saturate at +-(R + 0.5): such a plane is
 * what pdeip_ac_solver can take.  5 launches (two transforms, k_sdf_combine); workspace: three planes.  out may be A.  Refused as
 * above, and: NULL out.
 *
 * pdeip_nearest_fill / pdeip_nearest_fill_dev: per frame the transform in mode PDEIP_EDT_NOT_NAN, then one gather launch.  A known
 * pixel keeps its own bits (-0.0 included, as in pdeip_inpaint_merge_dev); a hole takes the bits of D[idx]; a hole without a source
 * (an empty frame, or none within max_dist) stays NaN.  filled_out (NULL allowed): 1 on the holes that were filled, 0 elsewhere;
 * dist_out (NULL allowed): the transform's dist.  3 launches; workspace: two planes.  out may be D.  Refused as above, and: NULL out,
 * filled_out or dist_out equal to another plane of the call.
 * This is the cheapest well-defined fill, NOT a substitute for pdeip_tv_inpaint4 on occlusion bands: the nearest neighbour of an
 * occlusion band is the foreground (3.45 px RMS on the scene of tests/inpaint_cases.py, against 3.11 for the mean and 1.20 for TV).
 *
 * pdeip_flow_interpolate_nearest / _dev: pdeip_flow_interpolate with step 3 replaced: one transform (PDEIP_EDT_NOT_NAN, max_dist) of
 * the splatted Ut's holes -- the splat gives Ut and Vt the same holes -- and one gather of both planes through its index; a hole
 * without a source becomes 0, so a field without any finite source gives the zero-flow blend.  Steps 1, 2 and 4 are the same calls.
 * prm->fill must be NULL (PDEIP_ERR_ARG otherwise); the other refusals are pdeip_flow_interpolate's, and a side above 32767.
 * _dev launches: [2 with Ub, Vb] + 3 (splat) + 2 (transform) + 1 (gather) + 1 (blend), plus one copy per Ut_out / Vt_out given,
 * whatever the data; graph-capturable once an eager call has created the workspaces. */
#define PDEIP_EDT_POSITIVE 0
#define PDEIP_EDT_NONNEG 1
#define PDEIP_EDT_NOT_NAN 2
#define PDEIP_EDT_POSITIVE_NOT 4
#define PDEIP_EDT_NONNEG_NOT 5
#define PDEIP_EDT_NOT_NAN_NOT 6
int pdeip_edt_dev(void *stream, const float *A, int nrows, int ncols, int frames, int mode, int max_dist, int *d2_out, int *idx_out,
                  float *dist_out);
int pdeip_edt(const float *A, int nrows, int ncols, int frames, int mode, int max_dist, int *d2_out, int *idx_out, float *dist_out);
int pdeip_bwdist_dev(void *stream, const float *BW, int nrows, int ncols, int frames, float *D_out, int *idx_out);
int pdeip_bwdist(const float *BW, int nrows, int ncols, int frames, float *D_out, int *idx_out);
int pdeip_signed_distance_dev(void *stream, const float *A, int nrows, int ncols, int frames, int max_dist, float *out);
int pdeip_signed_distance(const float *A, int nrows, int ncols, int frames, int max_dist, float *out);
int pdeip_nearest_fill_dev(void *stream, const float *D, int nrows, int ncols, int frames, int max_dist, float *out, float *filled_out,
                           float *dist_out);
int pdeip_nearest_fill(const float *D, int nrows, int ncols, int frames, int max_dist, float *out, float *filled_out, float *dist_out);
int pdeip_flow_interpolate_nearest_dev(void *stream, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf,
                                       const float *Ub, const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm,
                                       int max_dist, float *It_out, float *Ut_out, float *Vt_out, float *source_out);
int pdeip_flow_interpolate_nearest(const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub,
                                   const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm, int max_dist,
                                   float *It_out, float *Ut_out, float *Vt_out, float *source_out);

/* ---- primal-dual total variation: TV-L1, ROF, Huber-TV (csrc/pdeip_tvpd.hip) ---------------------------------------------------------
 *
 * This library's own call (the reference's TVdenoise4 / TVdenoise8 are lagged-diffusivity TV with a quadratic data term): the
 * first-order primal-dual iteration of Chambolle and Pock for  min_u  TV(u) + lambda |u - f|  (PDEIP_TVPD_L1, which rejects outliers)
 * or  TV(u) + lambda/2 (u - f)^2  (PDEIP_TVPD_L2, ROF), with the Huber norm in place of TV when huber > 0.  No linear solver, no
 * pyramid, no eps.  Planes are column-major float32 [nrows x ncols x frames], i the contiguous row index; each frame on its own.
 * The contract, in float32 without contraction, / and sqrt correctly rounded, in exactly this order; tl = tau lambda, 1 + tl and
 * 1 + sigma huber are each formed once on the host in float32 (tests/tvpd_ref.py restates it, and the device equals it bit for bit).
 * Start: u = u_prev = the start, px = py = 0.  Each of the `iter` iterations:
 *   ub       = (u + u) - u_prev
 *   gx[i,j]  = ub[i+1,j] - ub[i,j]   (0 on the last row);   gy[i,j] = ub[i,j+1] - ub[i,j]   (0 on the last column)
 *   qx       = px + sigma gx;  qy = py + sigma gy;   huber > 0:  qx = qx / (1 + sigma huber), qy likewise
 *   n        = s > 1 ? s : 1  with  s = sqrt(qx qx + qy qy)      (max(1, s); a NaN norm divides by 1)
 *   px'      = qx / n;  py' = qy / n
 *   d        = (px'[i,j] - px'[i-1,j]) + (py'[i,j] - py'[i,j-1])   (a missing neighbour: the term is px'[i,j] / py'[i,j] alone)
 *   v        = u + tau d
 *   L2:  u' = (v + tl f) / (1 + tl)
 *   L1:  u' = v - tl  if v - f > tl;   v + tl  if v - f < -tl;   f  otherwise
 *   f is NaN (no data here):  u' = v
 *   u_prev'  = u
 * px stays exactly 0 on the last row and py on the last column, so 1 x N, N x 1 and 1 x 1 planes need no special case.  +-Inf in f is
 * data; what comes of it is whatever the recurrence gives.
 * The start is u0 if given; with u0 == NULL it is f with its NaNs replaced by pdeip_nearest_fill's result (a frame without a known
 * pixel stays NaN).  iter = 0 returns the start.  tau, sigma: NaN = the defaults 0.25 and 0.5 (tau sigma 8 = 1, both exact in binary).
 * _dev: device pointers, launches on `stream`, nothing read back, graph-capturable once an eager call has created the workspaces
 * (nine planes of its own, and pdeip_nearest_fill's for the start).  f and u0 are never written; planes may start at any 4-byte offset.
 * Kernels: k_tvpd_step does one iteration per launch, k_tvpd_block<T> does T per launch on LDS tiles with a halo of T; both give the
 * same bits.  Environment PDEIP_TVPD_STEPS: unset or 0 the library's choice, 1 single steps, 2 / 4 / 8 blocks of that many.
 * Launches (pdeip_last_launch_count()), a function of iter, T and u0 == NULL alone, with T = 1 for single steps:
 *   [3 with u0 == NULL]  +  (T > 1 ? iter / T + iter % T : iter);   iter = 0:  3 with u0 == NULL, 1 (a copy) otherwise.
 * pdeip_set_mode does not apply.
 * Refused with PDEIP_ERR_ARG before any HIP call: a NULL f, u_out or prm; u_out equal to f or u0; a side or frames < 1; more than
 * 2^31-1 elements; an unknown model; lambda or huber negative or not finite; iter < 0; tau or sigma not positive and finite;
 * tau sigma 8 > 1 (evaluated in double); an unsupported PDEIP_TVPD_STEPS.  PDEIP_ERR_UNSUPPORTED: more than 65535 columns or frames. */
#define PDEIP_TVPD_L1 0
#define PDEIP_TVPD_L2 1
typedef struct {
    int model;     /* PDEIP_TVPD_L1, PDEIP_TVPD_L2 */
    double lambda; /* data weight */
    double huber;  /* 0 = TV, > 0 = Huber-TV */
    int iter;
    double tau;   /* NaN = default */
    double sigma; /* NaN = default */
} pdeip_tvpd_params;
int pdeip_tv_pd_dev(void *stream, const float *f, const float *u0 /* or NULL */, int nrows, int ncols, int frames,
                    const pdeip_tvpd_params *prm, float *u_out);
/* the same without `stream`, on host pointers */
int pdeip_tv_pd(const float *f, const float *u0, int nrows, int ncols, int frames, const pdeip_tvpd_params *prm, float *u_out);

/* ---- TV-L1 optical flow: primal-dual, warped, coarse to fine (csrc/pdeip_tvl1.hip, csrc/pdeip_drivers.hip) -----------------------------
 *
 * This library's own calls (the reference's flow drivers are lagged-diffusivity models solved by SOR or line relaxation): the TV-L1
 * flow of Zach, Pock and Bischof,  min_{u,v}  TV(u, v) + lambda |rho(u, v)|  with rho the brightness constancy linearised about the
 * flow of one warp, by the first-order primal-dual iteration of Chambolle and Pock; the Huber norm in place of TV when huber > 0.
 * No linear solver, no eps.  Planes are column-major float32 [nrows x ncols], i the contiguous row index; x runs along the columns
 * with flow U, y down the rows with flow V.  The contract, in float32 without contraction, / and sqrt correctly rounded, in exactly
 * this order; tl = tau lambda and 1 + sigma huber are each formed once on the host in float32 (tests/tvl1_ref.py restates it, and the
 * device equals it bit for bit).
 *
 * Linearisation of one warp about (U0, V0) -- pdeip_tvl1_rc_dev, 1 launch:
 *   W = frame 1 warped by pdeip_flow_warp_dev;  gx, gy = the Idx, Idy planes of pdeip_fst_derivatives5_dev(I0, W)  (its Idt is not used)
 *   rc = ((W - I0) - gx U0) - gy V0          NaN wherever the warp left the frame: "no data here"
 *
 * The iteration -- pdeip_tvl1_iterate_dev.  State u, v, u_prev, v_prev and the four dual planes pxu, pyu, pxv, pyv.  A call starts from
 * u = u_prev = U, v = v_prev = V and from the duals in P (four planes of nrows x ncols, contiguous, in the order above), or from zero
 * duals with P == NULL.  Each of the `iter` iterations:
 *   ub = (u + u) - u_prev;   vb = (v + v) - v_prev
 *   gxu[i,j] = ub[i+1,j] - ub[i,j] (0 on the last row);  gyu[i,j] = ub[i,j+1] - ub[i,j] (0 on the last column);  gxv, gyv of vb likewise
 *   q*  = p* + sigma g*  for each of the four;   huber > 0: each q* = q* / (1 + sigma huber)
 *   s   = sqrt((qxu qxu + qyu qyu) + (qxv qxv + qyv qyv))      the joint norm of the four
 *   n   = s > 1 ? s : 1                                        (a NaN norm divides by 1)
 *   p*' = q* / n
 *   du  = (pxu'[i,j] - pxu'[i-1,j]) + (pyu'[i,j] - pyu'[i,j-1])   (a missing neighbour: the term is pxu'[i,j] / pyu'[i,j] alone); dv likewise
 *   a   = u + tau du;   b = v + tau dv
 *   g2  = gx gx + gy gy;   rho = (rc + gx a) + gy b;   t = tl g2
 *   c   = rho > t ? -tl : rho < -t ? tl : g2 > 0 ? -rho / g2 : 0
 *   rc is NaN:  u' = a, v' = b;   otherwise:  u' = a + c gx, v' = b + c gy
 *   u_prev' = u;  v_prev' = v
 * Settled here: every comparison with a NaN is false, so a NaN rho or g2 beside a number in rc takes the last two branches in turn (and
 * u', v' become NaN); a pixel with gx = gy = 0 has c = +0 and u' = a + 0 * 0.  +-Inf in rc is data.  pxu and pxv stay exactly 0 on the
 * last row, pyu and pyv on the last column, so 1 x N, N x 1 and 1 x 1 planes need no special case.
 * On return U_out, V_out hold u, v and, with P given, P holds the duals; u_prev, v_prev are not handed on: the next call starts from
 * u_prev = u again.  iter = 0 copies U, V to U_out, V_out and leaves P alone.  Members of prm: NaN = the default (lambda 15, huber 0, tau
 * 0.25, sigma 0.5; tau sigma 8 = 1, both exact in binary); iter has none.  rc, gx, gy, U, V are never written; planes may start at any
 * 4-byte offset.  Kernels: k_tvl1_step does one iteration per launch, each thread recomputing the duals of its north and west
 * neighbour; k_tvl1_block<T> does T per launch on LDS tiles with a halo of T; both give the same bits.  Environment PDEIP_TVL1_STEPS:
 * unset or 0 the library's choice, 1 single steps, 2 / 4 blocks of that many.
 * _dev: device pointers, launches on `stream`, nothing read back, graph-capturable once an eager call has created the workspace
 * (sixteen planes).  Launches (pdeip_last_launch_count()), a function of iter, T and P == NULL alone, with T = 1 for single steps:
 *   iter = 0: 2 (the copies);   iter >= 1: L + [P != NULL and L = 1]  with  L = (T > 1 ? iter / T + iter % T : iter)   (the single
 *   launch of such a call cannot write the planes its neighbours still read, so its duals reach P by a copy)
 * pdeip_set_mode does not apply.
 * Refused with PDEIP_ERR_ARG before any HIP call: a NULL plane (P excepted), prm or output; an output that is an input, the other
 * output or within P; P equal to an input plane; a side < 1; more than 2^31-1 elements; lambda or huber negative or infinite; iter < 0;
 * tau or sigma not positive and finite; tau sigma 8 > 1 (evaluated in double); an unsupported PDEIP_TVL1_STEPS.
 * PDEIP_ERR_UNSUPPORTED: more than 65535 columns.
 *
 * The level -- `warps` times: W = warp of frame 1 by (U, V); gx, gy; rc; `iter` iterations from (U, V); (U, V) = medfilt2 of both
 * (pdeip_median3_pair_dev).  The duals are zero at the start of a scale and persist from warp to warp within it.
 *
 * pdeip_flow_tvl1 -- the whole driver on host pointers, one resident run: Iin [nrows x ncols x 2], gray, 0..255, is divided by 255; the
 * pyramid is that of pdeip_flow_nd_llin (scl_factor 0.75, down to a side <= 20, the 5 x 5 Gaussian of sigma 1.25, the coarsest scale
 * smoothed too); the start is zero; from the coarsest scale on [the level; U (1 / scl_factor) resized bilinearly to the finer scale, no
 * median there]; the duals are not carried between scales.  The frames go up once and U, V [nrows x ncols] come down once.  A member
 * of the parameter struct that is <= 0 or NaN keeps the default (lambda 15, huber 0, tau 0.25, sigma 0.5, scl_factor 0.75, warps 3,
 * iter 20, scales unlimited); NULL: all defaults.  Refused with PDEIP_ERR_ARG before any HIP call: a NULL Iin, U or V; U == V; a side
 * < 2; more than 2^31-1 elements; an infinite lambda or huber; bad step sizes (as above); scl_factor not below 1. */
typedef struct {
    double lambda; /* data weight; NaN = 15 */
    double huber;  /* 0 = TV, > 0 = Huber-TV; NaN = 0 */
    int iter;
    double tau;   /* NaN = default */
    double sigma; /* NaN = default */
} pdeip_tvl1_params;
typedef struct {
    double lambda, huber, tau, sigma, scl_factor;
    int warps, iter, scales;
} pdeip_flow_tvl1_params;
int pdeip_tvl1_rc_dev(void *stream, const float *I0, const float *W, const float *gx, const float *gy, const float *U0, const float *V0,
                      int nrows, int ncols, float *rc);
int pdeip_tvl1_iterate_dev(void *stream, const float *rc, const float *gx, const float *gy, const float *U, const float *V,
                           float *P /* or NULL */, int nrows, int ncols, const pdeip_tvl1_params *prm, float *U_out, float *V_out);
int pdeip_flow_tvl1(const float *Iin, int nrows, int ncols, const pdeip_flow_tvl1_params *prm, float *U, float *V);

/* ---- structure-tensor anisotropic diffusion (csrc/pdeip_stensor.hip) --------------------------------------------------------
 * Weickert's edge-enhancing (EED) and coherence-enhancing (CED) diffusion, each semi-implicit step (I - tau A(u^k)) u^{k+1} = u^k
 * one PDEsolver8 solve by pdeip_pde_sor8_dev / pdeip_pde_alr8_dev.  Not in the reference toolbox; tests/stensor_ref.py restates
 * every stage.  Planes are single, column-major [nrows x ncols x frames]; x runs along the columns, y down the rows.
 *
 * pdeip_gauss_taps (host only, no HIP call): R = ceil(3 sigma) and the 2R + 1 taps g[k] = exp(-k^2 / (2 sigma^2)), k = -R..R, in
 * double, divided by their double sum (added in ascending k), each rounded to single; sigma = 0: R = 0 and the tap 1.  The
 * ceiling is that of the exact product: sigma = 32 / 3 as a double has R = 32, the next double above it needs 33 and is refused
 * (its double product rounds to 32.0).  A sigma whose square underflows (1e-200) has R = 1 and the taps 0, 1, 0.
 * PDEIP_ERR_ARG: sigma NaN, negative or infinite, capacity < 2R + 1 (nothing written); PDEIP_ERR_UNSUPPORTED: R > 32.
 *
 * pdeip_gauss / pdeip_gauss_dev: out = G_sigma * in, separable, border 'replicate'.  Pass 1 runs along the rows (down a column)
 * and its result is rounded to single; pass 2 runs along the columns.  Each output of a pass is
 * ((g[-R] x[-R] + g[-R+1] x[-R+1]) + ...) + g[R] x[R] in single, left to right, no FMA, indices clamped to the frame.
 * sigma = 0 is a copy (1 launch), otherwise 2 launches; the intermediate plane is library workspace.  Refused before any HIP
 * call: what pdeip_gauss_taps refuses, a NULL pointer, a frame below 3x3, frames < 1, more than 2^31-1 elements, out == in
 * (PDEIP_ERR_ARG); more than 65535 columns or frames (PDEIP_ERR_UNSUPPORTED).
 *
 * pdeip_structure_tensor_dev: J = [J11, J12, J22], three planes [nrows x ncols], of I [nrows x ncols x channels]:
 *   v   = G_sigma * I per channel (pdeip_gauss_dev; sigma = 0: I itself)
 *   gx, gy  the Alvarez 3x3 derivative of v toward increasing column / row, border 'replicate', single: with w1 = 1/(4 + sqrt 8) and
 *       w2 = sqrt 2/(4 + sqrt 8) rounded to single, d-, d0, d+ the differences v(., j+1) - v(., j-1) on rows i-1, i, i+1 (for gy:
 *       v(i+1, .) - v(i-1, .) on columns j-1, j, j+1), the derivative is (w1 d- + w2 d0) + w1 d+
 *   J11 = sum_c gx^2, J12 = sum_c gx gy, J22 = sum_c gy^2, single, channel 0's product first and the others added in index order
 *       (Weickert's joint tensor of a colour image)
 *   J   = G_rho * J as three frames (rho = 0: the products themselves)
 * 2 [sigma > 0] + 1 + 2 [rho > 0] launches.  Refused as pdeip_gauss_dev refuses, for both scales; J == I.
 *
 * pdeip_st_weights_dev: the diffusion tensor and the eight weights, w8 = eight planes [nrows x ncols] in the order W NW N NE E
 * SE S SW.  Per pixel, in double from the single J:
 *   s = j11 + j22, d = j11 - j22, r = sqrt(d d + 4 j12 j12), mu1 = 0.5 (s + r), c2 = r > 0 ? d / r : 1, s2 = r > 0 ? 2 j12 / r : 0
 *   EED (mode 0): l1 = mu1 > 0 ? 1 - exp(-3.31488 / q^4) : 1 with q = mu1 / (lambda lambda), q^4 = (q q)(q q); l2 = 1
 *   CED (mode 1): l1 = alpha; l2 = r > 0 ? alpha + (1 - alpha) exp(-C / (r r)) : alpha
 *   m = 0.5 (l1 + l2), h = 0.5 (l1 - l2), D11 = m + h c2, D22 = m - h c2, D12 = h s2
 *   the eight weights by TVdenoise8's assembly with dyy := D11, dxx := D22, dxy := D12 (wW = (D11 + D11 of the west pixel) / 2, wN =
 *   (D22 + D22 north) / 2, wNW = (D12 + D12 north-west) / 4, wNE = -(D12 + D12 north-east) / 4, and so on), a weight across the
 *   frame's edge zero; sum = ((wW + wNW) + wN) + ... + wSW; w8[k] = (float)(tau w_k), TRACE = (float)(1 + tau sum).
 * A NaN in J fails every comparison above (a flat pixel's tensor).  An Inf in j11 or j22 passes them: r = Inf, c2 = Inf / Inf = NaN and s2 =
 * 2 j12 / Inf = 0, so D11 and D22 of that pixel are NaN and D12 is finite: TRACE and the four axial weights (W, N, E, S) are NaN at
 * the pixel and TRACE and the one axial weight that reads it at each of its four axial neighbours (5 NaN in TRACE, 2 in each axial
 * plane for an interior pixel), the diagonal weights stay finite.  The weights across the frame's edge are zero by selection, not
 * by a product, so a non-finite tensor on one edge of the frame leaves the opposite edge as it was.  Only mode, lambda, alpha and C of `prm` are read (NaN or
 * prm == NULL: the defaults below); tau is the argument.  1 launch.  Refused before any HIP call: a NULL plane, a frame below 3x3,
 * more than 65535 columns, an unknown mode, lambda <= 0 or not finite (EED), alpha outside [0, 1], C <= 0 or not finite (CED), tau
 * NaN, negative or infinite.
 *
 *
 * The ring.  PDEsolver8 relaxes the interior of a plane and after every sweep copies the neighbours into the plane's outer ring
 * of pixels (pdeSolvers.c:249-262).  Handed the image as it is, it would never relax the image's edge pixels, and the copies make
 * the structure tensor there degenerate: on the scene of tests/test_stensor_ref.py ten such iterations leave an RMS error of 66
 * on the first row and of 17 overall, against 7.9 when every pixel is relaxed.  So a step solves on planes [(nrows + 2) x
 * (ncols + 2)] that hold the image inside a ring of one pixel: every pixel of the image is an interior pixel of the solve; its
 * weights across the image's edge are zero (no flux, the system symmetric with unit row sums); the ring is the solver's.
 *   pdeip_st_weights_padded_dev  pdeip_st_weights_dev onto such planes: TRACE [(nrows+2) x (ncols+2)] and w8, eight of them, hold
 *                                the image's values inside and TRACE = 1, weights 0 on the ring.  1 launch.
 *   pdeip_st_pad_dev             out (and out2 unless NULL) [(nrows+2) x (ncols+2) x frames] = in [nrows x ncols x frames] inside a
 *                                ring of its nearest pixels.  1 launch; out == in refused.
 *   pdeip_st_crop_dev            out [nrows x ncols x frames] = the inside of in.  1 launch; out == in refused.
 * These refuse what pdeip_st_weights_dev / pdeip_gauss_dev refuse for the frame, and more than 65533 columns.
 *
 * pdeip_diffusion8 / pdeip_diffusion8_dev: Iout = the filtered Iin, both [nrows x ncols x channels], 0..255 data as Diffusion4_v10
 * takes it; Iout == Iin is allowed, otherwise Iin is untouched.  Iout = Iin, then `iters` times: J of Iout; the weights and
 * TRACE (padded); X = B = Iout inside its ring (pdeip_st_pad_dev, all channels at once); per channel one call of
 * pdeip_pde_sor8_dev (solver 1, inner_iter sweeps at omega) or pdeip_pde_alr8_dev (solver 2: one iteration whatever inner_iter
 * says, like the reference) in place on the channel's X, nframes = 1, in the library's current ordering (pdeip_set_mode), every
 * channel on the one set of weight planes; Iout = the inside of X (pdeip_st_crop_dev).
 * Every member is a double; NaN (or prm == NULL) takes the default:
 *   mode 1 (CED): sigma 0.7, rho 4, alpha 0.001, C 1;  mode 0 (EED): sigma 1.5, rho 0, lambda 6;
 *   both: tau 1, iters 10, solver 1, inner_iter 4, omega 1.  Counts are floored; a negative count is none.
 * At tau = 1 every row of the system stays weakly diagonally dominant; at tau = 2 it does not.
 * _dev: one stream, nothing read back, no allocation once an eager call has created the workspaces: graph-capturable.  Launches
 * (pdeip_last_launch_count()), a function of shape and parameters alone:
 *   [Iout != Iin] + iters * (2 [sigma > 0] + 1 + 2 [rho > 0] + 3 + channels * L)
 * with L what pdeip_last_launch_count() reports after the solver call on one [(nrows+2) x (ncols+2)] plane in the current ordering.
 * Refused before any HIP call: a NULL pointer; a frame below 3x3, channels < 1, more than 2^31-1 elements; sigma, rho or tau NaN,
 * negative or infinite; what pdeip_st_weights_dev refuses; omega not finite in single; an infinite or over-large iters or
 * inner_iter; a workspace (3 planes of the image, 9 + 2 channels planes with the ring) of more than 2^31-1 elements
 * (PDEIP_ERR_ARG); a solver other than 1 or 2 (PDEIP_ERR_SOLVER); a radius above 32, more than 65533 columns or 65535 channels
 * (PDEIP_ERR_UNSUPPORTED). */
typedef struct pdeip_diffusion8_params {
    double mode, sigma, rho, lambda, alpha, C, tau, iters, inner_iter, omega, solver;
} pdeip_diffusion8_params;
int pdeip_gauss_taps(double sigma, float *taps, int capacity, int *radius);
int pdeip_gauss(const float *in, int nrows, int ncols, int frames, double sigma, float *out);
int pdeip_gauss_dev(void *stream, const float *in, int nrows, int ncols, int frames, double sigma, float *out);
int pdeip_structure_tensor_dev(void *stream, const float *I, int nrows, int ncols, int channels, double sigma, double rho, float *J);
int pdeip_st_weights_dev(void *stream, const float *J, int nrows, int ncols, const pdeip_diffusion8_params *prm, double tau,
                         float *TRACE, float *w8);
int pdeip_st_weights_padded_dev(void *stream, const float *J, int nrows, int ncols, const pdeip_diffusion8_params *prm, double tau,
                                float *TRACE, float *w8);
int pdeip_st_pad_dev(void *stream, const float *in, int nrows, int ncols, int frames, float *out, float *out2);
int pdeip_st_crop_dev(void *stream, const float *in, int nrows, int ncols, int frames, float *out);
int pdeip_diffusion8(const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion8_params *prm, float *Iout);
int pdeip_diffusion8_dev(void *stream, const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion8_params *prm,
                         float *Iout);

#ifdef __cplusplus
}
#endif
#endif /* PDEIP_H */
