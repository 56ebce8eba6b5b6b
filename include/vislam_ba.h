/*
 * vislam_ba.h -- C ABI of the MI355X local bundle-adjustment backend.
 *
 * Drop-in boundary.  The reference (mc275/MC_SLAM) has no FFI layer; the boundary
 * is the point where its host code hands a freshly built factor graph to g2o:
 *
 *     optimizer.initializeOptimization(); optimizer.optimize(5); ... optimizer.optimize(10);
 *       src/Optimizer.cpp:458-493   (Optimizer::LocalBAPRVIDP,            variant 2)
 *       src/Optimizer.cpp:1259-1317 (Optimizer::LocalBundleAdjustmentNavStatePRV, variant 1)
 *       src/Optimizer.cpp:4093-4143 (Optimizer::LocalBundleAdjustment,    variant 0)
 *
 * Everything g2o does between those lines (active-set construction, residuals + analytic Jacobians,
 * Huber weighting, H/b assembly, Schur complement, reduced solve, back-substitution, manifold update,
 * GN / LM control flow, the two-stage outlier protocol) happens behind vba_solve().  The host keeps graph
 * extraction (src/Optimizer.cpp:49-451) and write-back (:496-623).
 *
 * Plain C: flat caller-owned arrays, f64 + i32, no C++ / torch types across the line.
 */
#ifndef VISLAM_BA_H
#define VISLAM_BA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBA_VARIANT_SE3_XYZ 0 /* VertexSE3Expmap + VertexSBAPointXYZ + EdgeSE3ProjectXYZ (types_six_dof_expmap.h:80) */
#define VBA_VARIANT_PRV_XYZ 1 /* VertexNavStatePR/V/Bias + XYZ + EdgeNavStatePRPointXYZ (g2otypes.h:255)          */
#define VBA_VARIANT_PRV_IDP 2 /* VertexNavStatePR/V/Bias + VertexIDP + EdgePRIDP (g2otypes.h:22,65)                */

#define VBA_ALGO_GN 0 /* OptimizationAlgorithmGaussNewton with the |dchi2|<1e-3 stop (gauss_newton.cpp:97) */
#define VBA_ALGO_LM 1 /* OptimizationAlgorithmLevenberg, g2o lambda/rho schedule (levenberg.cpp:61-164)    */

#define VBA_PROTO_LOCAL 0  /* optimize(its_stage1); outlier pass; optimize(its_stage2): the LocalBA functions */
#define VBA_PROTO_SINGLE 1 /* one optimize(its_stage1), no outlier pass: BundleAdjustment / GlobalBundleAdjustmentNavStatePRV
                            * (src/Optimizer.cpp:3377-3607, 629-933) */

#define VBA_SOLVER_LDLT 0 /* dense LDL^T on 32x32 tiles of the reduced system: what LinearSolverEigen does (linear_solver_eigen.h:94-124) */
#define VBA_SOLVER_PCG 1  /* block-Jacobi preconditioned conjugate gradients on the reduced system (not in the reference: BASELINE
                           * north_star / configs[3] "Schur + PCG"); tolerance 1e-10, so the outer iterations follow the direct path */

#define VBA_IMU_MEAS_STRIDE 61 /* dt, dP(3), dV(3), dR(9 row-major), JPg, JPa, JVg, JVa, JRg (9 each, row-major) */
#define VBA_TRACE_MAX 64

/* status values of vba_result.status */
#define VBA_OK 0
#define VBA_ABORTED_AFTER_STAGE1 1 /* stop flag seen after optimize(5): src/Optimizer.cpp:464-470 */
#define VBA_ABORTED_BEFORE 2       /* stop flag set on entry: src/Optimizer.cpp:453-455, nothing touched */
#define VBA_SOLVER_FAILED (-2)     /* reduced system not positive definite (linear_solver_eigen.h:105-111 -> Fail) */

typedef struct vba_problem {
    int32_t variant;          /* VBA_VARIANT_* */
    int32_t n_kf, n_kf_free;  /* free keyframes first (hessian order = caller order), fixed after */
    int32_t n_pt, n_obs, n_imu;
    /* keyframe state, updated IN PLACE for the free entries.
     * variant 0: T_cw as SE3Quat  (tx ty tz qx qy qz qw)          se3quat.h:40-47
     * variant 1,2: NavState P, R  (px py pz qx qy qz qw) = T_wb   src/IMU/NavState.h:124-138 */
    double *kf_pose;          /* [n_kf][7] */
    double *kf_vel;           /* [n_kf][3]  (variants 1,2; only KFs touched by IMU edges are read) */
    double *kf_bias;          /* [n_kf][12] bg(3) ba(3) dbg(3) dba(3); only dbg,dba are optimised */
    /* landmarks, updated IN PLACE.  variant 0,1: world xyz.  variant 2: rho, xbar, ybar (rho updated;
     * xbar,ybar = normalised ref-KF pixel, src/Optimizer.cpp:382-385) */
    double *pt;               /* [n_pt][3] */
    const int32_t *pt_ref_kf; /* [n_pt] variant 2: reference keyframe index (may be a fixed KF) */
    const int32_t *pt_obs_begin; /* [n_pt+1] CSR: observations of point p are [begin[p], begin[p+1]) */
    const int32_t *obs_kf;    /* [n_obs] observing keyframe (variant 2: never the reference KF, :395-398) */
    const double *obs_uv;     /* [n_obs][2] undistorted pixel (kpUn.pt) */
    const double *obs_w;      /* [n_obs] invSigma2 of the keypoint octave (information = w * I2) */
    double K[4];              /* fx fy cx cy */
    double T_cb[7];           /* camera<-body extrinsic, t_cb(3) q_cb(4) (variants 1,2; ConfigParam::GetEigT_cb) */
    double g_w[3];            /* gravity in world (variants 1,2) */
    const int32_t *imu_kf_i;  /* [n_imu] keyframe i (previous) */
    const int32_t *imu_kf_j;  /* [n_imu] keyframe j (owner of the preintegrator, pKF1) */
    const double *imu_meas;   /* [n_imu][VBA_IMU_MEAS_STRIDE] */
    const double *imu_info_prv; /* [n_imu][81] row-major information of EdgeNavStatePRV in P,phi,V order
                                 * (= inverse of the V/phi-swapped covariance, src/Optimizer.cpp:273-280) */
    double inv_bg_rw2, inv_ba_rw2; /* 1/IMUData::getGyrBiasRW2(), 1/getAccBiasRW2(); bias info = diag/dt (:244-249,302) */
    double huber_vis, huber_prv, huber_bias; /* Huber deltas (float-rounded sqrt(5.991), sqrt(2166.6), sqrt(1681.2)) */
    int32_t algo;             /* VBA_ALGO_* */
    int32_t its_stage1, its_stage2; /* 5, 10 */
    double chi2_th;           /* 5.991 */
    double depth_min;         /* isDepthPositive threshold: 0.01 (EdgePRIDP, g2otypes.h:122-127) or 0.0 */
    double rho_min;           /* 2e-6 (variant 2 outlier gate, src/Optimizer.cpp:484) */
    /* --- global bundle adjustment; all zero / NULL = the local-BA protocol above --- */
    int32_t protocol;         /* VBA_PROTO_* */
    int32_t robust;           /* VBA_PROTO_SINGLE only: bRobust -- Huber on every edge (1) or none at all (0) */
    const uint8_t *kf_fix;    /* NULL or [n_kf]: per-vertex setFixed() of the keyframes listed as free: bit0 PR, bit1 V,
                               * bit2 Bias (GlobalBundleAdjustmentNavStatePRV fixes PR and Bias of keyframe 0 but not
                               * its V: src/Optimizer.cpp:667-685) */
    int32_t solver;           /* VBA_SOLVER_*: how the reduced system is solved (0 = LDL^T, the reference's choice) */
} vba_problem;

typedef struct vba_result {
    double chi2_vis;   /* sum e'We over level-0 vision edges at the final estimates (N3 in SURVEY 8a) */
    double chi2_prv;   /* same for EdgeNavStatePRV */
    double chi2_bias;  /* same for EdgeNavStateBias */
    int32_t its_done[2];  /* outer iterations executed by optimize(5) / optimize(10) (cjIterations) */
    int32_t n_outliers;   /* number of set entries of obs_outlier */
    int32_t status;       /* VBA_OK / VBA_ABORTED_* / VBA_SOLVER_FAILED */
    uint8_t *obs_outlier; /* [n_obs] caller-allocated or NULL: 1 = host must erase (src/Optimizer.cpp:509-514) */
    double *obs_chi2;     /* [n_obs] caller-allocated or NULL: e->chi2() as the reference's erase loop reads it */
    int32_t n_trace;      /* entries of chi2_trace */
    double chi2_trace[VBA_TRACE_MAX]; /* activeRobustChi2 after every accepted/terminating evaluation (diagnostic) */
    double lambda_final;  /* LM only */
    int32_t lin_iterations; /* VBA_SOLVER_PCG: conjugate-gradient iterations summed over all solves of the window (0 for LDL^T) */
} vba_result;

/* Per-kernel-class device time of the last vba_batch_run, measured with HIP events on the backend's
 * own stream (only filled when profiling is enabled with vba_set_profile). */
#define VBA_PROF_LINEARIZE 0
#define VBA_PROF_CONTROL 1
#define VBA_PROF_SCHUR 2
#define VBA_PROF_FACTOR 3
#define VBA_PROF_TRSV 4
#define VBA_PROF_UPDATE 5
#define VBA_PROF_MISC 6
#define VBA_PROF_N 8
typedef struct vba_profile {
    double ms[VBA_PROF_N];       /* summed device time per class */
    int64_t launches[VBA_PROF_N];
    double bytes[VBA_PROF_N];    /* algorithmic bytes moved per class (SURVEY 8d accounting) */
    double total_ms;             /* first launch -> last launch of the run */
    double factor_flops;         /* FP64 flop the factorisation class executed on MFMA: 2*32^3 per tile product of the
                                    symbolic tile lists, per solve (structurally zero tiles are never touched) */
    int64_t kernel_launches;     /* kernel launches the last vba_batch_run / vba_solve / vba_sim3_optimize / vba_sim3_ransac / vba_triangulate / vba_two_view_init (at most 2) / vba_search_triangulation / vba_fuse / vba_search_by_sim3 / vba_search_by_projection / vba_search_by_projection_kf / vba_search_by_bow / vba_posegraph_optimize enqueued (filled with or without profiling) */
} vba_profile;

/* One handle per host thread / GPU; owns device buffers and a stream.  Errors: nonzero return, message
 * via vba_last_error.  Never throws, never aborts. */
int vba_create(int device, void **handle);
int vba_destroy(void *handle);
const char *vba_last_error(void *handle);

/* Replaces optimizer.initializeOptimization(); optimize(its_stage1); <outlier pass>; optimize(its_stage2)
 * (src/Optimizer.cpp:458-493 / 4093-4143).  stop_flag (may be NULL) plays g2o's forceStopFlag
 * (sparse_optimizer.h:188): polled before the solve, between outer iterations and between the stages. */
int vba_solve(void *handle, vba_problem *inout, vba_result *out, const volatile int *stop_flag);

/* Batched / device-resident form: independent windows solved in lock-step on one GPU.
 * upload = H2D + structure build (g2o buildStructure, block_solver.hpp:143-295);
 * run    = the whole two-stage solve from the uploaded initial state, everything HBM-resident;
 * download = D2H of states and per-edge results into the caller's arrays.
 * run may be repeated (each run restarts from the uploaded state). */
int vba_batch_upload(void *handle, int32_t n_windows, vba_problem *const *problems);
int vba_batch_run(void *handle, const volatile int *stop_flag);
int vba_batch_download(void *handle, int32_t n_windows, vba_problem *const *inout, vba_result *const *out);

/* Streamed form of the same: n FRESH windows in, n solved windows out (states updated in place, results filled), for callers
 * that have many independent windows at once (map-server replays, multi-session back-ends).  Equivalent to
 * upload + run + download of the whole batch, but the call cuts the batch into chunks and keeps several in flight, so the
 * host packing, the PCIe transfers and the structure build of one chunk overlap the solve of another. */
int vba_batch_solve(void *handle, int32_t n_windows, vba_problem *const *inout, vba_result *const *out,
                    const volatile int *stop_flag);

/* The same three entry points for a caller whose flag is a C++ `bool` (one byte): the reference hands `bool* pbStopFlag` =
 * &LocalMapping::mbAbortBA down to g2o (include/Optimizer.h:22-24; written by the Tracking thread, src/LocalMapping.cpp:1769-1772).
 * The flag is read at its own width, so `Optimizer::LocalBAPRVIDP` passes its argument straight through -- no mirror word, no
 * helper thread.  (sizeof(bool) == 1 on every ABI the library is built for; the facade static_asserts it.) */
int vba_solve_b(void *handle, vba_problem *inout, vba_result *out, const volatile unsigned char *stop_flag);
int vba_batch_run_b(void *handle, const volatile unsigned char *stop_flag);
int vba_batch_solve_b(void *handle, int32_t n_windows, vba_problem *const *inout, vba_result *const *out,
                      const volatile unsigned char *stop_flag);

/* Asynchronous form of vba_batch_solve, for a caller that produces one batch after another: batch k+1 is packed, copied and
 * structured while batch k solves.
 *   submit  returns at once with a ticket (strictly increasing per handle, from 1); it neither blocks nor reads the windows, and
 *           tickets queue without bound.  The two pointer arrays are copied at submit; the vba_problem / vba_result structs, every
 *           array they point to and the stop flag must stay valid and unmodified until vba_batch_wait of the ticket returns (or
 *           vba_batch_poll returns 0).  The results land in the caller's arrays, as with vba_batch_solve.
 *   order   batches are uploaded one at a time in ticket order and solved one at a time in ticket order, each as ONE run (never
 *           chunked); a download may overlap the next solve.  At most `depth` batches hold device buffers at once; a batch whose
 *           arena is not free yet waits inside the library.
 *   results for any state of the stop flag, bit for bit what vba_batch_solve / _b gives for the same batch and flag (with no flag
 *           set: what vba_batch_upload + run + download of the batch gives).
 *   errors  wait returns 0 or -1; on -1 vba_last_error reads "vba_batch_submit, ticket T, windows 0..n-1: <message>".  A window
 *           rejected by the upload fails that ticket only.  A HIP error (launch, copy, synchronisation) fails that ticket and
 *           every later one, those submitted afterwards included, with the same message: no GPU work starts for them (earlier
 *           tickets finish).  Waiting on an unknown or retired ticket returns -1.
 *   handle  while any ticket is submitted and not yet waited for, every synchronous entry point of the handle (vba_solve*,
 *           vba_batch_upload / run / download / solve*, vba_pose_optimize, vba_sim3_optimize, vba_sim3_ransac, vba_triangulate, vba_two_view_init, vba_search_triangulation, vba_fuse, vba_search_by_sim3, vba_search_by_projection, vba_search_by_projection_kf, vba_search_by_bow, vba_posegraph_optimize, vba_preintegrate, vba_set_profile,
 *           vba_batch_set_depth) returns -1 with "asynchronous batches pending: wait for them first"; afterwards the handle
 *           works synchronously as before.  vba_destroy finishes pending tickets (their results land) before it frees.
 *           Profiling (vba_set_profile) covers synchronous calls only.  One caller thread at a time, as everywhere. */
int vba_batch_set_depth(void *handle, int32_t depth);   /* batches resident on the device at once: 1..4, default 2 */
int vba_batch_submit(void *handle, int32_t n_windows, vba_problem *const *inout, vba_result *const *out,
                     const volatile int *stop_flag, int64_t *ticket);
int vba_batch_submit_b(void *handle, int32_t n_windows, vba_problem *const *inout, vba_result *const *out,
                       const volatile unsigned char *stop_flag, int64_t *ticket);
int vba_batch_poll(void *handle, int64_t ticket);       /* 1 pending, 0 finished (wait will not block), -1 unknown ticket */
int vba_batch_wait(void *handle, int64_t ticket);       /* the batch's return code; retires the ticket */

/* On-device IMU preintegration: IMUPreintegrator::update (src/IMU/IMUPreintegrator.cpp:63-112) applied
 * over the samples of n_edges keyframe intervals, the way KeyFrame::ComputePreInt feeds it (src/KeyFrame.cpp:195-252:
 * the caller lists the samples and their dt, including the duplicated first sample).  gyr/acc are bias-corrected
 * (measurement - bias of the previous keyframe).  Outputs, per interval: imu_meas[VBA_IMU_MEAS_STRIDE] and the 9x9
 * covariance in P,V,phi order as the reference keeps it; imu_info_prv (may be NULL) = inverse of the V/phi-swapped
 * covariance, i.e. exactly what vba_problem.imu_info_prv expects (src/Optimizer.cpp:273-280). */
int vba_preintegrate(void *handle, int32_t n_edges, const int32_t *sample_begin, const double *gyr, const double *acc,
                     const double *dt, double gyr_meas_cov, double acc_meas_cov, double *imu_meas, double *cov_pvphi,
                     double *imu_info_prv);

/* ---- IMU-aided per-frame pose optimisation ----
 * Optimizer::PoseOptimization(Frame*, KeyFrame* pLastKF, IMUPreintegrator, gw, bComputeMarg)   src/Optimizer.cpp:2046-2317
 * Optimizer::PoseOptimization(Frame*, Frame*   pLastFrame, IMUPreintegrator, gw, bComputeMarg) src/Optimizer.cpp:1671-2044
 * Optimizer::PoseOptimization(Frame*)  (vision only, BASELINE configs[0])                        src/Optimizer.cpp:3610-3835
 * Everything between the vertex set-up and the write-back: the four optimize(10) rounds of Levenberg-Marquardt on the
 * 6-, 15- or 30-dimensional system, the chi2 > 5.991 reclassification after every round, the kernel removal after the third,
 * and computeMarginals.  One call solves a batch of independent frames (one workgroup per frame). */
#define VBA_FRAME_KF 0
#define VBA_FRAME_FRAME 1
#define VBA_FRAME_VISION 2
#define VBA_NAV_STRIDE 22 /* NavState: P(3) q(4, xyzw) V(3) bg(3) ba(3) dbg(3) dba(3)   src/IMU/NavState.h:124-138 */
typedef struct vba_frame_problem {
    int32_t last_is_frame;  /* VBA_FRAME_*: 0 last keyframe, fixed (:2082-2097); 1 last frame, free, tied to its marginal prior
                             * (:1710-1747); 2 vision only: nav[0..6] is T_cw as SE3Quat (t, q xyzw), one VertexSE3Expmap +
                             * EdgeSE3ProjectXYZOnlyPose edges (:3623-3672), no IMU fields are read */
    int32_t compute_marg;   /* bComputeMarg */
    int32_t n_obs;          /* monocular correspondences of the frame (mvpMapPoints[i] != NULL, mvuRight[i] < 0) */
    int32_t n_obs_last;     /* those of the last frame (last_is_frame only) */
    double nav[VBA_NAV_STRIDE];      /* in: pFrame->GetNavState(); out: the optimised state (P, R, V, dbg, dba change) */
    double nav_last[VBA_NAV_STRIDE]; /* pLastKF / pLastFrame NavState; never written back by the reference */
    const double *obs_pw;   /* [n_obs][3] MapPoint world positions */
    const double *obs_uv;   /* [n_obs][2] undistorted keypoints */
    const double *obs_w;    /* [n_obs] invSigma2 */
    const double *last_pw, *last_uv, *last_w; /* the same for the last frame */
    double K[4];            /* fx fy cx cy */
    double T_cb[7];         /* as in vba_problem */
    double g_w[3];
    double imu_meas[VBA_IMU_MEAS_STRIDE]; /* imupreint (last -> current) */
    double imu_cov_pvphi[81];             /* its covariance; information of EdgeNavStatePVR = inverse, same P,V,phi order */
    double prior_nav[VBA_NAV_STRIDE];     /* pLastFrame->mNavStatePrior (last_is_frame) */
    double prior_info[225];               /* pLastFrame->mMargCovInv, row-major 15x15, order P V phi bg ba */
    double inv_bg_rw2, inv_ba_rw2;
} vba_frame_problem;

typedef struct vba_frame_result {
    int32_t n_inliers;      /* the function's return value: nInitialCorrespondences - nBad (0 if fewer than 3 correspondences) */
    int32_t status;         /* VBA_OK */
    int32_t its_done[4];    /* LM iterations of each round */
    uint8_t *outlier;       /* [n_obs] caller-allocated: pFrame->mvbOutlier */
    uint8_t *outlier_last;  /* [n_obs_last] caller-allocated or NULL: pLastFrame->mvbOutlier */
    double chi2_round[4];   /* activeRobustChi2 at the end of each round (diagnostic) */
    double marg_cov_inv[225]; /* pFrame->mMargCovInv when compute_marg (pFrame->mNavStatePrior = the returned nav) */
} vba_frame_result;

int vba_pose_optimize(void *handle, int32_t n_frames, vba_frame_problem *const *inout, vba_frame_result *const *out);

/* ---- loop-closure Sim3 refinement ----
 * Optimizer::OptimizeSim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, g2o::Sim3&, th2, bFixScale)   src/Optimizer.cpp:4579-4785
 * Everything between the edge set-up (:4623-4720) and the write-back (:4727-4784): optimize(5) with Levenberg-Marquardt on the
 * one VertexSim3Expmap (types_seven_dof_expmap.h:48-94), the chi2 > th2 test of EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ
 * (:130-171) of every matched pair, the early exit when fewer than 10 pairs are left, optimize(10 or 5) on the survivors, the
 * inlier count.  The map points are fixed vertices, so the caller passes them in the two cameras' frames.  One call refines a
 * batch of independent candidates (one workgroup per candidate, one kernel launch per call).  Jacobians are analytic; the
 * reference differentiates both edges numerically (DESIGN.md gives the measured difference). */
typedef struct vba_sim3_problem {
    int32_t n_pairs;        /* matched map-point pairs that passed the reference's filters (:4640-4678); 0 is legal */
    int32_t fix_scale;      /* bFixScale: VertexSim3Expmap::_fix_scale (update[6] = 0, types_seven_dof_expmap.h:64-65) */
    double  S12[8];         /* in/out: g2o::Sim3 as t(3) q(4, xyzw) s, maps KF2-camera into KF1-camera coordinates (sim3.h:144-146).
                             * Written back only when the candidate survives the first test (:4755-4756, :4781-4782) */
    const double *p1c, *p2c;   /* [n_pairs][3] map points in KF1's / KF2's camera frame (P3D1c, P3D2c: :4659-4669) */
    const double *uv1, *uv2;   /* [n_pairs][2] undistorted keypoints in KF1 / KF2 (kpUn1.pt, kpUn2.pt: :4682-4702) */
    const double *w1,  *w2;    /* [n_pairs] invSigma2 of the keypoints' octaves (information = w * I2, :4692-4710) */
    double K1[4], K2[4];    /* fx fy cx cy of each keyframe (:4612-4619; they may differ) */
    double th2;             /* chi2 gate of both tests (10 at the reference's call site, src/LoopClosing.cpp:399) */
    double huber;           /* Huber width of every edge: (double)(float)sqrt((float)th2), :4634 */
    int32_t its_stage1, its_stage2_bad, its_stage2_clean;  /* 5, 10, 5 (:4724, :4749-4752); each at least 1 */
    int32_t min_inliers;    /* 10 (:4755) */
} vba_sim3_problem;

typedef struct vba_sim3_result {
    int32_t n_inliers;      /* the function's return value (0 when n_pairs - n_bad_stage1 < min_inliers) */
    int32_t status;         /* VBA_OK */
    int32_t n_bad_stage1;   /* nBad of the first test: tells which stage-2 budget was used */
    int32_t its_done[2];    /* LM iterations of the two optimize() calls (0 for a stage that did not run) */
    double  chi2_stage[2];  /* robust chi2 of the accepted estimate at the end of each optimize() (LM's currentChi) */
    uint8_t *outlier;       /* [n_pairs] caller-allocated: 1 = the host nulls vpMatches1[idx] (:4738-4739, :4773-4774); set for the
                             * pairs of the first test also when 0 is returned */
    double  *chi2_12, *chi2_21; /* [n_pairs] caller-allocated or NULL: e12->chi2(), e21->chi2() as the last test of each pair read them */
} vba_sim3_result;

/* Synchronous, like vba_pose_optimize; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0.  A bad problem
 * (negative n_pairs, NULL array with n_pairs > 0, non-finite S12, scale <= 0, zero quaternion, a budget below 1) fails the whole
 * call before any GPU work, message through vba_last_error.  No upper bound on n_pairs. */
int vba_sim3_optimize(void *handle, int32_t n_problems, vba_sim3_problem *const *inout, vba_sim3_result *const *out);

/* ---- loop-candidate Sim3 RANSAC ----
 * Sim3Solver::iterate (src/Sim3Solver.cpp:138-220), ComputeSim3 (:253-359: Horn's closed form on three pairs) and CheckInliers
 * (:363-388: the two-sided reprojection test of every pair), the first of the three solver stages of LoopClosing::ComputeSim3
 * (src/LoopClosing.cpp:329-426); its hit is the S12 that vba_sim3_optimize takes.  One call runs n_hyp hypotheses of every
 * candidate of a batch (one workgroup per candidate, one kernel launch per call) and applies iterate's accept rule in hypothesis
 * order.  With c[h] the inlier count of hypothesis h and b = best_inliers: for h = 0 .. n_hyp-1, c[h] >= b makes b = c[h],
 * best_hyp = h, best_S12 = S12[h] (a later tie replaces the best, :193); if in addition c[h] > min_inliers (strict, :203), hit = h
 * and the scan stops.  best_inliers is written back as b.  The library has no random numbers: the caller draws the triples (the
 * reference draws with rand(), and its removal step (:182) lets a triple hold a pair twice, so duplicates are legal here).  A
 * degenerate triple gives whatever Horn's formulas give; a NaN estimate counts 0 inliers, as in the reference.  FP64 throughout;
 * the reference computes in CV_32F (gives the measured difference). */
typedef struct vba_sim3_ransac_problem {
    int32_t n_pairs;          /* N: pairs that passed the constructor's filters (:49-95) */
    int32_t fix_scale;        /* mbFixScale */
    const double *p1c, *p2c;  /* [n_pairs][3] mvX3Dc1, mvX3Dc2 (camera frames of KF1 / KF2) */
    const double *max_err1, *max_err2; /* [n_pairs] 9.210 * sigma2 of the keypoints' octaves (:78-79) */
    double K1[4], K2[4];      /* fx fy cx cy; the kernel forms mvP1im1 / mvP2im2 itself (:441-460) */
    int32_t min_inliers;      /* mRansacMinInliers (20 at the call site) */
    int32_t n_hyp;            /* hypotheses of THIS call (iterate's nIterations, or the whole budget) */
    const int32_t *sample;    /* [n_hyp][3] pair indices of every hypothesis, drawn by the caller */
    int32_t best_inliers;     /* in/out: mnBestInliers, 0 for a fresh solver */
    double  best_S12[8];      /* in/out: mBestRotation / Translation / Scale as t(3) q(4, xyzw) s */
} vba_sim3_ransac_problem;

typedef struct vba_sim3_ransac_result {
    int32_t status;           /* VBA_OK */
    int32_t hit;              /* hypothesis at which iterate() returns (:203-211), -1: none */
    int32_t its_done;         /* hypotheses consumed: hit + 1, or n_hyp */
    int32_t best_hyp;         /* last hypothesis of this call that became the best, -1: none */
    int32_t n_inliers;        /* mnInliersi of the hit, 0 without one */
    double  S12[8];           /* the hit's T12, vba_sim3_problem.S12 layout; untouched without a hit */
    uint8_t *inlier;          /* [n_pairs] caller-allocated: mvbInliersi of the hit; untouched without one */
    int32_t *hyp_inliers;     /* [n_hyp] caller-allocated or NULL: inlier count of EVERY hypothesis of the call */
} vba_sim3_ransac_result;

/* Synchronous, like vba_sim3_optimize; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; n_hyp == 0 is legal
 * (hit = -1, its_done = 0, state untouched); n_pairs < min_inliers is legal and not short-circuited (the iteration budget and
 * bNoMore belong to the caller).  A bad problem fails the whole call before any GPU work, message through vba_last_error naming
 * the problem: NULL problem or result, a negative n_pairs / n_hyp / min_inliers / best_inliers, a NULL array with a non-zero count
 * (inlier is required when n_pairs > 0), n_pairs < 3 with n_hyp > 0, a sample index outside [0, n_pairs), a non-finite K, point
 * or gate.  The quaternion of S12 / best_S12 is the unit eigenvector of Horn's N with w >= 0. */
int vba_sim3_ransac(void *handle, int32_t n_problems, vba_sim3_ransac_problem *const *inout,
                    vba_sim3_ransac_result *const *out);

/* ---- two-view triangulation of new map points ----
 * The geometric part of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1334-1517), monocular: for every match of a
 * keyframe pair (keyframe 1 = mpCurrentKeyFrame, keyframe 2 = one neighbour) the two rays and the parallax gate (:1360-1389), the
 * linear triangulation (:1393-1408: the right singular vector of the smallest singular value of the 4x4 A, divided by its last
 * entry), the two depth tests (:1428-1433), the two chi-square reprojection tests (:1437-1480) and the scale-consistency test
 * (:1499-1517).  One problem is one keyframe pair with all its matches; one call takes any number of pairs, ragged, in one kernel
 * launch (one lane per match).  The tests are applied in the reference's order with its comparison operators, and `reason` says
 * which `continue` dropped a match:
 *   0  accepted (:1520)
 *   1  parallax gate: not (cos > 0 && cos < cos_max); a NaN cosine lands here (:1389, :1423)
 *   2  homogeneous coordinate == 0 (:1404)
 *   3  z1 <= 0 (:1429)
 *   4  z2 <= 0 (:1433)
 *   5  squared reprojection error in keyframe 1 > chi2_th * sigma2 of the keypoint's octave (:1450)
 *   6  the same in keyframe 2 (:1479)
 *   7  dist1 == 0 || dist2 == 0 (:1505)
 *   8  ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor (:1516)
 * x3d holds the triangulated point for reason 0 and for 3 .. 8 (the point that failed), zeros for 1 and 2.  Past the input
 * validation NaN compares as IEEE says, as in the reference.  MONOCULAR ONLY, as everywhere in this backend: the stereo branches
 * (:1374-1377, :1411-1419, :1455-1465, :1484-1494) do not exist here.  FP64 throughout; the reference computes in CV_32F
 * (gives the measured difference).  The singular vector comes from A itself (one-sided Jacobi), not
 * from A^T A. */
typedef struct vba_triangulate_problem {
    double Rcw1[9], tcw1[3];  /* GetRotation() (row-major) / GetTranslation() of mpCurrentKeyFrame (:1254-1256), float32 widened */
    double Ow1[3];            /* GetCameraCenter() as the keyframe holds it (:1262), not recomputed */
    double K1[4];             /* fx fy cx cy (:1265-1268); invfx = 1 / fx is formed in FP64 */
    double Rcw2[9], tcw2[3];  /* the neighbour pKF2 (:1320-1322) */
    double Ow2[3];            /* :1287 */
    double K2[4];             /* :1327-1330 */
    int32_t n_levels1, n_levels2;             /* 1 .. 64: entries of the level tables */
    const double *level_sigma2_1, *scale_1;   /* [n_levels1] mvLevelSigma2 (:1437), mvScaleFactors (:1513) of keyframe 1 */
    const double *level_sigma2_2, *scale_2;   /* [n_levels2] of keyframe 2 (:1468, :1513) */
    double ratio_factor;      /* 1.5f * mfScaleFactor (:1272) */
    double cos_max;           /* 0.9998 (:1389) */
    double chi2_th;           /* 5.991 (:1450, :1479) */
    int32_t n_matches;        /* vMatchedIndices.size() (:1335) */
    const double *uv1, *uv2;  /* [n_matches][2] mvKeysUn[idx].pt of the match in keyframe 1 / 2 (:1347, :1353) */
    const uint8_t *oct1, *oct2; /* [n_matches] kp.octave (:1437, :1468, :1513) */
} vba_triangulate_problem;

typedef struct vba_triangulate_result {
    int32_t status;           /* VBA_OK */
    int32_t n_accepted;       /* matches with reason 0 (nnew of the pair, :1542), counted on the host from the reasons */
    double *x3d;              /* [n_matches][3] caller-allocated: x3D (:1408) */
    uint8_t *reason;          /* [n_matches] caller-allocated: the codes above */
} vba_triangulate_result;

/* Synchronous, like vba_sim3_ransac; -1 while asynchronous tickets are pending.  n_pairs == 0 returns 0; n_matches == 0 is legal
 * (n_accepted = 0, nothing else written).  A bad pair fails the whole call before any GPU work with "vba_triangulate: pair K:
 * <why>" through vba_last_error: a NULL problem or result, a negative count, a NULL array with a non-zero count (x3d and reason
 * are required when n_matches > 0), n_levels outside 1 .. 64, an octave >= n_levels, a non-finite pose, K, level table, threshold
 * or pixel, a zero fx / fy, a level scale <= 0.  A match's outputs do not depend on where its pair stands in the batch. */
int vba_triangulate(void *handle, int32_t n_pairs, vba_triangulate_problem *const *in, vba_triangulate_result *const *out);

/* ---- monocular two-view initialisation ----
 * Initializer::Initialize (src/Initializer.cpp:36-130) for a batch of frame pairs (frame 1 = reference, frame 2 = current): the
 * normalisation of both frames' keypoints (:893-946, once per frame), for every 8-set the caller drew ComputeH21 (:263-305) and
 * ComputeF21 (:320-356), CheckHomography (:362-461) and CheckFundamental (:465-545) over all matches, the scans (:179, :233), the
 * model choice (:120-126), ReconstructH (:673-835) or ReconstructF (:555-667) with CheckRT (:950-1082) and Triangulate (:859-880).
 * One problem is one frame pair; one call takes any number of pairs, ragged, in one kernel launch (one 256-lane workgroup per
 * pair).  The library has no RNG: the caller draws the sets (mvSets, :78-101), as in vba_sim3_ransac.  FP64 on float32 inputs
 * widened; the reference computes in CV_32F.  The chi-square gates are the reference's float
 * variables widened: (double)5.991f in H, (double)3.841f (gate) and (double)5.991f (score) in F.
 *   reason  0  success
 *           1  the chosen model has no hypothesis with a score above 0 (the reference would read an empty cv::Mat)
 *           2  d1 / d2 < 1.00001 || d2 / d3 < 1.00001 (:699)
 *           3  the rule of :822 failed (ReconstructH)
 *           4  maxGood < nMinGood || nsimilar > 1 (:613)
 *           5  the parallax of the hypothesis with maxGood is not > min_parallax (:619-663)
 * The scans run in hypothesis order with a strict > against a score that starts at 0.0: a tie keeps the earlier hypothesis, and a
 * hypothesis whose score is NaN (a singular H21, whose inverse is not finite here) never becomes the best.  RH = SH / (SH + SF);
 * the H path is taken when RH > 0.40, a NaN goes to F.
 * Sign convention of the 3x3 SVDs: singular values descending; (u_i, v_i) are flipped together so that the
 * largest-magnitude component of u_i (the first among equals) is positive; in DecomposeE, where the third singular value is zero,
 * u_3 = u_1 x u_2 and v_3 = v_1 x v_2.  rt_good[] / rt_parallax[] are listed in the reference's order under this convention: F:
 * (R1,t) (R2,t) (R1,-t) (R2,-t); H: the eight Faugeras hypotheses of :718-790.  ok, reason, R21, t21, x3d and triangulated do not
 * depend on the convention. */
typedef struct vba_two_view_problem {
    int32_t n_keys1, n_keys2; /* mvKeys1.size(), mvKeys2.size() (:33, :42) */
    const double *uv1;        /* [n_keys1][2] mvKeysUn[i].pt of ALL keypoints of frame 1: Normalize averages over all (:893-946) */
    const double *uv2;        /* [n_keys2][2] the same of frame 2 */
    int32_t n_matches;        /* mvMatches12.size() (:65) */
    int32_t n_hyp;            /* mMaxIterations (200, :78) */
    const int32_t *match;     /* [n_matches][2] mvMatches12 (:51-62): index in frame 1, index in frame 2; the first indices are distinct */
    const int32_t *sets;      /* [n_hyp][8] mvSets (:78-101): match indices of every hypothesis */
    double K[4];              /* fx fy cx cy (mK, :30) */
    double sigma;             /* mSigma (1.0, :32) */
    double min_parallax;      /* minParallax in degrees (1.0, :124) */
    int32_t min_triangulated; /* minTriangulated (50, :124) */
    int32_t pad;
} vba_two_view_problem;

typedef struct vba_two_view_result {
    int32_t status;           /* VBA_OK */
    int32_t ok;               /* the return value of Initialize */
    int32_t model;            /* 1 = H (RH > 0.40), 2 = F */
    int32_t reason;           /* the codes above */
    int32_t best_hyp_h, best_hyp_f;    /* the hypotheses the scans kept (-1: none) */
    int32_t n_inliers_h, n_inliers_f;  /* set flags of vbMatchesInliersH / F (0 without a best hypothesis) */
    int32_t n_rt;             /* (R, t) hypotheses CheckRT ran on: 0 (reasons 1, 2), 4 (F) or 8 (H) */
    int32_t best_rt;          /* the winner among them when ok, otherwise -1 */
    int32_t rt_good[8];       /* nGood of every hypothesis (:1075) */
    double score_h, score_f;  /* SH, SF (:105) */
    double rh;                /* RH (:120) */
    double H21[9], F21[9];    /* of the two best hypotheses, row-major, denormalised as in :172 and :228 (zeros without one) */
    double rt_parallax[8];    /* parallax of every hypothesis in degrees (:1067-1079) */
    double R21[9], t21[3];    /* written when ok */
    uint8_t *inlier_h, *inlier_f; /* [n_matches] caller-allocated, required: vbMatchesInliersH / F (zeros without a best hypothesis) */
    double *x3d;              /* [n_keys1][3] caller-allocated, required: vP3D, written when ok (zeros where no point was accepted) */
    uint8_t *triangulated;    /* [n_keys1] caller-allocated, required: vbTriangulated, written when ok (1 only where cosParallax < 0.99998) */
    double *hyp_score_h, *hyp_score_f; /* [n_hyp] caller-allocated or NULL: currentScore of every hypothesis */
} vba_two_view_result;

/* Synchronous, like vba_triangulate; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; n_hyp == 0 is legal
 * (best_hyp_* = -1, ok = 0, reason = 1).  On failure (ok = 0) R21, t21, x3d and triangulated are left untouched.  A bad problem
 * fails the whole call before any GPU work with "vba_two_view_init: pair K: <why>" through vba_last_error: a NULL problem or
 * result, a negative count, a NULL array with a non-zero count (inlier_h / inlier_f are required when n_matches > 0, x3d and
 * triangulated when n_keys1 > 0), n_matches < 8 with n_hyp > 0, a set index outside [0, n_matches), a match index outside its
 * frame, a repeated first index, a non-finite pixel, K, sigma or min_parallax, a zero fx / fy / sigma.  A pair's outputs do not
 * depend on where it stands in the batch. */
int vba_two_view_init(void *handle, int32_t n_problems, vba_two_view_problem *const *in, vba_two_view_result *const *out);

/* ---- matching for triangulation ----
 * ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955) with CheckDistEpipolarLine (:167-192) and ComputeThreeMaxima
 * (:1800-1841), monocular (bOnlyStereo == false, no mvuRight): the matcher call in front of every vba_triangulate call of
 * LocalMapping::CreateNewMapPoints.  One problem is one keyframe pair; one call takes any number of pairs, ragged, in one kernel
 * launch (one 256-lane workgroup per pair).  The reference is restated as it stands:
 *   node join   the two feature vectors are walked as the `while` of :801-921 does; a keypoint of keyframe 1 is compared with the
 *               keypoints of keyframe 2 that its vocabulary node lists, in the order the node lists them
 *   query       bestDist = th_low, bestIdx2 = -1 (:833-834); a candidate is skipped when it has a map point (:848), when
 *               dist > th_low || dist > bestDist (:863: an EQUAL distance replaces the best, so the last one in list order wins among
 *               equals), when (ex - u2)^2 + (ey - v2)^2 < epipole_r2 * scale_2[octave] (:871-875), when den == 0 or not
 *               num^2 / den < chi2_epi * level_sigma2_2[octave] (:184-191); otherwise it becomes the best (:881-882)
 *   vbMatched2  is declared at :782 and read at :848 but never set: nothing marks a keypoint of keyframe 2 as taken, the queries are
 *               independent of each other and two of them may return the same idx2.  That is kept
 *   orientation rot = angle1 - angle2; if (rot < 0) rot += 360.0f; bin = round(rot * (1.0f / 30)) in float32 with C round (:898-905,
 *               bit for bit the reference's bin; only bins 0 .. 12 can occur and that is kept), ComputeThreeMaxima with its strict >
 *               and its 0.1f * (float)max1 rules, every match of another bin back to -1 (:931-940)
 * `state` says where a keypoint of keyframe 1 left the function, numbered in the order of the reference's exits:
 *   0  matched (:893) and kept by the orientation filter
 *   1  it has a map point (:817); this wins over 2
 *   2  no node that both keyframes list holds it (the walk of :801-921 never reaches it)
 *   3  no candidate passed (:890 fails)
 *   4  matched, then dropped by the orientation filter (:937)
 * Everything but the bin is FP64 on the float32 inputs widened; the reference computes in float32 (DESIGN.md section 8, row f-10,
 * gives the measured difference). */
typedef struct vba_search_tri_problem {
    int32_t n_keys1, n_keys2;        /* pKF->N */
    const uint8_t *desc1, *desc2;    /* [n_keys][32] the rows of mDescriptors (:831, :858) */
    const uint8_t *has_mp1, *has_mp2; /* [n_keys] GetMapPoint(idx) != NULL (:813, :843) */
    int32_t n_nodes1, n_nodes2;      /* entries of mFeatVec (:763-764) */
    const uint32_t *node_id1, *node_id2;      /* [n_nodes] strictly ascending: the order of the std::map */
    const int32_t *node_begin1, *node_begin2; /* [n_nodes + 1] node k lists node_feat[node_begin[k] .. node_begin[k + 1]) */
    const int32_t *node_feat1, *node_feat2;   /* keypoint indices in the order the node's vector holds them; each keypoint at most once */
    const double *uv1, *uv2;         /* [n_keys][2] mvKeysUn[idx].pt (:828, :867) */
    const float *angle1, *angle2;    /* [n_keys] mvKeysUn[idx].angle in [0, 360) (:898); read only with check_orientation */
    const uint8_t *oct2;             /* [n_keys2] mvKeysUn[idx].octave (:874, :191) */
    int32_t n_levels2;               /* 1 .. 64 */
    const double *level_sigma2_2, *scale_2;   /* [n_levels2] mvLevelSigma2 (:191), mvScaleFactors (:874) of keyframe 2 */
    double F12[9];                   /* row-major: the caller's ComputeF12 (src/LocalMapping.cpp:1659-1680), float32 widened */
    double epipole[2];               /* ex, ey of :768-775 */
    int32_t th_low;                  /* TH_LOW = 50 (:833, :863); 0 .. 255 */
    int32_t check_orientation;       /* mbCheckOrientation (:896, :923) */
    double chi2_epi;                 /* 3.84 (:191) */
    double epipole_r2;               /* 100 (:874) */
} vba_search_tri_problem;

typedef struct vba_search_tri_result {
    int32_t status;           /* VBA_OK */
    int32_t n_matches;        /* the return value (:954) */
    int32_t n_before_filter;  /* nmatches in front of :923 */
    int32_t hist[30];         /* rotHist[i].size() in front of the filter (zeros without check_orientation) */
    int32_t ind[3];           /* ind1 .. ind3 of ComputeThreeMaxima, -1 as the reference leaves them (and without check_orientation) */
    int32_t *match12;         /* [n_keys1] caller-allocated: vMatches12 behind the filter (:783, :937) */
    uint8_t *best_dist;       /* [n_keys1] caller-allocated: bestDist of a keypoint in state 0 or 4, 255 otherwise */
    uint8_t *state;           /* [n_keys1] caller-allocated: the codes above */
    int32_t *pairs;           /* [n_keys1][2] caller-allocated: vMatchedPairs (:947-952), ascending idx1; the first n_matches rows are
                                 written (on the host, from match12) */
} vba_search_tri_result;

/* Synchronous, like vba_triangulate; -1 while asynchronous tickets are pending.  n_pairs == 0 returns 0; a pair without keypoints
 * or without a shared node is legal (n_matches = 0, every state 1 or 2).  A bad pair fails the whole call before any GPU work with
 * "vba_search_triangulation: pair K: <why>" through vba_last_error: a NULL problem or result, a negative count, a NULL array with a
 * non-zero count (match12, best_dist, state and pairs are required when n_keys1 > 0), n_levels2 outside 1 .. 64, th_low outside
 * 0 .. 255, an octave >= n_levels2, a non-finite pixel, F12, epipole, threshold or level table, node ids that are not strictly
 * ascending, a node_begin that does not start at 0 or decreases, a keypoint index outside its keyframe or listed twice in one
 * feature vector, and with check_orientation an angle outside [0, 360).  A pair's outputs do not depend on where it stands in the
 * batch. */
int vba_search_triangulation(void *handle, int32_t n_pairs, vba_search_tri_problem *const *in, vba_search_tri_result *const *out);

/* ---- projection search for map-point fusion ----
 * The search half of both ORBmatcher::Fuse overloads (src/ORBmatcher.cpp:958-1119 and :1123-1254) with KeyFrame::GetFeaturesInArea
 * (src/KeyFrame.cpp:1071-1115), IsInImage (:1119-1122) and MapPoint::PredictScale (src/MapPoint.cpp:529-540), monocular (mvuRight < 0,
 * the `else` branch at :1070): the calls LocalMapping::SearchInNeighbors and LoopClosing::SearchAndFuse are made of.  One problem is
 * one keyframe and one list of map points; one call takes any number of problems, ragged, in one kernel launch (256 points per
 * workgroup).  A point's search reads the point and the keyframe's static data only, never the associations the function mutates, so
 * the points are independent; the mutation (:1095-1115, :1234-1250) stays with the caller.  The reference is restated as it stands:
 *   gates       p3Dc = Rcw p + tcw; z < 0 leaves (:991).  z == 0 passes: invz is infinite, u and v are infinite or NaN and the point
 *               leaves at IsInImage, written as the positive conjunction u >= minX && u < maxX && v >= minY && v < maxY (:1004).
 *               dist3D = |p - Ow| outside [dist_min, dist_max] (:1016), PO . Pn < cos_view * dist3D (:1023),
 *               nPredictedLevel = ceil(log(pred_max / dist3D) / log_scale_factor) outside 0 .. n_levels - 1 (:1027)
 *   area        GetFeaturesInArea(u, v, th * scale[level]) literally: floor for the first cell and CEIL for the last one, the four
 *               early returns, the clamps to the grid, fabs(dx) < r && fabs(dy) < r.  Candidates come in cell order (ix outer, iy
 *               inner) and inside a cell in list order
 *   candidate   skipped when kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel (:1052) and, with check_reproj, when
 *               (ex^2 + ey^2) * inv_level_sigma2[kpLevel] > chi2_reproj (:1072-1080); dist < bestDist is strict (:1087), so among equal
 *               distances the first in walk order wins
 * One deviation: the Sim3 overload has no range check in front of mvScaleFactors[nPredictedLevel] (:1196-1200) and PredictScale
 * does not clamp, so with dist3D in [0.8 min, 1.2 max] the reference can read outside the vector.  vba_fuse applies the check of
 * :1027 in both modes (state 6).
 * `state` says where a point left the function, numbered in the order of the reference's exits:
 *   0  bestDist <= th_low (:1095): the caller applies :1097-1114 or :1236-1249
 *   1  skipped by the caller's `skip`
 *   2  z < 0 (:991)
 *   3  not in the image (:1004)
 *   4  dist3D outside [dist_min, dist_max] (:1016)
 *   5  viewing angle (:1023)
 *   6  predicted level outside 0 .. n_levels - 1 (:1027)
 *   7  no keypoint in the area (:1034)
 *   8  keypoints in the area but bestDist > th_low; best_idx and best_dist are what the loop left (-1 and 256 when every candidate
 *      failed the level or reprojection test)
 * All floating point is FP64 on the float32 inputs widened; the reference computes in float32 (gives
 * the measured difference). */
typedef struct vba_fuse_problem {
    double Rcw[9], tcw[3], Ow[3];    /* row-major GetRotation(), GetTranslation(), GetCameraCenter(); for the Sim3 overload the caller
                                        decomposes Scw as :1134-1138 does */
    double K[4];                     /* fx fy cx cy */
    double bounds[4];                /* mnMinX mnMaxX mnMinY mnMaxY */
    int32_t n_keys;                  /* pKF->N */
    int32_t n_levels;                /* mnScaleLevels, 1 .. 64 */
    const uint8_t *desc;             /* [n_keys][32] mDescriptors */
    const double *uv;                /* [n_keys][2] mvKeysUn[idx].pt */
    const uint8_t *oct;              /* [n_keys] mvKeysUn[idx].octave */
    const double *scale;             /* [n_levels] mvScaleFactors (:1031) */
    const double *inv_level_sigma2;  /* [n_levels] mvInvLevelSigma2 (:1079) */
    double log_scale_factor;         /* mfLogScaleFactor */
    int32_t grid_cols, grid_rows;    /* mnGridCols, mnGridRows (64 x 48); >= 1, cols * rows <= 65536 */
    double grid_inv_w, grid_inv_h;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t *cell_begin;       /* [cols * rows + 1] cell (ix, iy) at ix * rows + iy lists cell_feat[cell_begin[c] .. cell_begin[c + 1]) */
    const int32_t *cell_feat;        /* keypoint indices in the order mGrid[ix][iy] holds them; each keypoint at most once */
    int32_t n_pt;                    /* vpMapPoints.size() */
    int32_t th_low;                  /* TH_LOW = 50 (:1095); 0 .. 256 */
    const double *pos, *normal;      /* [n_pt][3] GetWorldPos(), GetNormal() */
    const double *dist_min, *dist_max; /* [n_pt] GetMinDistanceInvariance(), GetMaxDistanceInvariance() as the reference returns them */
    const double *pred_max;          /* [n_pt] mfMaxDistance, which PredictScale reads */
    const uint8_t *pt_desc;          /* [n_pt][32] GetDescriptor() */
    const uint8_t *skip;             /* [n_pt] non-zero: the caller's test of :980-984 or :1154 (NULL, bad, already in the keyframe) */
    double th;                       /* the radius factor: 3.0 for :958, the caller's value for :1123 */
    double cos_view;                 /* 0.5 (:1023) */
    int32_t check_reproj;            /* the gate of :1072-1080 exists in the first overload only: the Sim3 caller passes 0 */
    double chi2_reproj;              /* 5.99 (:1079) */
} vba_fuse_problem;

typedef struct vba_fuse_result {
    int32_t status;           /* VBA_OK */
    int32_t n_found;          /* points in state 0 (summed on the host) */
    int32_t *best_idx;        /* [n_pt] caller-allocated: bestIdx; -1 unless state 0 or 8 */
    uint16_t *best_dist;      /* [n_pt] caller-allocated: bestDist; 256 when no candidate passed */
    int8_t *level;            /* [n_pt] caller-allocated: nPredictedLevel for the states 0, 7 and 8, the out-of-range value itself clamped
                                 to int8 for state 6, -128 otherwise */
    double *uv;               /* [n_pt][2] caller-allocated: the projection for the states 0 and 3 .. 8, NaN otherwise */
    uint8_t *state;           /* [n_pt] caller-allocated: the codes above */
} vba_fuse_result;

/* Synchronous, like vba_search_triangulation; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; a problem with
 * n_pt == 0 or n_keys == 0 is legal.  A bad problem fails the whole call before any GPU work with "vba_fuse: problem K: <why>"
 * through vba_last_error: a NULL problem or result, a negative count, a NULL array with a non-zero count (the result arrays are
 * required when n_pt > 0), n_levels outside 1 .. 64, an octave >= n_levels, th_low outside 0 .. 256, grid sizes outside their range,
 * a cell_begin that does not start at 0, decreases or ends above n_keys, a cell_feat entry out of range or listed twice, any
 * non-finite pose, intrinsic, bound, pixel, level table, position, normal, distance or threshold.  A problem's outputs do not depend
 * on where it stands in the batch. */
int vba_fuse(void *handle, int32_t n_problems, vba_fuse_problem *const *in, vba_fuse_result *const *out);

/* ---- Sim3 projection matching for loop candidates ----
 * ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cpp:1258-1496) with
 * KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:1071-1115), IsInImage (:1119-1122) and MapPoint::PredictScale
 * (src/MapPoint.cpp:529-540), monocular: the call LoopClosing::ComputeSim3 makes between Sim3Solver::iterate (vba_sim3_ransac) and
 * Optimizer::OptimizeSim3 (vba_sim3_optimize) (src/LoopClosing.cpp:390).  One problem is one keyframe pair with its Sim3; one call
 * takes any number of pairs, ragged, in one kernel launch (256 queries per workgroup).  Both projection searches (:1310-1392 and
 * :1398-1475) read static data only, so every keypoint that has a usable map point and no prior match is an independent query; the
 * agreement loop (:1480-1493) runs on the host in the write-back.  The reference is restated as it stands, direction 1 (keyframe 1
 * into keyframe 2) with the line numbers below, direction 2 alike with the sides exchanged:
 *   transform   p3Dc1 = R1w p + t1w, p3Dc2 = sR21 p3Dc1 + t21 (:1321-1322), with sR12 = s12 R12, sR21 = (1 / s12) R12^T and
 *               t21 = -sR21 t12 formed once per pair on the host in the order :1277-1279 write them
 *   gates       z < 0 leaves (:1325); z == 0 passes, u and v are infinite or NaN and the point leaves at IsInImage of the TARGET
 *               keyframe, written as the positive conjunction u >= minX && u < maxX && v >= minY && v < maxY (:1337).  The
 *               projection uses K of pKF1 in BOTH directions, as the reference does (:1262-1265, :1333, :1420).
 *               dist3D = |p3Dc2| outside [dist_min, dist_max] (:1345),
 *               nPredictedLevel = ceil(log(pred_max / dist3D) / log_scale_factor of the target) outside 0 .. n_levels - 1 of the target
 *   area        GetFeaturesInArea(u, v, th * scale[level]) of the target literally: floor for the first cell and CEIL for the last
 *               one, the four early returns, the clamps to the grid, fabs(dx) < r && fabs(dy) < r.  Candidates come in cell order
 *               (ix outer, iy inner) and inside a cell in list order
 *   candidate   skipped when kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel (:1374), nothing else: there is no
 *               viewing-angle gate and no reprojection gate here.  dist < bestDist is strict (:1381), so among equal distances the
 *               first in walk order wins.  Target keypoints are never filtered by has_pt or matched
 * One deviation: the reference reads mvScaleFactors[nPredictedLevel] unchecked (:1354, :1439) and PredictScale does not clamp, so it
 * can read outside the vector.  vba_search_by_sim3 leaves with state 6 instead, as vba_fuse does.
 * `state` says where a keypoint left its loop, numbered in the order of the reference's exits, the same in both directions:
 *   0  bestDist <= th_high (:1388): match holds bestIdx
 *   1  no usable point (has_pt == 0: !pMP or pMP->isBad(), :1314-1318)
 *   2  already matched (:1314)
 *   3  z < 0 (:1325)
 *   4  not in the image of the target keyframe (:1337)
 *   5  dist3D outside [dist_min, dist_max] (:1345)
 *   6  predicted level outside 0 .. n_levels - 1 of the target (the deviation)
 *   7  no keypoint in the area (:1359)
 *   8  keypoints in the area but none at or under th_high; best_dist is what the loop left (256 when every candidate failed the
 *      level test)
 * All floating point is FP64 on the float32 inputs widened; the reference computes in float32 (gives
 * the measured difference).  No floating-point value is returned. */
typedef struct vba_search_sim3_kf {
    double Rcw[9], tcw[3];           /* row-major GetRotation(), GetTranslation() */
    double bounds[4];                /* mnMinX mnMaxX mnMinY mnMaxY */
    int32_t n_keys;                  /* N = GetMapPointMatches().size() */
    int32_t n_levels;                /* mnScaleLevels, 1 .. 64 */
    const uint8_t *desc;             /* [n_keys][32] mDescriptors */
    const double *uv;                /* [n_keys][2] mvKeysUn[idx].pt */
    const uint8_t *oct;              /* [n_keys] mvKeysUn[idx].octave */
    const double *scale;             /* [n_levels] mvScaleFactors (:1354) */
    double log_scale_factor;         /* mfLogScaleFactor */
    int32_t grid_cols, grid_rows;    /* mnGridCols, mnGridRows; >= 1, cols * rows <= 65536 */
    double grid_inv_w, grid_inv_h;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t *cell_begin;       /* [cols * rows + 1] as in vba_fuse_problem */
    const int32_t *cell_feat;        /* keypoint indices in the order mGrid[ix][iy] holds them; each keypoint at most once */
    /* the keyframe's own map points, GetMapPointMatches(), per keypoint */
    const uint8_t *has_pt;           /* [n_keys] non-zero: pMP && !pMP->isBad() */
    const uint8_t *matched;          /* [n_keys] non-zero: vbAlreadyMatched1 (kf1) / vbAlreadyMatched2 (kf2), built as :1291-1301 do,
                                        GetIndexInKeyFrame included */
    const double *pos;               /* [n_keys][3] GetWorldPos(); read only where has_pt */
    const double *dist_min, *dist_max; /* [n_keys] GetMinDistanceInvariance(), GetMaxDistanceInvariance(); read only where has_pt */
    const double *pred_max;          /* [n_keys] mfMaxDistance, which PredictScale reads; read only where has_pt */
    const uint8_t *pt_desc;          /* [n_keys][32] GetDescriptor(); read only where has_pt */
} vba_search_sim3_kf;

typedef struct vba_search_sim3_problem {
    vba_search_sim3_kf kf1, kf2;
    double K[4];                     /* fx fy cx cy of pKF1, used in both directions */
    double s12, R12[9], t12[3];      /* the Sim3: s12 finite and positive, R12 row-major */
    double th;                       /* the radius factor, 7.5 at the call site */
    int32_t th_high;                 /* TH_HIGH = 100 (:1388); 0 .. 256 */
} vba_search_sim3_problem;

typedef struct vba_search_sim3_result {
    int32_t status;           /* VBA_OK */
    int32_t n_found;          /* nFound of :1478-1493 (counted on the host) */
    int32_t *match1;          /* [kf1.n_keys] caller-allocated: vnMatch1, a keypoint of keyframe 2 or -1 */
    int32_t *match2;          /* [kf2.n_keys] caller-allocated: vnMatch2, a keypoint of keyframe 1 or -1 */
    uint16_t *best_dist1;     /* [kf1.n_keys] caller-allocated: bestDist; 256 where the loop left INT_MAX or was not reached */
    uint16_t *best_dist2;     /* [kf2.n_keys] */
    int8_t *level1;           /* [kf1.n_keys] caller-allocated: nPredictedLevel for the states 0, 7 and 8, the out-of-range value itself
                                 clamped to int8 for state 6, -128 otherwise */
    int8_t *level2;           /* [kf2.n_keys] */
    uint8_t *state1;          /* [kf1.n_keys] caller-allocated: the codes above */
    uint8_t *state2;          /* [kf2.n_keys] */
    int32_t *match12;         /* [kf1.n_keys] caller-allocated: the keypoint of keyframe 2 both directions agree on (:1480-1493) or -1; the
                                 caller does vpMatches12[i1] = vpMapPoints2[match12[i1]] */
} vba_search_sim3_result;

/* Synchronous, like vba_fuse; -1 while asynchronous tickets are pending.  n_pairs == 0 returns 0; n_keys == 0 on either side is
 * legal.  A bad pair fails the whole call before any GPU work, with nothing written, as "vba_search_by_sim3: pair K: <why>" through
 * vba_last_error: a NULL problem or result; for either side ("keyframe 1: ..." / "keyframe 2: ...") everything vba_fuse refuses for
 * its keyframe (a negative count, a NULL array with a non-zero count -- the result arrays of a side are required when its n_keys
 * > 0 --, n_levels outside 1 .. 64, an octave >= n_levels, grid sizes outside their range, a cell_begin that does not start at 0,
 * decreases or ends above n_keys, a cell_feat entry out of range or listed twice, a non-finite pose, bound, cell size, pixel or level
 * table) and a non-finite position or distance where has_pt is set; s12 not finite or not positive; a non-finite R12, t12, K or th;
 * th_high outside 0 .. 256.  A pair's outputs do not depend on where it stands in the batch. */
int vba_search_by_sim3(void *handle, int32_t n_pairs, vba_search_sim3_problem *const *in, vba_search_sim3_result *const *out);

/* ---- projection matching for tracking ----
 * The two matchers the tracking thread runs directly in front of its two PoseOptimization calls (vba_pose_optimize), monocular
 * (mvuRight < 0, bMono == true), selected by `mode`:
 *   VBA_SEARCH_PROJ_LAST_FRAME  ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cpp:1511-1665), the
 *                               call of Tracking::TrackWithMotionModel (src/Tracking.cpp:1735-1804)
 *   VBA_SEARCH_PROJ_LOCAL_MAP   Frame::isInFrustum (src/Frame.cpp:492-550) per point fused with ORBmatcher::SearchByProjection(F,
 *                               vpMapPoints, th) (src/ORBmatcher.cpp:63-156): Tracking::SearchLocalPoints (src/Tracking.cpp:2111-2174)
 * both over Frame::GetFeaturesInArea (src/Frame.cpp:562-620).  One problem is one frame and one ORDERED list of queries (the keypoints
 * of the last frame, or the local map points, in the reference's loop order); one call takes any number of problems, ragged, in one
 * kernel launch (one 256-lane workgroup per problem).  The queries of a problem are not independent: a query skips the keypoints
 * that hold a point with Observations() > 0, among them those an earlier query of the same call has claimed (:113-115, :1596-1598),
 * and then claims its own (:150, :1623).  The kernel resolves that with an order-preserving conflict pass whose result is the
 * sequential one: claim[k] is the smallest index of a blocking query (q_blocks) whose current result is keypoint k, query q treats k
 * as taken iff occupied[k] || claim[k] < q, and rounds of (every query walks against the table of the round before; the table is
 * rebuilt) run until a round changes nothing.  `rounds` counts them, the detecting round included; it is at most n_q + 1
 * (has the proof).  The reference is restated as it stands:
 *   last frame  x3Dc = Rcw p + tcw; invzc = 1 / z < 0 leaves (:1553); u = fx * xc * invzc + cx, v alike; u < minX || u > maxX ||
 *               v < minY || v > maxY leaves (:1559-1562); radius = th * scale[q_oct] (:1567); GetFeaturesInArea(u, v, radius,
 *               q_oct - 1, q_oct + 1) (:1580, neither bForward nor bBackward with bMono); a taken keypoint is skipped; dist < bestDist is
 *               strict (:1613); bestDist <= th_high matches (:1621); the bin of :1628-1633 in float32 with C round
 *   local map   Pc = Rcw p + tcw; PcZ < 0 leaves (:506); the same projection and bounds tests (:513-516); dist = |p - Ow| outside
 *               [q_dist_min, q_dist_max] (:525); viewCos = PO . Pn / dist < cos_view (:532); nPredictedLevel =
 *               ceil(log(q_pred_max / dist) / log_scale_factor) outside 0 .. n_levels - 1 (:537); r = RadiusByViewingCos(viewCos) (2.5
 *               when viewCos > 0.998, else 4.0), r *= th only when th != 1.0 (:67, :88); GetFeaturesInArea(u, v, r * scale[level],
 *               level - 1, level) (:93); best and second best as :129-141; bestDist <= th_high (:145) and then the ratio test
 *               bestLevel == bestLevel2 && bestDist > nn_ratio * bestDist2 with the product in float32 (:147)
 *   area        Frame::GetFeaturesInArea literally: floor for the first cell and CEIL for the last one, the four early returns, the
 *               clamps to the grid, bCheckLevels = minLevel > 0 || maxLevel >= 0, the level test INSIDE the cell loop (so an area
 *               that holds keypoints of other levels only is empty), fabs(dx) < r && fabs(dy) < r.  Candidates come in cell order
 *               (ix outer, iy inner) and inside a cell in list order
 * One deviation: the reference's bounds tests are written as u < min || u > max, which a NaN projection (z == 0 with xc == 0)
 * passes, to reach an int cast of NaN inside GetFeaturesInArea.  Here a non-finite u or v leaves with state 3.  (With th_high = 256 a
 * query whose candidates are all taken would index mvpMapPoints with -1 in the reference; here it leaves as bestDist > th_high does.)
 * `state` says where a query left, numbered in the order of the reference's exits.  Last-frame mode:
 *   0  matched and kept        1  skipped (q_skip)      2  invzc < 0 (:1553)      3  outside the image (:1559-1562)
 *   4  no keypoint in the area (:1582)      5  bestDist > th_high (:1621), every candidate taken included
 *   6  matched, then dropped by the orientation filter (:1651-1661)
 * Local-map mode:
 *   0  matched      1  skipped (q_skip)      2  PcZ < 0 (:506)      3  outside the image (:513-516)      4  distance (:525)
 *   5  viewCos < cos_view (:532)      6  level outside 0 .. n_levels - 1 (:537)      7  area empty (:96)
 *   8  bestDist > th_high (:145)      9  failed the ratio test (:147)
 * In local-map mode the states 0 and 7 .. 9 are exactly the points for which isInFrustum returned true (IncreaseVisible,
 * src/Tracking.cpp:2154).  Everything but the ratio test and the bin is FP64 on the float32 inputs widened; the reference computes in
 * float32 (gives the measured margins). */
#define VBA_SEARCH_PROJ_LAST_FRAME 0
#define VBA_SEARCH_PROJ_LOCAL_MAP 1
#define VBA_SEARCH_PROJ_MAX_KEYS 16384   /* the claim table of a frame lives in LDS */
typedef struct vba_search_proj_problem {
    int32_t mode;                    /* VBA_SEARCH_PROJ_LAST_FRAME or VBA_SEARCH_PROJ_LOCAL_MAP */
    int32_t check_orientation;       /* mbCheckOrientation (:1626, :1643); last-frame mode only */
    double Rcw[9], tcw[3];           /* row-major mTcw rotation and translation (:1521-1522) / mRcw, mtcw (Frame.cpp:500) */
    double Ow[3];                    /* mOw (Frame.cpp:523); local-map mode only */
    double K[4];                     /* fx fy cx cy */
    double bounds[4];                /* mnMinX mnMaxX mnMinY mnMaxY */
    int32_t n_keys;                  /* CurrentFrame.N; at most VBA_SEARCH_PROJ_MAX_KEYS */
    int32_t n_levels;                /* mnScaleLevels, 1 .. 64 */
    const uint8_t *desc;             /* [n_keys][32] mDescriptors */
    const double *uv;                /* [n_keys][2] mvKeysUn[idx].pt */
    const uint8_t *oct;              /* [n_keys] mvKeysUn[idx].octave */
    const float *angle;              /* [n_keys] mvKeysUn[idx].angle in [0, 360) (:1628); read with check_orientation only */
    const double *scale;             /* [n_levels] mvScaleFactors (:93, :1567) */
    double log_scale_factor;         /* mfLogScaleFactor (Frame.cpp:536); local-map mode only */
    int32_t grid_cols, grid_rows;    /* FRAME_GRID_COLS, FRAME_GRID_ROWS (64 x 48); >= 1, cols * rows <= 65536 */
    double grid_inv_w, grid_inv_h;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t *cell_begin;       /* [cols * rows + 1] as in vba_fuse_problem */
    const int32_t *cell_feat;        /* keypoint indices in the order mGrid[ix][iy] holds them; each keypoint at most once */
    const uint8_t *occupied;         /* [n_keys] non-zero: mvpMapPoints[idx] && mvpMapPoints[idx]->Observations() > 0 before the call */
    int32_t n_q;                     /* LastFrame.N / vpMapPoints.size(): the queries in the reference's loop order */
    int32_t th_high;                 /* TH_HIGH = 100 (:145, :1621); 0 .. 256 */
    const double *q_pos;             /* [n_q][3] GetWorldPos() */
    const uint8_t *q_desc;           /* [n_q][32] GetDescriptor() */
    const uint8_t *q_skip;           /* [n_q] non-zero: last-frame mode, no point or mvbOutlier (:1540-1542); local-map mode, the caller's
                                        tests of src/Tracking.cpp:2145-2148 (mnLastFrameSeen == mnId, isBad) */
    const uint8_t *q_blocks;         /* [n_q] non-zero: pMP->Observations() > 0, so the keypoint this query claims is taken for later ones */
    const uint8_t *q_oct;            /* [n_q] LastFrame.mvKeys[i].octave (:1564), < n_levels; last-frame mode only */
    const float *q_angle;            /* [n_q] LastFrame.mvKeysUn[i].angle in [0, 360) (:1628); last-frame mode with check_orientation only */
    const double *q_normal;          /* [n_q][3] GetNormal(); local-map mode only, as the next three */
    const double *q_dist_min, *q_dist_max; /* [n_q] GetMinDistanceInvariance(), GetMaxDistanceInvariance() as the reference returns them */
    const double *q_pred_max;        /* [n_q] mfMaxDistance, which PredictScale reads */
    double th;                       /* the radius factor: 15 and 30 at the retry (Tracking.cpp:1752-1766) / 1 or 5 (:2163-2169) */
    float nn_ratio;                  /* mfNNratio, 0.8f at Tracking.cpp:2162; local-map mode only */
    double cos_view;                 /* 0.5 (Tracking.cpp:2151); local-map mode only */
} vba_search_proj_problem;

typedef struct vba_search_proj_result {
    int32_t status;           /* VBA_OK */
    int32_t n_matches;        /* the return value of the function */
    int32_t n_before_filter;  /* nmatches in front of the orientation filter (:1643); n_matches without one */
    int32_t hist[30];         /* rotHist[i].size() in front of the filter (zeros without check_orientation) */
    int32_t ind[3];           /* ind1 .. ind3 of ComputeThreeMaxima, -1 as the reference leaves them (and without check_orientation) */
    int32_t rounds;           /* rounds of the conflict pass, 1 .. n_q + 1 */
    int32_t *best_idx;        /* [n_q] caller-allocated: bestIdx as the candidate loop left it, -1 without a candidate */
    uint16_t *best_dist;      /* [n_q] caller-allocated: bestDist; 256 = none */
    uint16_t *best_dist2;     /* [n_q] caller-allocated: bestDist2 (local-map mode; 256 in last-frame mode) */
    int8_t *level;            /* [n_q] caller-allocated: local-map mode, nPredictedLevel (mnTrackScaleLevel) for the states 0 and 7 .. 9, the
                                 out-of-range value itself clamped to int8 for state 6; -128 otherwise and in last-frame mode */
    double *view_cos;         /* [n_q] caller-allocated: local-map mode, mTrackViewCos for the states 0 and 5 .. 9; NaN otherwise */
    double *uv;               /* [n_q][2] caller-allocated: the projection (mTrackProjX / Y) for every state but 1 and 2, NaN there */
    uint8_t *bin;             /* [n_q] caller-allocated: the histogram bin of a match (states 0 and 6) with check_orientation; 255 = none */
    uint8_t *state;           /* [n_q] caller-allocated: the codes above */
    int32_t *key_match;       /* [n_keys] caller-allocated: what the function leaves in mvpMapPoints, as a query index: -1 untouched,
                                 -2 cleared by the orientation filter (:1657), else the last query that wrote the keypoint */
} vba_search_proj_result;

/* Synchronous, like vba_fuse; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; a problem with n_q == 0 or
 * n_keys == 0 is legal.  A bad problem fails the whole call before any GPU work, with nothing written, as
 * "vba_search_by_projection: problem K: <why>" through vba_last_error: a NULL problem or result, an unknown mode, a negative count,
 * n_keys above VBA_SEARCH_PROJ_MAX_KEYS, a NULL array with a non-zero count (the per-query result arrays are required when n_q > 0,
 * key_match when n_keys > 0; the arrays of the other mode may be NULL), n_levels outside 1 .. 64, an octave >= n_levels, th_high
 * outside 0 .. 256, grid sizes outside their range, a cell_begin that does not start at 0, decreases or ends above n_keys, a
 * cell_feat entry out of range or listed twice, with check_orientation an angle outside [0, 360), any non-finite pose, intrinsic,
 * bound, pixel, level table, position, normal, distance or threshold that the mode reads.  A problem's outputs do not depend on
 * where it stands in the batch. */
int vba_search_by_projection(void *handle, int32_t n_problems, vba_search_proj_problem *const *in, vba_search_proj_result *const *out);

/* ---- projection matching for loop closure and relocalisation ----
 * The two ORBmatcher::SearchByProjection overloads that project the map points of keyframes into one target, monocular, selected by
 * `mode`:
 *   VBA_SEARCH_PROJ_KF_LOOP   SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:354-475), the
 *                             last step of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:470) behind vba_sim3_optimize; the target is
 *                             the keyframe pKF, the queries are vpPoints in their order
 *   VBA_SEARCH_PROJ_KF_RELOC  SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (:1667-1797), called
 *                             twice per candidate by Tracking::Relocalization (src/Tracking.cpp:2513, :2527) between two
 *                             PoseOptimization calls (vba_pose_optimize, VBA_FRAME_VISION); the target is the frame, the queries are
 *                             the keypoints i of pKF in their order
 * One problem is one target and one ORDERED list of queries; one call takes any number of problems, ragged, both modes mixed, in one
 * kernel launch (one 256-lane workgroup per problem).  The queries of a problem are not independent: a match takes its keypoint away
 * from every later query (:446 and :468; :1738 and :1754).  The kernel resolves that with the order-preserving conflict pass of
 * vba_search_by_projection, with every query blocking: claim[k] is the smallest index of a query whose current result is keypoint k,
 * query q treats k as taken iff occupied[k] || claim[k] < q, and rounds of (every open query walks against the table of the round
 * before; the table is rebuilt) run until a round changes nothing.  `rounds` counts them, the detecting round included; it is at most
 * n_q + 1.  The reference is restated as it stands:
 *   loop    p3Dc = Rcw p + tcw; z < 0 leaves (:395; z == 0 passes and fails IsInImage); invz = 1 / z, u = fx * (xc * invz) + cx, v alike
 *           (:399-404); IsInImage is the positive conjunction u >= minX && u < maxX && v >= minY && v < maxY (:407); dist = |p - Ow|
 *           outside [q_dist_min, q_dist_max] leaves (:417); PO . Pn < cos_view * dist leaves (:423); nPredictedLevel =
 *           ceil(log(q_pred_max / dist) / log_scale_factor) (:426); radius = th * scale[level] (:430); KeyFrame::GetFeaturesInArea(u, v,
 *           radius) without level arguments, so the area counts as non-empty whatever the levels of its keypoints (:434); per
 *           candidate: taken -> skip (:446), kpLevel < level - 1 || kpLevel > level -> skip (:451), dist < bestDist strict (:458);
 *           bestDist <= th_dist matches (:466).  No ratio test, no orientation filter; n_matches counts the matches of this call only
 *   reloc   x3Dc = Rcw p + tcw; NO depth test: invzc = 1.0 / z, u = (fx * xc) * invzc + cx, v alike (:1698-1701), so a point behind
 *           the camera that lands inside the bounds goes on and can match; u < minX || u > maxX || v < minY || v > maxY leaves
 *           (:1703-1706); dist3D = |p - Ow| outside [q_dist_min, q_dist_max] leaves (:1716); no viewing-angle test; the level as in
 *           loop mode (:1719); radius = th * scale[level] (:1722); Frame::GetFeaturesInArea(u, v, radius, level - 1, level + 1) with the
 *           level test INSIDE the cell loop: an area that holds only other levels is empty (:1727); per candidate: taken -> skip
 *           (:1738), dist < bestDist strict (:1745); bestDist <= th_dist matches (:1752); with check_orientation the bin of
 *           :1760-1766 in float32 with C round, rotHist[bin] holds bestIdx2, and ComputeThreeMaxima and the drop (:1775-1794) run in
 *           the write-back: the drop clears the keypoint and decrements n_matches
 *   area    GetFeaturesInArea literally (src/KeyFrame.cpp:1071-1115, src/Frame.cpp:562-620): floor for the first cell and CEIL for the
 *           last one, the four early returns, the clamps, fabs(dx) < r && fabs(dy) < r; candidates in cell order (ix outer, iy inner)
 *           and inside a cell in list order
 * Deviations, those of the sibling entry points: the reference reads mvScaleFactors[nPredictedLevel] unchecked (:430, :1722), here a
 * level outside 0 .. n_levels - 1 leaves with its own state; a non-finite u or v leaves as "outside the image" (the reference's
 * reloc tests let a NaN through); with th_dist = 256 a query whose candidates all fail leaves as bestDist > th_dist does instead of
 * indexing with -1.  `state` says where a query left, numbered in the order of the reference's exits.  Loop mode:
 *   0  matched      1  skipped (q_skip)      2  z < 0 (:395)      3  not in the image (:407)      4  distance (:417)
 *   5  viewing angle (:423)      6  level outside 0 .. n_levels - 1      7  area empty (:434)
 *   8  bestDist > th_dist (:466), every candidate taken or of the wrong level included
 * Reloc mode:
 *   0  matched and kept      1  skipped (q_skip)      2  outside the image (:1703-1706)      3  distance (:1716)
 *   4  level outside 0 .. n_levels - 1      5  area empty (:1727)      6  bestDist > th_dist (:1752), every candidate taken included
 *   7  matched, then dropped by the orientation filter (:1783-1793)
 * Everything but the bin is FP64 on the float32 inputs widened; the reference computes in float32. */
#define VBA_SEARCH_PROJ_KF_LOOP  0   /* :354-475  */
#define VBA_SEARCH_PROJ_KF_RELOC 1   /* :1667-1797 */
#define VBA_SEARCH_PROJ_KF_MAX_KEYS 16384   /* the claim table of a target lives in LDS */
typedef struct vba_search_proj_kf_problem {
    int32_t mode;                    /* VBA_SEARCH_PROJ_KF_LOOP or VBA_SEARCH_PROJ_KF_RELOC */
    int32_t check_orientation;       /* mbCheckOrientation (:1758, :1775); reloc mode only */
    double Rcw[9], tcw[3];           /* row-major.  loop: Scw decomposed as :364-367 (Rcw = sRcw / scw, tcw = Scw.col(3) / scw), as for
                                        vba_fuse; reloc: CurrentFrame.mTcw (:1672-1673) */
    double Ow[3];                    /* -Rcw^T tcw, formed by the caller (:368, :1674) */
    double K[4];                     /* fx fy cx cy of the target (:358-361, :1700-1701) */
    double bounds[4];                /* mnMinX mnMaxX mnMinY mnMaxY of the target */
    int32_t n_keys;                  /* pKF->N / CurrentFrame.N; at most VBA_SEARCH_PROJ_KF_MAX_KEYS */
    int32_t n_levels;                /* mnScaleLevels of the target, 1 .. 64 */
    const uint8_t *desc;             /* [n_keys][32] mDescriptors of the target (:454, :1741) */
    const double *uv;                /* [n_keys][2] mvKeysUn[idx].pt */
    const uint8_t *oct;              /* [n_keys] mvKeysUn[idx].octave (:449) */
    const float *angle;              /* [n_keys] CurrentFrame.mvKeysUn[idx].angle in [0, 360) (:1760); reloc mode with check_orientation only */
    const double *scale;             /* [n_levels] mvScaleFactors of the target (:430, :1722) */
    double log_scale_factor;         /* mfLogScaleFactor of the target (:426, :1719) */
    int32_t grid_cols, grid_rows;    /* the target's grid; >= 1, cols * rows <= 65536 */
    double grid_inv_w, grid_inv_h;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t *cell_begin;       /* [cols * rows + 1] as in vba_fuse_problem */
    const int32_t *cell_feat;        /* keypoint indices in the order the grid's cells hold them; each keypoint at most once */
    const uint8_t *occupied;         /* [n_keys] non-zero: loop, vpMatched[idx] != NULL (:446); reloc, mvpMapPoints[i2] != NULL (:1738).  No
                                        Observations() test in either */
    int32_t n_q;                     /* vpPoints.size() / vpMPs.size(): the queries in the reference's loop order */
    int32_t th_dist;                 /* loop: TH_LOW = 50 (:466); reloc: ORBdist (:1752); 0 .. 256 */
    double th;                       /* the radius factor: 10 in loop mode (LoopClosing.cpp:470); 10 or 3 in reloc mode (Tracking.cpp:2513, :2527) */
    double cos_view;                 /* 0.5 (:423); loop mode only */
    const double *q_pos;             /* [n_q][3] GetWorldPos() */
    const uint8_t *q_desc;           /* [n_q][32] GetDescriptor() */
    const uint8_t *q_skip;           /* [n_q] non-zero: loop, isBad() || spAlreadyFound.count(pMP) with the set as built at :372 and not updated
                                        (:385); reloc, !pMP || isBad() || sAlreadyFound.count(pMP) (:1688-1690) */
    const double *q_normal;          /* [n_q][3] GetNormal() (:421); loop mode only */
    const double *q_dist_min, *q_dist_max; /* [n_q] GetMinDistanceInvariance(), GetMaxDistanceInvariance() as the reference returns them */
    const double *q_pred_max;        /* [n_q] mfMaxDistance, which PredictScale reads */
    const float *q_angle;            /* [n_q] pKF->mvKeysUn[i].angle in [0, 360) (:1760); reloc mode with check_orientation only */
} vba_search_proj_kf_problem;

typedef struct vba_search_proj_kf_result {
    int32_t status;           /* VBA_OK */
    int32_t n_matches;        /* the return value of the function */
    int32_t n_before_filter;  /* nmatches in front of the orientation filter (:1775); n_matches without one */
    int32_t hist[30];         /* rotHist[i].size() in front of the filter (zeros in loop mode and without check_orientation) */
    int32_t ind[3];           /* ind1 .. ind3 of ComputeThreeMaxima, -1 as the reference leaves them (and without the filter) */
    int32_t rounds;           /* rounds of the conflict pass, 1 .. n_q + 1 */
    int32_t *best_idx;        /* [n_q] caller-allocated: bestIdx as the candidate loop left it, -1 for none */
    uint16_t *best_dist;      /* [n_q] caller-allocated: bestDist; 256 = none */
    int8_t *level;            /* [n_q] caller-allocated: nPredictedLevel where it was computed and in range, the out-of-range value
                                 clamped to int8 for the level state (6 in loop mode, 4 in reloc mode); -128 where not computed */
    double *uv;               /* [n_q][2] caller-allocated: the projection; NaN where not computed (loop: states 1 and 2; reloc: state 1) */
    uint8_t *bin;             /* [n_q] caller-allocated: the histogram bin of a match (reloc states 0 and 7) with check_orientation; 255 = none */
    uint8_t *state;           /* [n_q] caller-allocated: the codes above */
    int32_t *key_match;       /* [n_keys] caller-allocated: what the function writes into vpMatched / mvpMapPoints, as a query index: -1
                                 untouched, -2 cleared by the orientation filter (:1789), else the query that wrote the keypoint */
} vba_search_proj_kf_result;

/* Synchronous, like vba_search_by_projection; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; a problem with
 * n_q == 0 or n_keys == 0 is legal.  A bad problem fails the whole call before any GPU work, with nothing written, as
 * "vba_search_by_projection_kf: problem K: <why>" through vba_last_error: a NULL problem or result, an unknown mode, a negative count,
 * n_keys above VBA_SEARCH_PROJ_KF_MAX_KEYS, a NULL array with a non-zero count (the per-query result arrays are required when
 * n_q > 0, key_match when n_keys > 0; the arrays of the other mode may be NULL), n_levels outside 1 .. 64, an octave >= n_levels,
 * th_dist outside 0 .. 256, grid sizes outside their range, a cell_begin that does not start at 0, decreases or ends above n_keys, a
 * cell_feat entry out of range or listed twice, with check_orientation in reloc mode an angle outside [0, 360), any non-finite pose,
 * intrinsic, bound, pixel, level table, position, normal, distance or threshold that the mode reads.  A problem's outputs do not
 * depend on where it stands in the batch. */
int vba_search_by_projection_kf(void *handle, int32_t n_problems, vba_search_proj_kf_problem *const *in, vba_search_proj_kf_result *const *out);

/* ---- bag-of-words matching ----
 * Both ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cpp), selected by `mode`:
 *   VBA_SEARCH_BOW_KF_FRAME  SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:207-350): Tracking::TrackReferenceKeyFrame
 *                            (src/Tracking.cpp:1600, in front of vba_pose_optimize) and Tracking::Relocalization (:2429)
 *   VBA_SEARCH_BOW_KF_KF     SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:609-748): LoopClosing::ComputeSim3
 *                            (src/LoopClosing.cpp:317, in front of vba_sim3_ransac)
 * One problem is one pair (side 1: the keyframe whose map points are carried over; side 2: the frame or the second keyframe); one
 * call takes any number of pairs, ragged, both modes mixed, in one kernel launch (one 256-lane workgroup per pair).  The reference
 * is restated as it stands:
 *   node join   the two feature vectors are walked as the `while` of :229-322 / :639-725 does (equal ids: the node is shared; else
 *               lower_bound on the side that is behind).  Every keypoint of side 1 in a shared node is visited in the order the
 *               node lists it; it leaves when it has no map point or a bad one (:243-247, :649-652: good_mp1)
 *   query       bestDist1 = 256, bestIdx = -1, bestDist2 = 256.  Every keypoint of side 2 in the same node, in list order: skipped
 *               when it is TAKEN by an earlier match of this call (:260 vpMapPointMatches[realIdxF], :667 vbMatched2[idx2]) and, in
 *               KF_KF mode only, when it has no map point or a bad one (:667-671: good_mp2); otherwise dist < bestDist1 (strict)
 *               moves the best to the second and replaces the best, else dist < bestDist2 replaces the second.  Among equal
 *               distances the FIRST in list order is the best and the equal one becomes bestDist2
 *   threshold   bestDist1 <= th_low in KF_FRAME mode (:280), bestDist1 < th_low in KF_KF mode (:691)
 *   ratio       (float)bestDist1 < nn_ratio * (float)bestDist2, the product in float32 (:284, :693)
 *   match       the keypoint of side 2 is taken for every later query (:287, :696); nmatches++
 *   orientation rot = angle1 - angle2; if (rot < 0) rot += 360.0f; bin = round(rot * (1.0f / 30)) in float32 with C round (:296-303,
 *               :700-707), ComputeThreeMaxima (:1800-1841), every match of another bin cleared and nmatches-- (:325-347, :727-745).  The
 *               drop clears outputs only: the walk is over, nothing is un-taken
 * The queries of a pair are not independent: a query reads the taken flags earlier queries wrote.  It reads them only for keypoints
 * of side 2 in its own node, and a keypoint is listed in at most one node, so queries of different shared nodes never interact.
 * Taking a query's best candidate away changes bestDist1 AND bestDist2, so a query can move between matched, ratio test failed and
 * threshold failed.  The kernel resolves that with an order-preserving conflict pass whose result is the sequential one (rounds of
 * every open query against the claim table of the round before, the table rebuilt, until a round changes no claim); `rounds` counts
 * them, the detecting round included, and is at most (the largest number of queries in one shared node) + 1 (DESIGN.md section 8,
 * row f-14, has the proof).
 * `state` says where a keypoint of side 1 left the function, numbered in the order of the reference's exits:
 *   0  matched and kept
 *   1  no good map point (:243-247, :649-652); this wins over 2
 *   2  no node that both sides list holds it
 *   3  threshold failed (:280, :691), "no candidate" and "every candidate taken" included
 *   4  ratio test failed (:284, :693)
 *   5  matched, then dropped by the orientation filter (:343, :741)
 * Every output is an integer; float32 appears in the ratio product and in the bin only. */
#define VBA_SEARCH_BOW_KF_FRAME 0      /* :207-350, threshold <=, every side-2 keypoint is a candidate */
#define VBA_SEARCH_BOW_KF_KF    1      /* :609-748, threshold <,  side-2 keypoints without a good map point are no candidates */
#define VBA_SEARCH_BOW_MAX_KEYS 16384  /* the claim table of side 2 lives in LDS */
typedef struct vba_search_bow_problem {
    int32_t mode;                    /* VBA_SEARCH_BOW_KF_FRAME or VBA_SEARCH_BOW_KF_KF */
    int32_t check_orientation;       /* mbCheckOrientation (:291, :325, :698, :727) */
    int32_t th_low;                  /* TH_LOW = 50 (:280, :691); 0 .. 255 */
    float nn_ratio;                  /* mfNNratio: 0.75f at src/LoopClosing.cpp:285, 0.7f at src/Tracking.cpp:1597, 0.75f at :2405 */
    int32_t n_keys1, n_keys2;        /* pKF->N / F.N; n_keys2 at most VBA_SEARCH_BOW_MAX_KEYS */
    const uint8_t *desc1, *desc2;    /* [n_keys][32] the rows of mDescriptors (:249, :263) */
    const uint8_t *good_mp1;         /* [n_keys1] non-zero: map point present and not bad (:243-247) */
    const uint8_t *good_mp2;         /* [n_keys2] the same of side 2 (:665-671); read in KF_KF mode only, may be NULL in KF_FRAME mode */
    const float *angle1, *angle2;    /* [n_keys] mvKeysUn[idx].angle / F.mvKeys[idx].angle in [0, 360) (:296, :700); read with check_orientation only */
    int32_t n_nodes1, n_nodes2;      /* entries of mFeatVec */
    const uint32_t *node_id1, *node_id2;      /* [n_nodes] strictly ascending: the order of the std::map */
    const int32_t *node_begin1, *node_begin2; /* [n_nodes + 1] node k lists node_feat[node_begin[k] .. node_begin[k + 1]) */
    const int32_t *node_feat1, *node_feat2;   /* keypoint indices in the order the node's vector holds them; each keypoint at most once */
} vba_search_bow_problem;

typedef struct vba_search_bow_result {
    int32_t status;           /* VBA_OK */
    int32_t n_matches;        /* the return value (:349, :747) */
    int32_t n_before_filter;  /* nmatches in front of the orientation filter; n_matches without one */
    int32_t hist[30];         /* rotHist[i].size() in front of the filter (zeros without check_orientation) */
    int32_t ind[3];           /* ind1 .. ind3 of ComputeThreeMaxima, -1 as the reference leaves them (and without check_orientation) */
    int32_t rounds;           /* rounds of the conflict pass, 1 .. (largest number of queries in one shared node) + 1 */
    int32_t *match12;         /* [n_keys1] caller-allocated: the keypoint of side 2 behind the filter, -1 otherwise (vpMatches12 as an index) */
    int32_t *best_idx;        /* [n_keys1] caller-allocated: bestIdx as the candidate loop left it, -1 if none (and in the states 1, 2) */
    uint16_t *best_dist;      /* [n_keys1] caller-allocated: bestDist1; 256 = none */
    uint16_t *best_dist2;     /* [n_keys1] caller-allocated: bestDist2; 256 = none */
    uint8_t *bin;             /* [n_keys1] caller-allocated: the histogram bin of a match (states 0 and 5) with check_orientation; 255 = none */
    uint8_t *state;           /* [n_keys1] caller-allocated: the codes above */
    int32_t *match21;         /* [n_keys2] caller-allocated: the keypoint of side 1 whose match the function leaves there: -1 untouched, -2
                                 set and then cleared by the orientation filter.  In KF_FRAME mode exactly vpMapPointMatches as an index */
} vba_search_bow_result;

/* Synchronous, like vba_search_triangulation; -1 while asynchronous tickets are pending.  n_pairs == 0 returns 0; a pair without
 * keypoints or without a shared node is legal (n_matches = 0, every state 1 or 2, rounds = 1).  A bad pair fails the whole call
 * before any GPU work, with nothing written, as "vba_search_by_bow: pair K: <why>" through vba_last_error: a NULL problem or
 * result, an unknown mode, a negative count, n_keys2 above VBA_SEARCH_BOW_MAX_KEYS, th_low outside 0 .. 255, a non-finite nn_ratio, a
 * NULL array with a non-zero count (match12, best_idx, best_dist, best_dist2, bin and state are required when n_keys1 > 0, match21
 * when n_keys2 > 0, good_mp2 in KF_KF mode), node ids that are not strictly ascending, a node_begin that does not start at 0 or
 * decreases, a keypoint index outside its side or listed twice in one feature vector, and with check_orientation a NULL angle array
 * or an angle outside [0, 360).  A pair's outputs do not depend on where it stands in the batch. */
int vba_search_by_bow(void *handle, int32_t n_pairs, vba_search_bow_problem *const *in, vba_search_bow_result *const *out);

/* ---- matching for the monocular initialisation ----
 * ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cpp:477-595), which
 * Tracking::MonocularInitialization calls on every frame until a map exists (src/Tracking.cpp:1371-1373), directly in front of
 * Initializer::Initialize (vba_two_view_init).  One problem is one frame pair; one call takes any number of pairs, ragged, in one
 * kernel launch (one 256-lane workgroup per pair).  The reference is restated as it stands:
 *   level gate  every keypoint i1 of frame 1, in index order, leaves when its octave is > 0 (:495)
 *   area        F2.GetFeaturesInArea(vbPrevMatched[i1].x, .y, windowSize, 0, 0) (src/Frame.cpp:562-620): both level arguments are 0, so
 *               bCheckLevels is true and the level test runs INSIDE the cell loop, in front of the pixel test: a candidate has octave
 *               0, and an area that holds only other levels is empty (:501).  Floor for the first cell and CEIL for the last one, the
 *               four early returns, the clamps, fabs(dx) < r && fabs(dy) < r; candidates in cell order (ix outer, iy inner) and inside
 *               a cell in list order
 *   candidates  `if (vMatchedDistance[i2] <= dist) continue;` comes first (:518): a skipped candidate counts for neither distance.
 *               Then dist < bestDist (strict) moves the best to the second and replaces the best, else dist < bestDist2 replaces the
 *               second (:521-530).  bestDist, bestDist2 and vMatchedDistance start at INT_MAX, not at 256
 *   threshold   bestDist <= th_low (:534)
 *   ratio       bestDist < (float)bestDist2 * nn_ratio in float32 (:536); with one surviving candidate the right-hand side is
 *               (float)INT_MAX * nn_ratio, and it is evaluated so although best_dist2 REPORTS "none" as 256
 *   match       if vnMatches21[bestIdx2] >= 0 that earlier query loses its match (vnMatches12[..] = -1, nmatches--); then
 *               vnMatches12[i1], vnMatches21[bestIdx2] and vMatchedDistance[bestIdx2] = bestDist are set and nmatches++ (:538-546)
 *   orientation rot = angle1 - angle2; if (rot < 0) rot += 360.0f; bin = round(rot * (1.0f / 30)) in float32 with C round (:550-555);
 *               rotHist[bin] receives i1 and KEEPS it when the match is stolen later, so stolen matches count in ComputeThreeMaxima
 *               (:570); the drop clears and decrements only where vnMatches12[idx1] >= 0 (:579-582) and leaves vnMatches21 alone
 *   positions   vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt for every match kept (:590-592)
 * The queries of a pair are not independent: query q reads vMatchedDistance[k] as the queries before it left it, which is
 * min { bestDist_p : p < q, p accepted, bestIdx_p = k } (INT_MAX for the empty set), and a later query can take a keypoint away from an
 * earlier one.  The kernel keeps per keypoint of frame 2 the list of its current claimers and runs the order-preserving conflict
 * pass of the other ordered matchers over it: rounds of (every open query walks against the lists of the round before; the lists
 * are rebuilt) until a round changes no claim.  Any fixed point is the sequential answer, and `rounds`, the detecting round
 * included, is at most (level-0 keypoints of frame 1) + 1 (has the proof).
 * `state` says where a keypoint of frame 1 left the function, numbered in the order of the reference's exits:
 *   0  matched and kept
 *   1  octave > 0 (:495)
 *   2  area empty (:501)
 *   3  bestDist > th_low (:534), every candidate skipped included
 *   4  ratio test failed (:536)
 *   5  matched, then replaced by a later query (:538-541); this wins over 6
 *   6  matched, then dropped by the orientation filter (:579-582)
 * Every decision is an integer one but the area: it is FP64 on the float32 inputs widened, the reference computes it in float32.
 * float32 appears in the ratio product and in the bin only.  Stereo is out of scope. */
#define VBA_SEARCH_INIT_MAX_KEYS 16384  /* the claimer lists of frame 2 live in LDS */
typedef struct vba_search_init_problem {
    int32_t check_orientation;       /* mbCheckOrientation (:548, :564) */
    int32_t th_low;                  /* TH_LOW = 50 (:534); 0 .. 255 */
    float nn_ratio;                  /* mfNNratio: 0.9f at src/Tracking.cpp:1371 */
    double window_size;              /* windowSize: 100 at src/Tracking.cpp:1372; finite, a negative value is legal and matches nothing */
    int32_t n_keys1;                 /* F1.mvKeysUn.size() */
    const uint8_t *desc1;            /* [n_keys1][32] the rows of F1.mDescriptors (:504) */
    const uint8_t *oct1;             /* [n_keys1] F1.mvKeysUn[i1].octave (:494) */
    const float *angle1;             /* [n_keys1] F1.mvKeysUn[i1].angle in [0, 360) (:550); read with check_orientation only */
    const float *prev_matched;       /* [n_keys1][2] vbPrevMatched as the caller holds it (:498); finite */
    int32_t n_keys2;                 /* F2.mvKeysUn.size(); at most VBA_SEARCH_INIT_MAX_KEYS */
    const uint8_t *desc2;            /* [n_keys2][32] the rows of F2.mDescriptors (:514) */
    const double *uv2;               /* [n_keys2][2] F2.mvKeysUn[i2].pt */
    const uint8_t *oct2;             /* [n_keys2] F2.mvKeysUn[i2].octave (src/Frame.cpp:602) */
    const float *angle2;             /* [n_keys2] F2.mvKeysUn[i2].angle in [0, 360) (:550); read with check_orientation only */
    double bounds[4];                /* mnMinX mnMaxX mnMinY mnMaxY of frame 2 */
    int32_t grid_cols, grid_rows;    /* frame 2's grid; >= 1, cols * rows <= 65536 */
    double grid_inv_w, grid_inv_h;   /* mfGridElementWidthInv, mfGridElementHeightInv */
    const int32_t *cell_begin;       /* [cols * rows + 1] as in vba_fuse_problem */
    const int32_t *cell_feat;        /* keypoint indices in the order the grid's cells hold them; each keypoint at most once */
} vba_search_init_problem;

typedef struct vba_search_init_result {
    int32_t status;           /* VBA_OK */
    int32_t n_matches;        /* the return value (:594) */
    int32_t n_before_filter;  /* nmatches in front of the orientation filter (:564), net of steals; n_matches without one */
    int32_t n_stolen;         /* how often :538-541 took a match back */
    int32_t hist[30];         /* rotHist[i].size() in front of the filter, stolen entries counted (zeros without check_orientation) */
    int32_t ind[3];           /* ind1 .. ind3 of ComputeThreeMaxima, -1 as the reference leaves them (and without check_orientation) */
    int32_t rounds;           /* rounds of the conflict pass, 1 .. (level-0 keypoints of frame 1) + 1 */
    int32_t *match12;         /* [n_keys1] caller-allocated: vnMatches12 as the function leaves it */
    int32_t *best_idx;        /* [n_keys1] caller-allocated: bestIdx2 as the candidate loop left it, -1 if none (and in the states 1, 2) */
    uint16_t *best_dist;      /* [n_keys1] caller-allocated: bestDist; 256 = none */
    uint16_t *best_dist2;     /* [n_keys1] caller-allocated: bestDist2; 256 = none */
    uint8_t *bin;             /* [n_keys1] caller-allocated: the histogram bin of a match (states 0, 5 and 6) with check_orientation; 255 = none */
    uint8_t *state;           /* [n_keys1] caller-allocated: the codes above */
    float *prev_matched;      /* [n_keys1][2] caller-allocated: a copy of the problem's prev_matched with :590-592 applied */
    int32_t *match21;         /* [n_keys2] caller-allocated: vnMatches21 as the function leaves it; the filter does not clear it */
    uint16_t *matched_dist;   /* [n_keys2] caller-allocated: vMatchedDistance as the function leaves it; 256 = none */
} vba_search_init_result;

/* Synchronous, like vba_search_by_bow; -1 while asynchronous tickets are pending.  n_pairs == 0 returns 0; a pair with n_keys1 == 0
 * or n_keys2 == 0 is legal (n_matches = 0, rounds = 1).  A bad pair fails the whole call before any GPU work, with nothing written,
 * as "vba_search_for_initialization: pair K: <why>" through vba_last_error: a NULL problem or result, a negative count, n_keys2 above
 * VBA_SEARCH_INIT_MAX_KEYS, th_low outside 0 .. 255, a non-finite nn_ratio or window_size, grid sizes outside their range, a NULL
 * array with a non-zero count (every per-keypoint result array of a side is required when the side has keypoints; the angles only
 * with check_orientation), a non-finite bound, cell size, pixel or prev_matched entry, with check_orientation an angle outside
 * [0, 360), a cell_begin that does not start at 0, decreases or ends above n_keys2, a cell_feat entry out of range or listed twice.
 * A pair's outputs do not depend on where it stands in the batch. */
int vba_search_for_initialization(void *handle, int32_t n_pairs, vba_search_init_problem *const *in, vba_search_init_result *const *out);

/* ---- map-point refresh: representative descriptor, mean viewing direction, scale-invariance range ----
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:336-413) and MapPoint::UpdateNormalAndDepth (:450-501), which
 * LocalMapping calls as a pair for every map point of the current keyframe (src/LocalMapping.cpp:1144-1171, :1532-1534, :1635-1650)
 * and every BA write-back calls for every local map point (src/Optimizer.cpp:605, :3328, :4213, :4545).  They produce what the
 * matchers read: pt_desc, normal, dist_min, dist_max of vba_fuse and its siblings.  One problem is one list of points over one table
 * of keyframes; one call takes any number of problems, ragged, in one kernel launch.  The reference is restated as it stands:
 *   descriptor  the observations in the order of mObservations, ascending keyframe id (:19-22); an observation whose keyframe isBad()
 *               contributes no descriptor (:360); with no observation (:349) or none from a good keyframe (:364) nothing is written.
 *               Otherwise N descriptors remain, Distances[i][j] is the 256-bit Hamming distance with a diagonal of 0, row i is sorted
 *               and its median is the entry (int)(0.5 * (N - 1)) (:394): the LOWER median, for N = 2 the 0 of the diagonal.  The first
 *               row with a strictly smaller median wins (:397); N = 1 gives median 0 and row 0
 *   normal      with no observation, return (:467).  normal = the sum over ALL observations, bad keyframes included (:472-481 has no
 *               isBad test), of (Pos - Ow_i) / |Pos - Ow_i|, divided by their count (:498); dist = |Pos - Ow_ref| (:484-485);
 *               mfMaxDistance = dist * mvScaleFactors[level] (:494), mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1] (:496),
 *               level the octave of the reference keyframe's keypoint observations[pRefKF] (:486).  `observations` is a local std::map:
 *               when the reference keyframe is no observer, operator[] inserts 0 and keypoint 0 is read.  The two scale factors are
 *               per-point inputs here, so that lookup stays with the caller
 * FP64 where the reference computes in float32 (cv::Mat CV_32F, cv::norm accumulating in double); a caller narrows to float32 when it
 * writes back.  One declared deviation: a point that coincides exactly with an observer's camera centre (|Pos - Ow_i| = 0), where the
 * reference divides by zero and stores NaN: the normal part leaves with normal_state 3 and writes nothing for the point.
 * desc_state / normal_state say where a part left:
 *   0  done
 *   1  not asked (its bit of `what` is clear)
 *   2  no observations (:349 / :467)
 *   3  descriptor: no observation from a good keyframe (:364); normal: the point lies in an observer's camera centre */
#define VBA_MAPPOINT_MAX_OBS 1024   /* observations of one point: its descriptors live in LDS */
#define VBA_MAPPOINT_DESC 1         /* bit of `what`: ComputeDistinctiveDescriptors */
#define VBA_MAPPOINT_NORMAL 2       /* bit of `what`: UpdateNormalAndDepth */
typedef struct vba_mappoint_problem {
    int32_t n_kf;                    /* keyframes of the table */
    const double *kf_center;         /* [n_kf][3] KeyFrame::GetCameraCenter (:476, :484); read when a point asks for the normal part */
    const uint8_t *kf_bad;           /* [n_kf] KeyFrame::isBad (:360); read when a point asks for the descriptor part */
    int32_t n_pt;                    /* points */
    const uint8_t *what;             /* [n_pt] VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL; 0 is legal */
    const double *pos;               /* [n_pt][3] mWorldPos (:464); may be NULL when no point asks for the normal part, like the next three */
    const int32_t *ref_kf;           /* [n_pt] mpRefKF as an index into the table (:463) */
    const double *ref_scale;         /* [n_pt] pRefKF->mvScaleFactors[level] (:486-487); > 0 */
    const double *ref_top_scale;     /* [n_pt] pRefKF->mvScaleFactors[nLevels - 1] (:496); > 0 */
    const int32_t *obs_begin;        /* [n_pt + 1] CSR: the observations of point i are obs_begin[i] .. obs_begin[i + 1], in the order of
                                        mObservations; at most VBA_MAPPOINT_MAX_OBS of them */
    const int32_t *obs_kf;           /* [obs_begin[n_pt]] the observing keyframe as an index into the table */
    const uint8_t *obs_desc;         /* [obs_begin[n_pt]][32] pKF->mDescriptors.row(mit->second) (:361), gathered by the caller; may be NULL
                                        when no point asks for the descriptor part */
} vba_mappoint_problem;

typedef struct vba_mappoint_result {
    int32_t status;           /* VBA_OK */
    int32_t n_desc_done;      /* points with desc_state 0 */
    int32_t n_normal_done;    /* points with normal_state 0 */
    int32_t *best_obs;        /* [n_pt] caller-allocated: BestIdx (:400) as an index INTO THE POINT'S OBSERVATION LIST, bad keyframes counted;
                                 -1 where the descriptor part did not run to its end */
    int32_t *best_median;     /* [n_pt] caller-allocated: BestMedian (:399); -1 likewise */
    int32_t *n_desc;          /* [n_pt] caller-allocated: N (:368); 0 where the part was not asked */
    uint8_t *desc;            /* [n_pt][32] caller-allocated: the winning row (:410), ready to be pt_desc of vba_fuse; zeros where none */
    double *normal;           /* [n_pt][3] caller-allocated: mNormalVector (:498); 0.0 where the normal part did not run to its end */
    double *dist_max;         /* [n_pt] caller-allocated: mfMaxDistance (:494); 0.0 likewise */
    double *dist_min;         /* [n_pt] caller-allocated: mfMinDistance (:496); 0.0 likewise */
    uint8_t *desc_state;      /* [n_pt] caller-allocated: the codes above */
    uint8_t *normal_state;    /* [n_pt] caller-allocated: the codes above */
} vba_mappoint_result;

/* Synchronous, like vba_fuse; -1 while asynchronous tickets are pending.  n_problems == 0 returns 0; a problem with n_pt == 0 or
 * n_kf == 0 is legal (a point of a table without keyframes can have no observation).  A bad problem fails the whole call before any
 * GPU work, with nothing written, as "vba_mappoint_update: problem K: <why>" through vba_last_error: a NULL problem or result, a
 * negative count, with n_pt > 0 a NULL what, obs_begin or result array, an obs_begin that does not start at 0 or decreases, a list
 * above VBA_MAPPOINT_MAX_OBS, a bit of `what` outside the two, a NULL array that a requested part needs (obs_kf with observations;
 * kf_bad and obs_desc for the descriptor part; kf_center, pos, ref_kf and both scale arrays for the normal part), and for the points
 * that ask for the part that reads them: an obs_kf or ref_kf out of range, a non-finite position or scale, a scale <= 0; with a
 * normal part in the problem a non-finite centre.  A point's outputs do not depend on where it stands in the batch. */
int vba_mappoint_update(void *handle, int32_t n_problems, vba_mappoint_problem *const *in, vba_mappoint_result *const *out);

/* ---- essential-graph optimisation (Sim3 pose graph) ----
 * Optimizer::OptimizeEssentialGraph(Map*, KeyFrame* pLoopKF, KeyFrame* pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
 * bFixScale, LoopClosing*)   src/Optimizer.cpp:4243-4552
 * Everything between the vertex / edge set-up (:4284-4478) and the write-back (:4488-4546): optimize(20) with Levenberg-Marquardt,
 * setUserLambdaInit(1e-16) (:4256-4266, :4481-4482; schedule of optimization_algorithm_levenberg.cpp:61-164), over one
 * VertexSim3Expmap per keyframe (types_seven_dof_expmap.h:48-94) and EdgeSim3 edges (:100-124) with identity information and no
 * robust kernel; error log(Sji * Siw * Sjw^-1) (sim3.h:148-230); Jacobians by g2o's own central differences with delta = 1e-9
 * through oplus (base_binary_edge.hpp:131-205: EdgeSim3 has no linearizeOplus); then every map point moved through its reference
 * keyframe (:4511-4546).  The four pair rules that choose the edges (:4331-4478) are host work and stay with the caller.  One call
 * takes any number of independent graphs (one workgroup per graph; one kernel launch per call, two with map points). */
typedef struct vba_posegraph_problem {
    int32_t n_vertices, n_edges;
    int32_t fix_scale;            /* bFixScale: VertexSim3Expmap::_fix_scale (update[6] = 0, types_seven_dof_expmap.h:60-69) */
    int32_t its;                  /* 20 (:4482); at least 1 */
    double  lambda_init;          /* 1e-16 (:4260); must be > 0 */
    double *S;                    /* [n_vertices][8] in/out: Siw as t(3) q(4, xyzw) s, the vba_sim3_problem.S12 layout (:4284-4325);
                                   * the caller forms Tiw = [R, t/s] from it (:4488-4508) */
    const uint8_t *fixed;         /* [n_vertices] 1 = setFixed(true): the loop keyframe (:4312-4313) */
    const int32_t *edge_i, *edge_j; /* [n_edges] vertex 0 / vertex 1 of EdgeSim3 (:4349-4350 and the like); a pair may occur twice */
    const double *edge_S;         /* [n_edges][8] measurement Sji, same layout (:4347, :4393, :4419, :4454) */
    int32_t n_pt;                 /* 0 = no map-point correction */
    double *pt;                   /* [n_pt][3] in/out world positions: correctedSwr.map(Srw.map(P)) (:4540-4543) */
    const int32_t *pt_ref;        /* [n_pt] vertex whose pose change carries the point (:4518-4530) */
} vba_posegraph_problem;

typedef struct vba_posegraph_result {
    int32_t status;               /* VBA_OK */
    int32_t its_done;             /* cjIterations */
    int32_t lm_trials;            /* LM trials summed over the iterations */
    int32_t stop;                 /* 0 budget used up, 1 ten trials failed, 2 rho == 0, 3 _nBad >= 3 */
    double chi2_initial, chi2_final, lambda_final;
} vba_posegraph_result;

/* Synchronous, like vba_sim3_optimize; -1 while asynchronous tickets are pending.  n_graphs == 0 returns 0.  Bad input fails the
 * whole call before any GPU work, with a message naming the graph: negative counts, a NULL array with a non-zero count, an edge
 * index out of range, edge_i == edge_j, an edge between two fixed vertices, a non-finite entry / zero quaternion / scale <= 0 in S
 * or edge_S, its < 1, lambda_init <= 0, pt_ref out of range, a graph with no free vertex, and a call whose factors exceed 2^21
 * 7x7 blocks (mc_slam_amd/csrc/vba_host_posegraph.h).  Duplicate edges and vertices without edges are legal.  A graph with a
 * component that holds no fixed vertex is singular: it does what Levenberg-Marquardt does with it and its status stays VBA_OK. */
int vba_posegraph_optimize(void *handle, int32_t n_graphs, vba_posegraph_problem *const *inout,
                           vba_posegraph_result *const *out);

/* ---- on-disk problem format: one vba_problem per file, so that windows recorded from a live system can
 * be replayed as fixtures.  Little-endian; header "VBAP" u32 version(=2) then the scalar fields in struct order
 * (i32 variant n_kf n_kf_free n_pt n_obs n_imu algo its_stage1 its_stage2 protocol robust has_kf_fix solver reserved(0), f64 K[4]
 * T_cb[7] g_w[3] inv_bg_rw2 inv_ba_rw2 huber_vis huber_prv huber_bias chi2_th depth_min rho_min), then the arrays in struct order
 * with the sizes of the struct comments.  Version 1 (no solver / reserved ints; solver = VBA_SOLVER_LDLT) is still read.
 * vba_problem_load allocates one block that vba_problem_free releases. */
int vba_problem_save(const char *path, const vba_problem *p);
int vba_problem_load(const char *path, vba_problem **out);
void vba_problem_free(vba_problem *p);

/* Host threads one handle of this process uses for packing, the host half of the structure build and the scatter of the results:
 * this rank's share of the cores it may run on (VBA_UPLOAD_THREADS, else cores / LOCAL_WORLD_SIZE, at most 16). */
int vba_host_threads(void);

int vba_set_profile(void *handle, int32_t enable);
int vba_get_profile(void *handle, vba_profile *out);

#ifdef __cplusplus
}
#endif
#endif /* VISLAM_BA_H */
