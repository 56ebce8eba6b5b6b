// vba_layout.h -- the records the host describes a batch with and the device reads: window descriptor, control block, the
// record-size constants and the item records of the small-problem entry points.  Plain C / C++ (no HIP): included by vba_device.h for the kernels, and by the host code that lays a batch
// out (vba_host_layout.h), which the tests compile with plain g++ under sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define VBA_NB 32          // block size of the dense reduced-system factorisation
#define VBA_EREC 18        // doubles per edge record, XYZ variants (144 B): Bi (2x6), g = -Bi^T r
#define VBA_EREC1 4        // doubles per edge record, inverse-depth variant (32 B): P_c (3), sqrt(rho' w) (1); the readers
                           // rebuild Bi = [A | B_rot] from it and the observer's rotation (rebuild_edge), the diagonal walk also
                           // the weighted residual from the observation's pixel (obs_uvk, idp_edge_wres)
#define VBA_PREC 32        // doubles per point record  (256 B)
#define VBA_SLOT 6         // doubles per slot record   (48 B), inverse-depth landmarks: U only
#define VBA_SLOT3 18       // doubles per slot record, XYZ landmarks (144 B): W = Bi^T A (6x3), independent of the damping
#define VBA_IMUH 960       // doubles per IMU edge pair: 30x30 local Hessian + 30 rhs (+ pad)
#define VBA_TRACE 64
// the inverse-depth records are written and read in 16-byte pieces (three per slot record, two per edge record): every piece stays
// aligned at any record index
static_assert((VBA_SLOT * 8) % 16 == 0 && (VBA_EREC1 * 8) % 16 == 0, "inverse-depth slot and edge records: a multiple of 16 bytes");

// Linearisation products kept in HBM between k_lin2 and its consumers (variant 2, EdgePRIDP).  A "slot" is one
// (landmark, keyframe) incidence = one H_pl block: observation e -> slot slot_perm[e] (keyframe-major), reference keyframe of
// landmark p -> slot n_obs + pt_perm[p].  Jacobians are pre-scaled by sqrt(rho' * invSigma2) and never stored unreduced.
//   slot record      [0..5] U = W * sqrt(Dinv)  (W = H_pl block, 6x1): edge slots and landmark reference records alike
//   landmark scalars [0] sqrt(Dinv)  [1] beta = sqrt(Dinv) * b_l: one pair per landmark, at the CALLER's landmark index (lm_sd)
//                    -> Schur term of a keyframe pair is -U_a U_b^T, reduced rhs term -U_a beta, x_l = sD (beta - sum U.x_p)
//   edge record      [0..2] P_c  [3] s = sqrt(rho' w), 0 if the observer's pose is fixed: Bi (2x6, d/d observing KF PR,
//                    g2otypes.cpp:139-145) and Br = [-A | A N0] (d/d reference KF PR, :128-134) are rebuilt from it by the
//                    readers (rebuild_edge).  The weighted residual s r of g = -Bi^T r is not stored: its one reader, the
//                    diagonal walk, forms it from P_c, s and the pixel (u, v) of the record's observation
//   pixel copy       [0..1] (u, v) of the observation behind every edge record, at the record's position (obs_uvk): written
//                    once per upload by the structure build, so the diagonal walk reads it in sequence beside the two records
//   point record     one per RUN of consecutive landmarks with one reference keyframe:
//                    [0..20] G0 = sum Br^T Br (upper 6x6 packed)  [21..26] g0 = -sum Br^T r
struct WinDesc {
    int variant, algo;
    int n_kf, n_free, n_pt, n_obs, n_imu;
    int pdim, np, nS, nb;
    int its[2];
    int kf0, pt0, obs0, imu0;
    int pair0, n_pairs;
    int item0;      // offset into the item array
    int pimu0;      // offset into the pair-imu list
    int vec0;       // offset into rhs/x vectors (nS slots per window)
    int part0;      // offset into the chi2 partial array
    int n_part_lin; // workgroups of this window in the linearise launch (= chi2 partials; XYZ: also the max-diagonal partials)
    int n_part_pt;  // 64-landmark blocks of the window (= the computeScale partials of k_update_xyz)
    int lin_runs;   // 1: the window has the work split of the edge-parallel linearisation (lin_blk); 0: thread-per-landmark fallback
    int tl_step0;   // offset of this window's step_begin / pan_begin rows (nb + 1 entries each)
    int tl_pair0;   // offset into the tile-pair list
    int tl_pan0;    // offset into the panel-tile list
    int lb0;        // first record of the window in the k_lin2 run table
    int win;        // index of this window in the uploaded batch: the CSR-style tables (pt_obs_begin, item_begin,
                    // pimu_begin) carry one extra entry per window, so their rows start at offset + win
    int tl_kb0;     // offset of this window's column-entry table of the left-looking factorisation (pan entries + nb + 1)
    int tl_k0;      // offset into its k lists
    int order;      // elimination order: 0 = V/Bias blocks first, 1 = keyframe by keyframe
    int nc;         // chain columns: block columns [0, nc) are factored by k_chol_chain, the per-column kernels start at nc
    int ct0;        // offset (records of four ints) of the window's chain-column table (Structure::chain_tab)
    int cu0, n_cu;  // few-window regime: the window's tiles that collect updates from chain columns (k_chol_chain_upd)
    int vp_pr0, vp_prs, vp_vb0, vp_vbs;  // position of dof r of free keyframe a: r < 6 ? pr0 + prs a + r : vb0 + vbs a + r - 6
    int vp_h, vp_vb1;   // order 2 (two-sided): the V/Bias block of keyframe a >= vp_h sits at vp_vb1 - 9 a (other orders: vp_h = INT_MAX)
    int pad0[3], padn[3];  // rows of S that belong to no variable (identity): up to three ranges (order 2 pads each chain and the tail)
    int nc_split;       // > 0: the chain columns [0, nc_split) and [nc_split, nc) are independent (k_chol_chain_rows walks them side by side)
    long long S0;   // offset (doubles) into S
    long long mask0; // offset (64-bit words) of the window's landmark masks (n_pt x mwords)
    int mwords;      // 64-bit words per landmark mask = ceil(n_kf / 64)
    int adj0;        // offset into the keyframe adjacency list (PCG)
    double K[4];
    double Rcb[9], tcb[3], g[3];
    double inv_bg, inv_ba;
    double hub_vis, hub_prv, hub_bias;
    double chi2_th, depth_min, rho_min;
    int protocol;    // VBA_PROTO_*: 1 = one optimize(its[0]) and no outlier pass (global BA)
    int robust;      // protocol 1: Huber on every edge, or on none
};

struct WinCtrl {
    int stage;        // 0,1
    int it;           // outer iteration inside the stage
    int active;       // 1 while the stage's optimize() loop is still running for this window
    int status;
    int its_done[2];
    int robust_vis;   // Huber on vision edges (stage 1)
    int chol_fail;    // set by the factorisation of the current iteration
    int aborted;      // stop flag seen
    int n_trace;
    int n_outliers;
    // LM state (levenberg.cpp)
    int lm_trial;     // trials done in the current outer iteration (qmax)
    int lm_need_trial;// 1: another trial must run in this outer iteration
    int lm_restore;   // 1: the last trial was rejected, k_restore must pop the state
    int nbad;
    int lin_its;      // PCG iterations of all solves so far
    int polls;        // terminate() polls of this window so far (test hook vba_debug_set_stop_after; oracle twin: stop_now)
    double lambda, ni;
    double chi_prev;  // GN: preChi2 of the last started iteration.  LM: currentChi
    double chi_ini;   // LM: iniChi
    double chi2_vis, chi2_prv, chi2_bias;
    double trace[VBA_TRACE];
    // Gauss-Newton, inverse-depth variant: the chi2-only probe of a pass that is expected to stop the window (k_ctrl_gn, LIN_AUTO /
    // LIN_REDO).  The last four ints of the block: a reader finds them at sizeof(WinCtrl) - 16 .. - 4 (vba_debug_window_layout [13])
    int lin_probe;    // 1: the window's next linearisation pass evaluates chi2 only
    int lin_redo;     // 1: the probe did not stop the window, the full pass is owed before the solve
    int n_probe;      // chi2-only passes of this run
    int n_redo;       // full passes redone behind a probe
};
static_assert(offsetof(WinCtrl, n_redo) + 4 == sizeof(WinCtrl) && offsetof(WinCtrl, lin_probe) + 16 == sizeof(WinCtrl),
              "the probe state is the tail of WinCtrl: tests read it from sizeof(WinCtrl) backwards");

// ---- the small-problem entry points: per-item descriptor (host -> device), result record (device -> host) and the *Batch of
// device pointers a kernel takes as its argument (filled by bind() of the topic's call object, vba_host_<topic>.h)
// vba_pose_optimize (vba_pose.h)
struct FrameDesc {
    int last_is_frame, compute_marg, n_obs, n_last;
    int obs0, last0;           // offsets into the concatenated observation arrays
    int pad0, pad1;
    double nav[22], nav_last[22], prior_nav[22];
    double K[4], Rcb[9], tcb[3], g[3];
    double meas[61];
    double info_pvr[81];       // inverse of the P,V,phi covariance (host, as the reference's set-up code does)
    double prior_info[225];
    double inv_bg, inv_ba;
    double hub_prior, hub_pvr, hub_bias, hub_mono;  // float-rounded Huber widths (:1741, :2107, :2125, :2137)
};
struct FrameOut {
    int n_inliers, status, its[4];
    int pad[2];
    double chi2_round[4];
    double nav[22];
    double marg[225];
};
struct PoseBatch {
    const FrameDesc* desc;
    FrameOut* out;
    const double *pw, *uv, *w;   // [total obs] current-frame observations first, then the last frames'
    double* err;                 // [total obs][2] stored _error of every mono edge
    unsigned char* lvl;          // [total obs] g2o level (1 = outlier, outside the active set)
    int n_frames;
};
// vba_sim3_optimize (vba_sim3.h)
struct Sim3Desc {
    int n_pairs, fix_scale;
    int its1, its2_bad, its2_clean, min_inliers;
    long long pair0;           // offset of the candidate's pairs in the concatenated arrays
    double S[8];               // t(3) q(4, xyzw) s
    double K1[4], K2[4];
    double th2, huber;
};
struct Sim3Out {
    int n_inliers, status, n_bad1, its[2];
    int pad[3];
    double chi2_stage[2];
    double S[8];
};
static_assert(sizeof(Sim3Desc) == 176 && sizeof(Sim3Out) == 112, "scripts/sim3_bench.py derives the copied bytes from these sizes");
struct Sim3Batch {
    const Sim3Desc* desc;
    Sim3Out* out;
    // per-pair arrays, the two sides of a pair interleaved (five base pointers instead of eleven: the kernel is short of scalar
    // registers, and a lane fetches both sides with one wide load)
    const double* p;           // [total pairs][6] P1c, P2c
    const double* uv;          // [total pairs][4] uv1, uv2
    const double* w;           // [total pairs][2] w1, w2
    double* c;                 // [total pairs][2] chi2 of e12 and e21 at the last evaluation
    unsigned char* flag;       // [total pairs] 1 = the pair left the problem (g2o: both edges removed)
};
// vba_sim3_ransac (vba_sim3_ransac.h)
struct RansacDesc {
    int n_pairs, fix_scale, min_inliers, n_hyp, best_inliers;
    int pad;
    long long pair0, hyp0;     // offsets of the candidate's pairs / hypotheses in the concatenated arrays
    double K1[4], K2[4];
};
struct RansacOut {
    int status, hit, its_done, best_hyp, n_inliers, best_inliers;
    int pad[2];
    double S[8];               // (t, q, s) of the hit
    double best_S[8];          // (t, q, s) of best_hyp
};
#define VBA_RANSAC_HYP 32      // doubles per hypothesis record (device only): sR12 (9) t12 (3) sR21 (9) t21 (3) t (3) q (4) s (1)
static_assert(sizeof(RansacDesc) == 104 && sizeof(RansacOut) == 160, "scripts/sim3_ransac_bench.py derives the copied bytes from these sizes");
struct RansacBatch {
    const RansacDesc* desc;
    RansacOut* out;
    const double* p;           // [total pairs][6] P1c, P2c
    const double* gate;        // [total pairs][2] max_err1, max_err2
    const int* sample;         // [total hypotheses][3]
    double* hyp;               // [total hypotheses][VBA_RANSAC_HYP] device only
    int* cnt;                  // [total hypotheses] inlier count of every hypothesis
    unsigned char* flag;       // [total pairs] inlier flags of the hit
};
// vba_triangulate (vba_triangulate.h)
#define VBA_TRI_CONST 41       // doubles of a pair's constants: Rcw1 (9) tcw1 (3) Ow1 (3) K1 (4), the same of keyframe 2, ratio_factor cos_max chi2_th
#define VBA_TRI_LEVELS 64      // most pyramid levels of a keyframe
#define VBA_TRI_NT 256         // matches per workgroup: the unit of the block-to-pair map
struct TriDesc {
    long long match0, lev0;    // offsets of the pair's matches in the concatenated arrays / of its level tables in the level region
    int n_matches, n_levels1, n_levels2;
    int pad;
    double c[VBA_TRI_CONST];
};
struct TriBlock {
    int pair, first;           // the pair of a workgroup and its first match inside the pair
};
static_assert(sizeof(TriDesc) == 360 && sizeof(TriBlock) == 8, "scripts/triangulate_bench.py derives the copied bytes from these sizes");
struct TriBatch {
    const TriDesc* desc;
    const TriBlock* blk;         // [workgroups] the pair of a workgroup and its first match inside the pair
    const double* lev;           // level tables of all pairs: sigma2_1 [n_levels1] scale_1 [n_levels1] sigma2_2 [n_levels2] scale_2 [n_levels2]
    const double* uv;            // [total matches][4] u1 v1 u2 v2
    const unsigned char* oct;    // [total matches][2] octave in keyframe 1 / 2
    double* x3d;                 // [total matches][3]
    unsigned char* reason;       // [total matches]
};
// vba_two_view_init (vba_two_view.h)
struct TvDesc {
    long long key1_0, key2_0, match0, hyp0;   // offsets of the pair's keypoints, matches and hypotheses in the concatenated arrays
    int n_keys1, n_keys2, n_matches, n_hyp;
    int min_triangulated, pad;
    double K[4], sigma, min_parallax;
};
struct TvOut {
    int status, ok, model, reason, best_hyp_h, best_hyp_f, n_inliers_h, n_inliers_f, n_rt, best_rt;
    int rt_good[8];
    double score_h, score_f, rh, H21[9], F21[9], rt_parallax[8], R21[9], t21[3];
};
#define VBA_TV_HYP_H 18        // doubles per H hypothesis record (device only): H21 (9) H12 (9)
#define VBA_TV_HYP_F 9         // doubles per F hypothesis record (device only): F21
#define VBA_TV_RT 8            // most (R, t) hypotheses of a pair: the per-(hypothesis, match) regions hold this many per match
static_assert(sizeof(TvDesc) == 104 && sizeof(TvOut) == 400, "scripts/two_view_bench.py derives the copied bytes from these sizes");
struct TvBatch {
    const TvDesc* desc;
    const double* uv1;           // [total keypoints of frames 1][2]
    const double* uv2;           // [total keypoints of frames 2][2]
    const int* match;            // [total matches][2]
    const int* sets;             // [total hypotheses][8]
    TvOut* out;
    unsigned char* flag_h;       // [total matches] inlier flags of the best H / F hypothesis
    unsigned char* flag_f;
    unsigned char* tri;          // [total keypoints of frames 1]
    double* x3d;                 // [total keypoints of frames 1][3]
    double* score_h;             // [total hypotheses]
    double* score_f;
    double* hyp_h;               // [total hypotheses][VBA_TV_HYP_H] device only
    double* hyp_f;               // [total hypotheses][VBA_TV_HYP_F] device only
    unsigned char* rt_state;     // [VBA_TV_RT * total matches] device only: 0 rejected, 1 counted, 2 counted and flagged
    double* rt_cos;              // [VBA_TV_RT * total matches] device only
    double* rt_x;                // [VBA_TV_RT * total matches][3] device only
};
// vba_search_triangulation (vba_search_tri.h)
#define VBA_ST_NT 256          // lanes of the one workgroup of a pair
#define VBA_ST_HISTO 30        // HISTO_LENGTH (src/ORBmatcher.cpp:42)
#define VBA_ST_CONST 13        // doubles of a pair's constants: F12 (9) ex ey chi2_epi epipole_r2
struct alignas(16) StKey {     // one keypoint of either keyframe, 64 bytes: four 16-byte loads, the descriptor in the first two
    unsigned int d[8];         // the row of mDescriptors
    double u, v;               // mvKeysUn[idx].pt
    float angle;               // mvKeysUn[idx].angle
    unsigned char oct;         // mvKeysUn[idx].octave (keyframe 2; 0 in keyframe 1)
    unsigned char role;        // keyframe 1: the state the host already knows (1 map point, 2 in no shared node), 0 = a query;
                               // keyframe 2: has_mp
    unsigned char pad[10];
};
struct alignas(16) StQuery {   // one keypoint of keyframe 1 that a shared node lists and that has no map point
    int idx1, c_begin, c_end, pad;   // its candidates: feat[feat0 + c_begin .. feat0 + c_end)
};
struct StDesc {
    long long key1_0, key2_0, feat0, lev0;   // offsets of the pair's keypoint records (the queries share key1_0), of its copy of
                                             // node_feat_2 and of its level tables in the concatenated arrays
    int n_keys1, n_keys2, n_q, n_levels2;
    int th_low, check_orientation;
    double c[VBA_ST_CONST];
};
struct StOut {
    int status, n_matches, n_before_filter;
    int hist[VBA_ST_HISTO];
    int ind[3];
};
static_assert(sizeof(StKey) == 64 && sizeof(StQuery) == 16 && sizeof(StDesc) == 160 && sizeof(StOut) == 144,
              "scripts/search_tri_bench.py derives the copied bytes from these sizes");
struct StBatch {
    const StDesc* desc;
    const StKey* key1;           // keypoint records of keyframe 1 of all pairs
    const StKey* key2;           // ... of keyframe 2
    const StQuery* query;        // [total keypoints of keyframe 1] the first n_q of a pair's region (at key1_0) are used
    const int* feat;             // node_feat_2 of all pairs
    const double* lev;           // level tables of all pairs: level_sigma2_2 [n_levels2] scale_2 [n_levels2]
    StOut* out;                  // [pairs]
    int* match12;                // [total keypoints of keyframe 1]
    unsigned char* best_dist;    // ...
    unsigned char* state;        // ...
};
// vba_fuse (vba_fuse.h)
#define VBA_FU_NT 256          // lanes of a workgroup = most points of a tile
#define VBA_FU_CONST 29        // doubles of a problem's constants: Rcw (9) tcw (3) Ow (3) K (4) bounds (4) grid_inv_w grid_inv_h
                               // log_scale_factor th cos_view chi2_reproj
struct alignas(16) FuKey {     // one keypoint, 64 bytes: the descriptor in the first half, pixel and octave in the second.  The record of
                               // all three projection matchers: vba_search_area.h owns the walk over it (sa_walk), vba_host_keygrid.h packs it
    unsigned int d[8];         // the row of mDescriptors
    double u, v;               // mvKeysUn[idx].pt
    unsigned char oct;         // mvKeysUn[idx].octave
    unsigned char pad[15];
};
struct alignas(16) FuPoint {   // one map point, 128 bytes
    unsigned int d[8];         // GetDescriptor()
    double pos[3], normal[3];
    double dist_min, dist_max, pred_max;
    int skip;
    int pad[5];
};
struct FuTile {                // one workgroup: the points first .. first + 255 of problem prob
    int prob, first;
};
struct FuDesc {
    long long key0, pt0, cell0, feat0, lev0;   // offsets of the problem's keypoint records, point records (and outputs), cell_begin copy,
                                               // cell_feat copy and level tables in the concatenated arrays
    int n_keys, n_pt, n_levels, th_low;
    int cols, rows, check_reproj, pad;
    double c[VBA_FU_CONST];
};
static_assert(sizeof(FuKey) == 64 && sizeof(FuPoint) == 128 && sizeof(FuTile) == 8 && sizeof(FuDesc) == 304,
              "scripts/fuse_bench.py derives the copied bytes from these sizes");
struct FuBatch {
    const FuDesc* desc;
    const FuTile* tile;          // [tiles]
    const FuKey* key;            // keypoint records of all problems
    const FuPoint* pt;           // point records of all problems
    const int* cell_begin;       // cell_begin of all problems
    const int* cell_feat;        // cell_feat of all problems
    const double* lev;           // level tables of all problems: scale [n_levels] inv_level_sigma2 [n_levels]
    int* best_idx;               // [total points]
    unsigned short* best_dist;   // ...
    signed char* level;          // ...
    double* uv;                  // [total points][2]
    unsigned char* state;        // [total points]
};
// vba_search_by_sim3 (vba_search_sim3.h); the target side of a direction reuses FuKey
#define VBA_SS_NT 256          // lanes of a workgroup = most queries of a tile
#define VBA_SS_CONST 36        // doubles of a direction's constants: R_src (9) t_src (3) sR (9) t (3) K (4) bounds of the target (4)
                               // grid_inv_w grid_inv_h log_scale_factor of the target, th
struct alignas(16) SsQuery {   // one keypoint of the source side with a usable, unmatched map point, 96 bytes
    unsigned int d[8];         // GetDescriptor()
    double pos[3];
    double dist_min, dist_max, pred_max;
    int idx;                   // the keypoint's index in its keyframe
    int pad[3];
};
struct SsTile {                // one workgroup: the queries first .. first + 255 of direction dir (0: 1 -> 2, 1: 2 -> 1) of pair
    int pair, dir, first, pad;
};
struct SsDir {                 // one direction of one pair, at [2 * pair + dir]
    long long q0, key0, cell0, feat0, lev0;   // offsets of its query records (and outputs) and of the TARGET's keypoint records, cell_begin
                                              // copy, cell_feat copy and scale table in the concatenated arrays
    int n_q, n_keys, n_levels, th_high;       // n_keys, n_levels, cols, rows: the target's
    int cols, rows, pad[2];
    double c[VBA_SS_CONST];
};
static_assert(sizeof(SsQuery) == 96 && sizeof(SsTile) == 16 && sizeof(SsDir) == 360,
              "scripts/search_sim3_bench.py derives the copied bytes from these sizes");
struct SsBatch {
    const SsDir* dir;            // [2 * pairs]
    const SsTile* tile;          // [tiles]
    const FuKey* key;            // keypoint records of all pairs: keyframe 1 of pair 0, keyframe 2 of pair 0, ...
    const SsQuery* query;        // query records of all pairs: direction 0 of pair 0, direction 1 of pair 0, ...
    const int* cell_begin;       // cell_begin of all keyframes
    const int* cell_feat;        // cell_feat of all keyframes
    const double* lev;           // scale tables of all keyframes
    int* match;                  // [total queries]
    unsigned short* best_dist;   // ...
    signed char* level;          // ...
    unsigned char* state;        // ...
};
// vba_search_by_projection (vba_search_proj.h); the frame's keypoints reuse FuKey
#define VBA_SP_NT 256          // lanes of the one workgroup of a problem (k_search_proj and k_search_proj_kf)
#define VBA_SP_MAX_KEYS 16384  // the claim table of a problem is n_keys int32 in LDS
#define VBA_SP_CONST 28        // doubles of a problem's constants: Rcw (9) tcw (3) Ow (3) K (4) bounds (4) grid_inv_w grid_inv_h
                               // log_scale_factor th cos_view
struct alignas(16) SpQuery {   // one query (a keypoint of the last frame or a local map point), 112 bytes
    unsigned int d[8];         // GetDescriptor()
    double pos[3], normal[3];
    double dist_min, dist_max, pred_max;
    unsigned char skip, blocks, oct;   // oct: LastFrame.mvKeys[i].octave (last-frame mode)
    unsigned char pad[5];
};
struct SpDesc {
    long long key0, q0, cell0, feat0, lev0;   // offsets of the problem's keypoint records (and occupied flags), query records (and
                                              // outputs), cell_begin copy, cell_feat copy and scale table in the concatenated arrays
    int n_keys, n_q, n_levels, th_high;
    int cols, rows, mode, pad0;
    float nn_ratio;
    int pad1;
    double c[VBA_SP_CONST];
};
static_assert(sizeof(SpQuery) == 112 && sizeof(SpDesc) == 304, "scripts/search_proj_bench.py derives the copied bytes from these sizes");
struct SpBatch {
    const SpDesc* desc;
    const FuKey* key;            // keypoint records of all problems
    const unsigned char* occupied;   // [total keypoints]
    const SpQuery* query;        // query records of all problems
    const int* cell_begin;       // cell_begin of all problems
    const int* cell_feat;        // cell_feat of all problems
    const double* lev;           // scale tables of all problems
    int* rounds;                 // [problems]
    int* best_idx;               // [total queries]
    unsigned short* best_dist;   // ...
    unsigned short* best_dist2;  // ... (k_search_proj only)
    signed char* level;          // ...
    double* view_cos;            // ... (k_search_proj only)
    double* uv;                  // [total queries][2]
    unsigned char* state;        // [total queries]
    double* rad;                 // [total queries] device only: the radius of the area
    int* prev;                   // [total queries] device only: -2 the query never reaches the area, else the keypoint it claimed in
                                 // the round before (-1: none)
};
// vba_search_by_projection_kf (vba_search_proj_kf.h) shares all of it: keypoints are FuKey, queries SpQuery (blocks = 1, oct unused),
// the descriptor SpDesc (mode: 0 loop, 1 reloc; th_high holds th_dist; nn_ratio = 0), the argument SpBatch with best_dist2 and
// view_cos null (k_search_proj_kf never touches them, and its arena has no region for them).  The former name of its argument stays
// as an alias: the sanitizer harness tests/host_search_proj_kf_check.cpp spells it
using SkBatch = SpBatch;
// vba_search_by_bow (vba_search_bow.h)
#define VBA_SB_NT 256          // lanes of the one workgroup of a pair
#define VBA_SB_MAX_KEYS 16384  // the claim table of a pair is n_keys2 int32 in LDS
struct alignas(16) SbKey {     // one keypoint of either side, 32 bytes
    unsigned int d[8];         // the row of mDescriptors
};
struct SbQuery {               // one keypoint of side 1 with a good map point in a shared node, in the order of the reference's walk
    int idx1;                  // the keypoint
    int c_begin, c_end;        // its candidates: feat[c_begin .. c_end) of the pair's copy of node_feat2
    int rank;                  // its place among the queries of its node: final after round `rank` of the conflict pass
};
struct SbDesc {
    long long key1_0, key2_0, feat0;   // offsets of the pair's keypoint records of side 1 (and query slots, roles and outputs), of side 2
                                       // (and blocked flags) and of its node_feat2 copy in the concatenated arrays
    int n_keys1, n_keys2, n_q, max_rank;   // max_rank: the largest number of queries in one shared node
    int th_pass;                       // bestDist1 <= th_pass passes the threshold: th_low in KF_FRAME mode, th_low - 1 in KF_KF mode
    float nn_ratio;
};
static_assert(sizeof(SbKey) == 32 && sizeof(SbQuery) == 16 && sizeof(SbDesc) == 48, "scripts/search_bow_bench.py derives the copied bytes from these sizes");
struct SbBatch {
    const SbDesc* desc;
    const SbKey* key1;           // keypoint records of side 1 of all pairs
    const SbKey* key2;           // ... of side 2
    const unsigned char* role;   // [total keypoints of side 1] 0 a query, else the state the host found (1, 2)
    const unsigned char* blocked;   // [total keypoints of side 2] 1: statically no candidate (KF_KF mode without a good map point)
    const SbQuery* query;        // [total keypoints of side 1] the first n_q of a pair's region (at key1_0) are used
    const int* feat;             // node_feat2 of all pairs
    int* rounds;                 // [pairs]
    int* best_idx;               // [total keypoints of side 1]
    unsigned short* best_dist;   // ...
    unsigned short* best_dist2;  // ...
    unsigned char* state;        // ...
    int* prev;                   // [total keypoints of side 1] device only, per query slot: the keypoint the query claimed in the round
                                 // before (-1: none)
};
// vba_search_for_initialization (vba_search_init.h); the keypoints of frame 2 reuse FuKey
#define VBA_SI_NT 256          // lanes of the one workgroup of a pair
#define VBA_SI_MAX_KEYS 16384  // the list heads of a pair are n_keys2 int32 in LDS
#define VBA_SI_CONST 8         // doubles of a pair's constants: the target block of sa_walk (bounds (4) grid_inv_w grid_inv_h, then the
                               // window at SA_LOGSF and 0 at SA_TH)
struct alignas(16) SiQuery {   // one level-0 keypoint of frame 1, in index order, 64 bytes
    unsigned int d[8];         // the row of F1.mDescriptors
    double u, v;               // vbPrevMatched[idx1], widened
    int idx1;                  // the keypoint
    int pad[3];
};
struct SiDesc {
    long long key0, q0, cell0, feat0;   // offsets of the pair's keypoint records of frame 2, query records (and outputs), cell_begin copy and
                                        // cell_feat copy in the concatenated arrays
    int n_keys, n_q, cols, rows;        // n_keys: of frame 2
    int th_low;
    float nn_ratio;
    int pad[2];
    double c[VBA_SI_CONST];
};
static_assert(sizeof(SiQuery) == 64 && sizeof(SiDesc) == 128, "scripts/search_init_bench.py derives the copied bytes from these sizes");
struct SiBatch {
    const SiDesc* desc;
    const FuKey* key;            // keypoint records of frame 2 of all pairs
    const SiQuery* query;        // query records of all pairs
    const int* cell_begin;       // cell_begin of all pairs
    const int* cell_feat;        // cell_feat of all pairs
    int* rounds;                 // [pairs]
    int* best_idx;               // [total queries]
    unsigned short* best_dist;   // ...
    unsigned short* best_dist2;  // ...
    unsigned char* state;        // ... 0 accepted, 2 area empty, 3 threshold, 4 ratio (the states 1, 5 and 6 are the host's)
    int* next;                   // [total queries] device only: the next claimer of the same keypoint, -1 at the end of a list
    int* cdist;                  // [total queries] device only: the distance of the query's claim as the last rebuild saw it
};
// vba_mappoint_update (vba_mappoint.h)
#define VBA_MP_NT 256          // lanes of a workgroup: four wave items or one workgroup item
#define VBA_MP_MAX_OBS 1024    // observations of a point: 1024 descriptors of 32 bytes are the 32 KB of LDS of a workgroup
#define VBA_MP_WAVE_OBS 256    // a point of at most so many observations is one wave's item (8 KB of LDS)
#define VBA_MP_ROWS 4          // rows a lane owns at most: VBA_MP_WAVE_OBS / 64 = VBA_MP_MAX_OBS / VBA_MP_NT
struct alignas(16) MpItem {    // one point with device work, 80 bytes
    long long desc0, obs0;     // its rows in the descriptor region; its entries in the observer region
    int n_desc;                // N: descriptors of good keyframes, 0 without a descriptor part
    int n_obs;                 // observations, bad keyframes counted, 0 without a normal part
    int ref;                   // the reference keyframe's row in the centre region
    int pad;
    double pos[3];             // mWorldPos
    double ref_scale, ref_top_scale;
    double pad2;
};
static_assert(sizeof(MpItem) == 80, "scripts/mappoint_bench.py derives the copied bytes from this size");
struct MpBatch {
    const MpItem* item;          // [items] workgroup items first, then the wave items, four to a workgroup
    const double* center;        // [total keyframes][3]
    const int* obs;              // observers of the points with a normal part, as rows of center
    const unsigned int* desc;    // [total N][8] the descriptors of good keyframes of the points with a descriptor part
    int n_items, n_big;          // n_big: the workgroup items
    int* best;                   // [items] (median << 16) | row, -1 without a descriptor part
    double* nrm;                 // [items][5] normal, dist_max, dist_min
    unsigned char* nstate;       // [items] 0 done, 3 the point lies in an observer's centre, 1 no normal part
};
// vba_posegraph_optimize (vba_posegraph.h)
struct PgDesc {
    int nv, ne, nf, npair;
    int fix_scale, its, n_pt, debug;   // debug: stop after the solve of the first trial of the first iteration (hooks flavour)
    double lambda_init;
    long long v0, e0, f0, r0, env0, inc0, pair0, pb0, pe0, pt0;   // offsets of the graph in the concatenated arrays (r0, pb0: the
                                                                  // arrays with one entry more than rows / pairs)
};
struct PgOut {
    int status, its_done, lm_trials, stop;
    double chi2_initial, chi2_final, lambda_final;
};
struct PgBatch {
    const PgDesc* desc;
    PgOut* out;
    const double* Sin;       // [vertices][8] t(3) q(4, xyzw) s: the initial estimates
    const double* meas;      // [edges][8] Sji
    const int *ei, *ej;      // [edges] vertex 0 / vertex 1
    const int* free_of;      // [vertices] free index or -1
    const int *vert_of, *first, *last_row;   // [free]
    const int *row_off, *inc_begin;          // [free + graphs]
    const int* inc;
    const int *pair_lo, *pair_hi;            // [pairs]
    const int* pair_begin;                   // [pairs + graphs]
    const int* pair_edge;
    const double* pt_in;     // [points][3]
    const int* pt_ref;       // [points] index into the concatenated vertices
    double* S;               // [vertices][8] the estimates (copied back)
    double* Sbk;             // [vertices][8] push() / pop()
    double* err;             // [edges][7]
    double* J;               // [edges][2][49] J_i, J_j row-major (error component, direction)
    double *H, *F;           // [envelope blocks][49]
    double* Ld;              // [free][49] factor of the diagonal blocks: unit lower L with D on the diagonal
    double *b, *w, *y, *x;   // [free][7]
    double* pt_out;          // [points][3]
    long long n_pt_total;
};
