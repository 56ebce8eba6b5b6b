// vba_host_plan.h -- the policy of a batch in one place (plain C++17, no HIP): every environment variable the library reads (one
// table), what the vba_debug_set_* hooks override, and the pure integer functions that decide which kernels a batch takes
// (plan_upload, plan_run), how a run is cut into window groups (group_bounds) and vba_batch_solve into chunks (chunk_bounds).
// Included by vislam_ba.hip (through vba_host_structure.h) and by the sanitizer harness tests/host_plan_check.cpp
// (tests/test_host_plan.py).  The summation order of the results depends on these choices and on nothing else: inside one regime
// -- one row of the thresholds 4 / 8 / 64 / VBA_LL_MIN below -- everything is bit-reproducible ("regime").
#pragma once
#include "../../include/vislam_ba.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>

namespace vba_host {

// ---- the knobs: every environment variable the library reads ---------------------------------------------------------------
// X(field, name, kind, default, read).  KNOB_FLAG: 1 when the variable is set at all (also to "" or "0"); KNOB_INT: atoi of its
// value, the default when unset; KNOB_TEXT: the string itself (nullptr when unset).  READ_ONCE: snapshotted at the first use in the
// process; READ_EACH: read again at every upload and every vba_batch_solve call (the tests flip these inside one process).
// INTEGRATION.md's knob table has one row per entry, in this order (tests/test_host_plan.py compares the names).
enum KnobKind { KNOB_FLAG, KNOB_INT, KNOB_TEXT };
enum KnobRead { READ_ONCE, READ_EACH };
const int KNOB_UNSET = INT_MIN;   // default of an int knob whose "0" differs from "unset"
#define VBA_KNOBS(X) \
    X(streams, "VBA_STREAMS", KNOB_INT, 0, READ_ONCE)                   /* > 0: window groups of a run */ \
    X(lane_streams, "VBA_LANE_STREAMS", KNOB_INT, 2, READ_ONCE)         /* window groups of a lane / arena */ \
    X(right_looking, "VBA_RIGHT_LOOKING", KNOB_FLAG, 0, READ_ONCE)      /* never the left-looking kernels */ \
    X(ll_min, "VBA_LL_MIN", KNOB_INT, 256, READ_ONCE)                   /* windows from which the factorisation is left-looking */ \
    X(no_chain, "VBA_NO_CHAIN", KNOB_FLAG, 0, READ_EACH)                /* one launch per block column everywhere */ \
    X(chain_rl_max, "VBA_CHAIN_RL_MAX", KNOB_INT, 64, READ_ONCE)        /* right-looking: chain columns in one launch up to here */ \
    X(chain_min, "VBA_CHAIN_MIN", KNOB_INT, 4, READ_ONCE)               /* fewest chain columns worth the chain kernels (structure) */ \
    X(one_chain, "VBA_ONE_CHAIN", KNOB_FLAG, 0, READ_EACH)              /* no two-sided order */ \
    X(order, "VBA_ORDER", KNOB_INT, -1, READ_ONCE)                      /* >= 0: forced elimination order (structure) */ \
    X(chol_step, "VBA_CHOL_STEP", KNOB_INT, 0, READ_ONCE)               /* 1: first form of the fused step */ \
    X(trsv_old, "VBA_TRSV_OLD", KNOB_FLAG, 0, READ_ONCE)                /* k_trsv also for the row-major factor */ \
    X(schur_split, "VBA_SCHUR_SPLIT", KNOB_FLAG, 0, READ_ONCE)          /* inverse-depth Schur in two launches */ \
    X(lin_imu_split, "VBA_LIN_IMU_SPLIT", KNOB_FLAG, 0, READ_ONCE)      /* IMU factors in a launch of their own */ \
    X(pcg_jacobi, "VBA_PCG_JACOBI", KNOB_FLAG, 0, READ_ONCE)            /* block-Jacobi PCG preconditioner */ \
    X(pace_depth, "VBA_PACE_DEPTH", KNOB_INT, 0, READ_ONCE)             /* > 0: iterations the host stays ahead */ \
    X(st_row_lds, "VBA_ST_ROW_LDS", KNOB_FLAG, 0, READ_EACH)            /* structure build: pair-row counts in LDS */ \
    X(arena_max, "VBA_ARENA_MAX", KNOB_INT, 8, READ_ONCE)               /* windows up to which an upload is one arena copy */ \
    X(upload_no_overlap, "VBA_UPLOAD_NO_OVERLAP", KNOB_FLAG, 0, READ_ONCE) /* no incremental copies */ \
    X(upload_threads, "VBA_UPLOAD_THREADS", KNOB_INT, KNOB_UNSET, READ_ONCE) /* host threads of a handle */ \
    X(local_world_size, "LOCAL_WORLD_SIZE", KNOB_INT, 1, READ_ONCE)     /* ranks that share this node's cores (torchrun) */ \
    X(rank_cpus, "VBA_RANK_CPUS", KNOB_FLAG, 0, READ_ONCE)              /* the launcher pinned this rank to its share */ \
    X(chunk, "VBA_CHUNK", KNOB_INT, 1536, READ_ONCE)                    /* vba_batch_solve: windows per chunk */ \
    X(lanes, "VBA_LANES", KNOB_INT, 2, READ_ONCE)                       /* vba_batch_solve: chunks in flight */ \
    X(run_slots, "VBA_RUN_SLOTS", KNOB_INT, 1, READ_ONCE)               /* vba_batch_solve: lanes inside the solve at once */ \
    X(no_ramp, "VBA_NO_RAMP", KNOB_FLAG, 0, READ_ONCE)                  /* vba_batch_solve: equal chunks */ \
    X(chunks, "VBA_CHUNKS", KNOB_TEXT, 0, READ_EACH)                    /* vba_batch_solve: explicit chunk sizes "384,1024" */ \
    X(timing, "VBA_TIMING", KNOB_FLAG, 0, READ_ONCE)                    /* timing lines on stderr */

template <KnobKind K> struct KnobValue { typedef int type; };
template <> struct KnobValue<KNOB_TEXT> { typedef const char* type; };
struct Knobs {
#define VBA_KNOB_FIELD(field, name, kind, def, read) KnobValue<kind>::type field = def;
    VBA_KNOBS(VBA_KNOB_FIELD)
#undef VBA_KNOB_FIELD
};
struct KnobEntry { const char* name; KnobKind kind; int def; KnobRead read; };
const KnobEntry knob_table[] = {
#define VBA_KNOB_ENTRY(field, name, kind, def, read) {name, kind, def, read},
    VBA_KNOBS(VBA_KNOB_ENTRY)
#undef VBA_KNOB_ENTRY
};

typedef const char* (*GetEnv)(const char*);
inline const char* process_env(const char* name) { return getenv(name); }
inline void knob_set(int& field, KnobKind kind, int def, const char* v) { field = kind == KNOB_FLAG ? (v ? 1 : 0) : (v ? atoi(v) : def); }
inline void knob_set(const char*& field, KnobKind, int, const char* v) { field = v; }
// the one reader: the knobs of read time `when`, from `get`
inline void read_knobs(Knobs& k, KnobRead when, GetEnv get) {
#define VBA_KNOB_READ(field, name, kind, def, read) if (read == when) knob_set(k.field, kind, def, get(name));
    VBA_KNOBS(VBA_KNOB_READ)
#undef VBA_KNOB_READ
}
// the snapshot of the process (what READ_EACH knobs hold in it is never used), and the knobs of an upload / a vba_batch_solve call
// (`get`: the harness feeds a fake environment; the snapshot is taken from the first caller's)
inline const Knobs& process_knobs(GetEnv get = process_env) {
    static const Knobs k = [get] { Knobs q; read_knobs(q, READ_ONCE, get); return q; }();
    return k;
}
inline Knobs current_knobs(GetEnv get = process_env) {
    Knobs k = process_knobs(get);
    read_knobs(k, READ_EACH, get);
    return k;
}

// ---- what the vba_debug_set_* hooks set, per handle.  Precedence everywhere: hook > environment > default.
// PathOverrides is what a lane of vba_batch_solve and an arena of vba_batch_submit inherit from their parent, copied as a whole;
// the rest of Overrides stays with the handle it was set on (a lane takes VBA_LANE_STREAMS, never its parent's `streams`).
struct PathOverrides {
    int ll_min = 0;        // > 0: windows from which the left-looking kernels are used (vba_debug_set_ll_min)
    int no_chain = 0;      // 1: one launch per block column everywhere (vba_debug_set_chain)
    int stop_after = -1;   // >= 0: every window reads the stop flag as 1 from that terminate() poll on (vba_debug_set_stop_after)
    int lin_fallback = 0;  // 1: XYZ windows without the edge-parallel work split (vba_debug_set_lin_fallback)
    int chol_step = 0;     // > 0: form of the fused factorisation step (vba_debug_set_chol_step)
    int schur_split = -1, trsv_old = -1, pcg_jacobi = -1;   // 0 / 1: vba_debug_set_path; -1: the environment's
    int lin_probe = -1;    // vba_debug_set_path "lin_probe": 0 off, 1 on at any batch size, 2 probe every pass that may be one; -1: plan_lin_probe's default
};
struct Overrides {
    PathOverrides path;
    int streams = 0;           // > 0: window groups of a run (vba_debug_set_streams)
    int chunk = 0, lanes = 0;  // > 0: chunk size / lanes of vba_batch_solve (vba_debug_set_chunking)
};
inline int ab_path(int hook, int env) { return hook >= 0 ? hook : env; }

// ---- kernel paths: what a plan chooses and what the capture hook records at the launch site (vba_debug_window_layout [10..12])
enum { CAP_SCHUR_ALL_W, CAP_SCHUR_ALL, CAP_SCHUR_SPLIT_W, CAP_SCHUR_SPLIT, CAP_SCHUR3_W, CAP_SCHUR3 };
enum { CAP_FACTOR_STEP1 = 1, CAP_FACTOR_STEP4 = 4, CAP_FACTOR_STEP4_ONE = 5, CAP_FACTOR_LL = 6, CAP_FACTOR_PCG = 7,
       CAP_FACTOR_MIXED = 8 };   // (MIXED: recorded only -- the columns of one factorisation took different step kernels)
enum { CAP_TRSV_P, CAP_TRSV };
enum { LIN_IMU_FUSED, LIN_IMU_PAIR, LIN_IMU_RES_HESS };   // k_lin2_imu / k_lin_imu_pair / k_lin_imu_res + k_lin_imu_hess

// Grids whose workgroups schur_map() (vba_schur.h) deals to the 8 XCDs by window: the windows of a group, rounded up to 8.
// Three places must agree on the 8: this function, schur_map's `B.n_win >= 8` test on the GROUP's window count, and plan_run's
// rule that a group never holds fewer than 8 windows unless it is the whole batch.
inline int xcd_windows(int n) { return (n >= 8) ? 8 * ((n + 7) / 8) : n; }

// ---- fixed at upload_begin, for the uploaded batch of n windows -----------------------------------------------------------------
struct UploadPlan {
    int n_win = 0;          // windows of the batch: decides WHICH kernels run, so that cutting it into groups never changes a summation order
    int left_looking = 0;   // left-looking tile kernels: S stays pristine, the factor is tile-packed (Batch::l_packed)
    int chain_on = 0;       // chain columns of the factorisation in one launch (vba_chain.h)
    int two_sided = 0;      // the two-sided V/Bias-first order is a candidate for every window
    int arena_on = 0;       // host-built arrays through ONE pinned arena and one H2D copy
    int inc_copy = 0;       // the bulk arrays cross PCIe behind every packing pass
    int results_block = 0;  // control blocks and result arrays in ONE device block, one D2H copy behind the run
    int dev_stop = 0;       // the windows poll a device word that k_poll_stop launches refresh; otherwise the pinned word itself
    int hist_block = 0;     // block size of k_st_hist
    int row_lds = 0;        // structure build: pair-row counts in LDS also for windows of <= 64 keyframes
    int zero_s = 0;         // S is zeroed whole at upload (otherwise only its pad rows)
    int pcg = 0;            // the batch's solver is VBA_SOLVER_PCG
};
inline UploadPlan plan_upload(int n, bool solver_is_pcg, const Overrides& ov, const Knobs& k) {
    UploadPlan u;
    u.n_win = n;
    // >= VBA_LL_MIN windows: left-looking factorisation kernels, which never modify S (measured: the fused right-looking launch per
    // block column is faster up to ~256 windows -- 64 windows 9.2 ms per step against 12.7 for the split kernels that used to serve
    // 64..255, 128: 15.1 / 17.7, 200: 21.8 / 23.1, left-looking at 200: 21.7)
    u.left_looking = !k.right_looking && n >= (ov.path.ll_min > 0 ? ov.path.ll_min : k.ll_min);
    // Chain columns in one launch: in the left-looking regime (two lean launches for all chain columns of all windows), and for up to
    // VBA_CHAIN_RL_MAX = 64 windows in the right-looking one (one workgroup per tile row walks the chain, the two chains of the
    // two-sided order side by side).  Every row workgroup redoes the chain's diagonal work, which is only free while compute units
    // idle -- measured on MI355X, ms per run with / without: 1 window 2.11 / 2.37, 8: 2.71 / 3.06, 16: 3.16 / 3.72, 32: 4.70 / 5.10,
    // 64: 7.44 / 7.52, 96: 10.6 / 10.0, 128: 13.4 / 12.0.  In between: one launch per block column.
    u.chain_on = !k.no_chain && !ov.path.no_chain && (u.left_looking || n <= k.chain_rl_max);
    // the two-sided V/Bias-first order (vba_host_structure.h, order 2): its two half-length chains leave half the fill in the PR rows
    // (C3: 408 tile products against 581), and the few-window chain kernel walks them side by side
    u.two_sided = !k.one_chain;
    // a single window is ~25 arrays of a few KB to a few 100 KB: 25 copies cost 0.4 ms of queue latency
    u.arena_on = n <= k.arena_max;
    u.inc_copy = !u.arena_on && !k.upload_no_overlap;
    u.results_block = n < 4;   // every synchronous copy of the download is a 20-us round trip on a 3-ms solve
    u.dev_stop = n >= 64;      // few windows read the pinned word themselves: no poll launches
    u.hist_block = n <= 64 ? 1024 : 256;
    u.row_lds = k.st_row_lds;
    u.pcg = solver_is_pcg;
    u.zero_s = u.left_looking || solver_is_pcg;   // (PCG reads whole keyframe-pair blocks, also sub-blocks no Schur kernel writes)
    return u;
}

// ---- evaluated at the start of every run (the hooks may change between upload and run and between runs of one upload) ----------
struct RunPlan {
    int schur = -1;          // CAP_SCHUR_*
    int factor = -1;         // CAP_FACTOR_*: PCG, LL, STEP1, STEP4, or STEP4_ONE (one window: descriptor and step table in the kernel arguments)
    int trsv = -1;           // CAP_TRSV*; -1 under PCG
    int step_form = 4;       // 1: k_chol_step, 4: k_chol_step4 (right-looking direct solver only)
    int imu_lin = 0;         // LIN_IMU_*
    int poll = 0;            // k_poll_stop launches
    int pace_depth = 2;      // Gauss-Newton iterations the host stays ahead of the device
    int pcg_tri = 1;         // Batch::pcg_tri
    int dbg_stop_after = -1; // Batch::dbg_stop_after
    int ngroups = 1;         // window groups, each with its own stream
    int word_report = 0;     // one Gauss-Newton window: k_ctrl_gn reports through the pinned word, no event per iteration
    int lin_probe = 0;       // plan_lin_probe (Batch::lin_probe; not one of the plan_ints)
};
// The chi2-only probe of a linearisation pass that is expected to stop its window (vba_batch.h, LIN_AUTO / LIN_REDO): 0 off,
// 1 on, 2 on for every pass that may be one (the hook only: the tests' way to reach every path).  Gauss-Newton over inverse-depth
// windows only -- the Levenberg-Marquardt schedule and the XYZ kernels have no such pass.  By default from 64 windows on, where
// the IMU factors have launches of their own (plan_run: imu_lin): below that a pass is launch latency, and the redo launches
// behind the control kernel would only add to it.  The hook (0 / 1 / 2) overrides the size rule, never the variant or the algorithm.
inline int plan_lin_probe(int n, int variant, int algo, const PathOverrides& path) {
    if (variant != VBA_VARIANT_PRV_IDP || algo != VBA_ALGO_GN) return 0;
    if (path.lin_probe >= 0) return std::min(path.lin_probe, 2);
    return n >= 64 ? 1 : 0;
}
inline RunPlan plan_run(const UploadPlan& u, int n, int variant, int algo, const Overrides& ov, const Knobs& k, bool profile, bool is_lane,
                        int streams_available) {
    RunPlan r;
    const bool idp = variant == VBA_VARIANT_PRV_IDP, xcd = n >= 8;   // (xcd: the per-quad kernels over XCD-mapped grids, below it per pair)
    if (!idp) r.schur = xcd ? CAP_SCHUR3 : CAP_SCHUR3_W;   // (two launches: fusing them as for the inverse-depth records gained nothing at C2)
    else if (ab_path(ov.path.schur_split, k.schur_split)) r.schur = xcd ? CAP_SCHUR_SPLIT : CAP_SCHUR_SPLIT_W;
    else r.schur = xcd ? CAP_SCHUR_ALL : CAP_SCHUR_ALL_W;
    // form 1 (vba_debug_set_chol_step / VBA_CHOL_STEP=1): the first version of the step -- diagonal tile, then the panel solves,
    // v_readlane broadcasts; kept as the cross-check of the hand-written DPP instruction stream.  Anything else: k_chol_step4.
    r.step_form = (ov.path.chol_step > 0 ? ov.path.chol_step : k.chol_step) == 1 ? 1 : 4;
    if (u.pcg) r.factor = CAP_FACTOR_PCG;
    else if (u.left_looking) r.factor = CAP_FACTOR_LL;
    else r.factor = r.step_form == 1 ? CAP_FACTOR_STEP1 : n == 1 ? CAP_FACTOR_STEP4_ONE : CAP_FACTOR_STEP4;
    // row-major factor: k_trsv_p, a solving wave + seven waves that work one column ahead; the packed factor has k_trsv only
    if (!u.pcg) r.trsv = (u.left_looking || ab_path(ov.path.trsv_old, k.trsv_old)) ? CAP_TRSV : CAP_TRSV_P;
    // few windows: latency matters, the IMU factors in one launch -- inside k_lin2's for inverse-depth windows
    r.imu_lin = n >= 64 ? LIN_IMU_RES_HESS : (idp && !k.lin_imu_split) ? LIN_IMU_FUSED : LIN_IMU_PAIR;
    r.poll = u.dev_stop;
    // how far ahead: two iterations for batches (the device must never wait for the host); ONE for a handful of windows, where an
    // iteration is a chain of ~30 short launches that the host enqueues three times faster than the device runs them, and every
    // launch enqueued for a window that has already converged (1.7 us each, 30 per iteration) is latency
    r.pace_depth = k.pace_depth > 0 ? k.pace_depth : (n < 8 ? 1 : 2);
    r.pcg_tri = ab_path(ov.path.pcg_jacobi, k.pcg_jacobi) ? 0 : 1;
    r.dbg_stop_after = ov.path.stop_after;
    // Window groups, each with its own stream (a profiling run uses one).  Measured on MI355X, C3 windows, windows/s with 1 / 2 / 4 / 8
    // groups: 64 windows 5.1k / 5.6k / 5.8k / 4.1k; 256: 7.5k / 8.0k / 8.5k / 6.1k; 512: 8.9k / 9.2k / 9.9k / 8.6k; 1024: 9.7k /
    // 10.1k / 10.2k / 10.0k; 2048: 10.2k / 10.4k / 10.3k / 10.1k.  LM (C2 windows, 1 / 2 / 4 groups): 256 windows 5.9k / 6.2k / 6.5k,
    // 2048: 6.4k / 6.6k / 6.8k.
    int want = ov.streams > 0 ? ov.streams : k.streams;
    if (want <= 0 && is_lane) want = k.lane_streams;   // several lanes share the chip: fewer window groups each
    // default policy (16..48 windows: 2 groups +5..10 %, 4 groups -40 %; from 64 windows on 4 groups -- 16 distinct ragged windows with
    // 3+1 .. 5+3 iterations: 4096 windows 14.0-14.2 k/s with 2 groups, 14.6-14.8 k with 4; 2048 windows 13.7 k either way)
    if (want <= 0) want = (n >= 64) ? 4 : (n >= 16) ? 2 : 1;
    const int max_streams = std::min(std::min(14, want), streams_available);
    if (!profile && max_streams > 1 && n >= 8)
        r.ngroups = std::max(1, std::min(max_streams, n / 8));   // a group never falls below the 8 windows of the XCD-aware mapping
    r.word_report = algo == VBA_ALGO_GN && n == 1 && !profile;   // see k_ctrl_gn
    r.lin_probe = plan_lin_probe(n, variant, algo, ov.path);
    return r;
}

// the windows [b[g], b[g + 1]) of group g of a run
inline std::vector<int> group_bounds(int n, int ngroups) {
    std::vector<int> b(ngroups + 1);
    for (int g = 0; g <= ngroups; g++) b[g] = (int)((long long)n * g / ngroups);
    return b;
}

// ---- vba_batch_solve: chunk boundaries, lanes -------------------------------------------------------------------------------------
// measured on MI355X, 4096 fresh C3 windows (scripts/e2e_sweep.py, resident 12.1-13.0k windows/s): chunk x lanes 512x4 7.8k
// windows/s, 768x3 8.1k, 1024x2 9.05k, 1024x3 8.97k, 1365x2 9.3-9.4k, 1536x2 9.4k, 1700x2 9.6k, 2048x2 (no ramp) 7.7k -- one lane
// solves while the other packs / transfers / builds its structure / scatters; every chunk pays the fixed cost of its ~1700 launches again
inline int chunk_max_of(const Overrides& ov, const Knobs& k) { return std::max(1, ov.chunk > 0 ? ov.chunk : k.chunk); }
inline int lanes_of(const Overrides& ov, const Knobs& k, int n_chunks) { return std::max(1, std::min(ov.lanes > 0 ? ov.lanes : k.lanes, n_chunks)); }
// A ramp at the start, then equal chunks (no tiny tail).  Uploads go one at a time in chunk order at ~57 us per window, a chunk of
// s windows solves in ~14 + 0.075 s ms: chunk k+1 is on the device before chunk k's solve ends when the uploads of chunks 2..k+1
// fit into the solves of chunks 1..k -- sizes c, 2c, 3.25c, 4.5c with c a quarter of VBA_CHUNK (384, 768, 1248, 1696 for 4096
// windows: measured timeline in DESIGN.md section 6).  No chunk falls below 256 windows when the batch has that many: a chunk of
// at least 256 windows takes the batch's kernels (plan_upload: VBA_LL_MIN is the last threshold).
// explicit_list (VBA_CHUNKS, experiments): chunk sizes "384,1024,1664"; the rest goes into one last chunk.
inline std::vector<int> chunk_bounds(int n, int chunk_max, bool ramp, const char* explicit_list) {
    std::vector<int> cbeg(1, 0);
    int left = n;
    if (explicit_list) {
        for (const char* q = explicit_list; *q && left > 0;) {
            const int c = std::min(left, std::max(1, atoi(q)));
            cbeg.push_back(cbeg.back() + c);
            left -= c;
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        if (left > 0) cbeg.push_back(cbeg.back() + left);
        left = 0;
    }
    const int c = std::max(256, chunk_max / 4);
    const int steps[4] = {c, 2 * c, 13 * c / 4, 9 * c / 2};
    int cap = chunk_max;
    if (ramp && chunk_max >= 1024) {
        cap = steps[3];
        for (int i = 0; i < 4 && left >= steps[i] + 256; i++) {
            cbeg.push_back(cbeg.back() + steps[i]);
            left -= steps[i];
        }
    }
    const int rest = (left > 0) ? std::max(1, (left + cap - 1) / cap) : 0;
    const int base = cbeg.back();
    for (int q = 1; q <= rest; q++) cbeg.push_back(base + (int)((long long)left * q / rest));
    return cbeg;
}

// ---- vba_debug_plan: the stored UploadPlan and the RunPlan of the last run as integers, in this order
//   [0] n_win [1] left_looking [2] chain_on [3] two_sided [4] arena_on [5] inc_copy [6] results_block [7] dev_stop [8] hist_block
//   [9] row_lds [10] zero_s [11] pcg | [12] schur [13] factor [14] trsv [15] step_form [16] imu_lin [17] poll [18] pace_depth
//   [19] pcg_tri [20] dbg_stop_after [21] ngroups [22] word_report
const int PLAN_INTS = 23, PLAN_UPLOAD_INTS = 12;
inline void plan_ints(const UploadPlan& u, const RunPlan& r, long long* out) {
    const int v[PLAN_INTS] = {u.n_win, u.left_looking, u.chain_on, u.two_sided, u.arena_on, u.inc_copy, u.results_block, u.dev_stop, u.hist_block,
                              u.row_lds, u.zero_s, u.pcg, r.schur, r.factor, r.trsv, r.step_form, r.imu_lin, r.poll, r.pace_depth, r.pcg_tri,
                              r.dbg_stop_after, r.ngroups, r.word_report};
    for (int i = 0; i < PLAN_INTS; i++) out[i] = v[i];
}

}  // namespace vba_host
