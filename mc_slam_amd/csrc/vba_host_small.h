// vba_host_small.h -- host side of the library, part 5: the small-problem entry points.  vba_preintegrate copies straight from and
// to the caller's arrays.  The other fourteen are one driver, run_small, over the call object of their topic (PoseCall, Sim3Call, ...:
// plain C++, vba_host_<topic>.h), which knows what is refused, the arena, the packing, the kernel's argument and the write-back;
// what an entry point adds here is the launch of its kernel.  No entry point shares its arena (Handle::side) with another.
#pragma once
#include "vba_host_pose.h"
#include "vba_host_sim3.h"
#include "vba_host_sim3_ransac.h"
#include "vba_host_triangulate.h"
#include "vba_host_two_view.h"
#include "vba_host_search_tri.h"
#include "vba_host_fuse.h"
#include "vba_host_search_sim3.h"
#include "vba_host_search_proj.h"
#include "vba_host_search_proj_kf.h"
#include "vba_host_search_bow.h"
#include "vba_host_search_init.h"
#include "vba_host_mappoint.h"
#include "vba_host_posegraph.h"

namespace {
using vba_host::at;

int preintegrate(Handle* h, int32_t n_edges, const int32_t* sample_begin, const double* gyr, const double* acc, const double* dt,
                 double gyr_meas_cov, double acc_meas_cov, double* imu_meas, double* cov_pvphi, double* imu_info_prv) {
    if (n_edges <= 0 || !sample_begin || !gyr || !acc || !dt || !imu_meas || !cov_pvphi) return fail(h, "vba_preintegrate: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    const int ns = sample_begin[n_edges];
    for (int e = 0; e < n_edges; e++)
        if (sample_begin[e] > sample_begin[e + 1] || sample_begin[e] < 0) return fail(h, "vba_preintegrate: sample_begin is not a CSR");
    // a small private arena, inputs | outputs, copied straight from and to the caller's arrays
    const size_t b_m = (size_t)n_edges * 61 * 8, b_c = (size_t)n_edges * 81 * 8;
    vba_host::ArenaLayout L;
    const size_t o_sb = L.take((size_t)(n_edges + 1) * 4), o_g = L.take((size_t)ns * 24), o_a = L.take((size_t)ns * 24), o_dt = L.take((size_t)ns * 8);
    const size_t o_m = L.take(b_m + 2 * b_c + 1024);   // imu_meas, cov_pvphi, imu_info_prv back to back
    DevBuf& dev = h->side[SIDE_PREINT].dev;
    HIPCHK(h, dev.ensure(L.total_bytes()));
    void* base = dev.p;
    int* d_sb = at<int>(base, o_sb);
    double *d_g = at<double>(base, o_g), *d_a = at<double>(base, o_a), *d_dt = at<double>(base, o_dt), *d_m = at<double>(base, o_m);
    double* d_c = d_m + (size_t)n_edges * 61;
    double* d_i = d_c + (size_t)n_edges * 81;
    HIPCHK(h, hipMemcpyAsync(d_sb, sample_begin, (size_t)(n_edges + 1) * 4, hipMemcpyHostToDevice, h->stream));
    if (ns > 0) {
        HIPCHK(h, hipMemcpyAsync(d_g, gyr, (size_t)ns * 24, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_a, acc, (size_t)ns * 24, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dt, dt, (size_t)ns * 8, hipMemcpyHostToDevice, h->stream));
    }
    VBA_LAUNCH(k_preint, dim3(n_edges), dim3(128), 0, h->stream, n_edges, d_sb, d_g, d_a, d_dt, gyr_meas_cov, acc_meas_cov,
                       d_m, d_c, imu_info_prv ? d_i : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(imu_meas, d_m, b_m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cov_pvphi, d_c, b_c, hipMemcpyDeviceToHost, h->stream));
    if (imu_info_prv) HIPCHK(h, hipMemcpyAsync(imu_info_prv, d_i, b_c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// threads that pack the items of a call
int small_pack_threads(int n_items) { return (n_items >= 256) ? std::max(1, std::min(8, host_threads())) : 1; }

// One call of a small-problem entry point, `name`, over its call object C (a fresh one) and its arena: refuse what cannot run,
// lay the arena out, pack the pinned staging block on a few host threads, then one H2D copy, launch(C.bind(device block), grid),
// one D2H copy of what the callers asked for and a sync on the handle's stream, and the write-back.  A refused call has written
// nothing; a call of no problems returns 0 unless empty_ok is false; a call whose grid is empty copies and launches nothing
template <class Call, class P, class R, class Launch>
int run_small(Handle* h, Side side, const std::string& name, Call& C, int32_t n, P* const* inout, R* const* out, const Launch& launch,
              bool empty_ok = true) {
    if (n < 0 || (n == 0 && !empty_ok) || (n > 0 && (!inout || !out))) return fail(h, name + ": bad arguments");
    if (n == 0) return 0;
    std::string err;
    if (C.prepare(n, inout, out, err)) return fail(h, name + ": " + err);
    HIPCHK(h, hipSetDevice(h->device));
    SideArena& A = h->side[side];
    HIPCHK(h, A.ensure(C.layout(), C.download_bytes()));
    void *hin = A.in.p, *hout = A.out.p, *base = A.dev.p;
    C.describe(inout, hin);   // offsets first, then the problems are packed by a few host threads
    std::atomic<const char*> refused(nullptr);
    host_parallel_for(h, n, small_pack_threads(n), [&](int f) {
        if (const char* why = C.pack(f, inout[f], hin)) refused.store(why);
    });
    if (const char* why = refused.load()) return fail(h, name + ": " + why);
    const long long launch0 = h->n_launch;
    if (C.grid() > 0) {
        HIPCHK(h, hipMemcpyAsync(base, hin, C.layout().upload_bytes(), hipMemcpyHostToDevice, h->stream));
        launch(C.bind(base), (unsigned)C.grid());
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hout, at<char>(base, C.layout().upload_bytes()), C.download_bytes(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->prof.kernel_launches = h->n_launch - launch0;
    for (int f = 0; f < n; f++) C.unpack(f, inout[f], out[f], hin, hout);
    return 0;
}

// Optimizer::PoseOptimization (src/Optimizer.cpp:1671-2317) between vertex set-up and write-back, for a batch of independent
// frames.  Alone among the entry points it refuses a call of no frames
int pose_optimize(Handle* h, int32_t n_frames, vba_frame_problem* const* inout, vba_frame_result* const* out) {
    vba_host::PoseCall C;
    return run_small(h, SIDE_POSE, "vba_pose_optimize", C, n_frames, inout, out,
                     [h](const PoseBatch& B, unsigned g) { VBA_LAUNCH(k_pose_opt, dim3(g), dim3(64), 0, h->stream, B); }, false);
}

// Optimizer::OptimizeSim3 (src/Optimizer.cpp:4579-4785) between edge set-up and write-back, for a batch of independent loop
// candidates
int sim3_optimize(Handle* h, int32_t n_problems, vba_sim3_problem* const* inout, vba_sim3_result* const* out) {
    vba_host::Sim3Call C;
    return run_small(h, SIDE_SIM3, "vba_sim3_optimize", C, n_problems, inout, out,
                     [h](const Sim3Batch& B, unsigned g) { VBA_LAUNCH(k_sim3_opt, dim3(g), dim3(64), 0, h->stream, B); });
}

// Sim3Solver::iterate (src/Sim3Solver.cpp:138-220) for the triples the caller drew, for a batch of independent loop candidates
int sim3_ransac(Handle* h, int32_t n_problems, vba_sim3_ransac_problem* const* inout, vba_sim3_ransac_result* const* out) {
    vba_host::RansacCall C;
    return run_small(h, SIDE_RANSAC, "vba_sim3_ransac", C, n_problems, inout, out,
                     [h](const RansacBatch& B, unsigned g) { VBA_LAUNCH(k_sim3_ransac, dim3(g), dim3(RS_NT), 0, h->stream, B); });
}

// The per-match loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1358-1517) for a batch of keyframe pairs
int triangulate(Handle* h, int32_t n_pairs, vba_triangulate_problem* const* in, vba_triangulate_result* const* out) {
    vba_host::TriCall C;
    return run_small(h, SIDE_TRI, "vba_triangulate", C, n_pairs, in, out,
                     [h](const TriBatch& B, unsigned g) { VBA_LAUNCH(k_triangulate, dim3(g), dim3(TR_NT), 0, h->stream, B); });
}

// Initializer::Initialize (src/Initializer.cpp:36-130) behind the drawing of the 8-sets, for a batch of frame pairs
int two_view_init(Handle* h, int32_t n_problems, vba_two_view_problem* const* in, vba_two_view_result* const* out) {
    vba_host::TwoViewCall C;
    return run_small(h, SIDE_TWO_VIEW, "vba_two_view_init", C, n_problems, in, out,
                     [h](const TvBatch& B, unsigned g) { VBA_LAUNCH(k_two_view, dim3(g), dim3(TV_NT), 0, h->stream, B); });
}

// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955, monocular) for a batch of keyframe pairs: the host does the node
// join while it packs
int search_triangulation(Handle* h, int32_t n_pairs, vba_search_tri_problem* const* in, vba_search_tri_result* const* out) {
    vba_host::SearchTriCall C;
    return run_small(h, SIDE_SEARCH_TRI, "vba_search_triangulation", C, n_pairs, in, out,
                     [h](const StBatch& B, unsigned g) { VBA_LAUNCH(k_search_tri, dim3(g), dim3(ST_NT), 0, h->stream, B); });
}

// The search half of both ORBmatcher::Fuse overloads (src/ORBmatcher.cpp:958-1254, monocular) for a batch of (keyframe, point list)
// problems
int fuse(Handle* h, int32_t n_problems, vba_fuse_problem* const* in, vba_fuse_result* const* out) {
    vba_host::FuseCall C;
    return run_small(h, SIDE_FUSE, "vba_fuse", C, n_problems, in, out,
                     [h](const FuBatch& B, unsigned g) { VBA_LAUNCH(k_fuse, dim3(g), dim3(FU_NT), 0, h->stream, B); });
}

// Both projection searches of ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1258-1496, monocular) for a batch of keyframe pairs; the
// agreement loop runs in the write-back
int search_by_sim3(Handle* h, int32_t n_pairs, vba_search_sim3_problem* const* in, vba_search_sim3_result* const* out) {
    vba_host::SearchSim3Call C;
    return run_small(h, SIDE_SEARCH_SIM3, "vba_search_by_sim3", C, n_pairs, in, out,
                     [h](const SsBatch& B, unsigned g) { VBA_LAUNCH(k_search_sim3, dim3(g), dim3(SS_NT), 0, h->stream, B); });
}

// Both tracking matchers, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, ...) (src/ORBmatcher.cpp:1511-1665) and
// Frame::isInFrustum with SearchByProjection(F, vpMapPoints, th) (:63-156), monocular, for a batch of (frame, ordered query list)
// problems: the claim table of a workgroup is dynamic LDS sized to the call's largest frame; the apply loop is replayed in the
// write-back
int search_by_projection(Handle* h, int32_t n_problems, vba_search_proj_problem* const* in, vba_search_proj_result* const* out) {
    vba_host::SearchProjCall C;
    return run_small(h, SIDE_SEARCH_PROJ, "vba_search_by_projection", C, n_problems, in, out, [h, &C](const SpBatch& B, unsigned g) {
        VBA_LAUNCH(k_search_proj, dim3(g), dim3(SP_NT), C.lds_bytes(), h->stream, B);
    });
}

// The loop-closure and the relocalisation matcher, ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
// (src/ORBmatcher.cpp:354-475) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1667-1797), monocular, for a
// batch of (target, ordered query list) problems, both modes mixed: the conflict pass of k_search_proj (vba_search_claim.h) with
// every query blocking, over k_search_proj's argument; histogram, maxima and drop of the relocalisation mode run in the write-back
int search_by_projection_kf(Handle* h, int32_t n_problems, vba_search_proj_kf_problem* const* in, vba_search_proj_kf_result* const* out) {
    vba_host::SearchProjKfCall C;
    return run_small(h, SIDE_SEARCH_PROJ_KF, "vba_search_by_projection_kf", C, n_problems, in, out, [h, &C](const SpBatch& B, unsigned g) {
        VBA_LAUNCH(k_search_proj_kf, dim3(g), dim3(SK_NT), C.lds_bytes(), h->stream, B);
    });
}

// Both ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cpp:207-350, :609-748) for a batch of pairs: the host does the node join
// while it packs; the claim table of a workgroup is dynamic LDS sized to the call's largest side 2; histogram, maxima and drop run
// in the write-back
int search_by_bow(Handle* h, int32_t n_pairs, vba_search_bow_problem* const* in, vba_search_bow_result* const* out) {
    vba_host::SearchBowCall C;
    return run_small(h, SIDE_SEARCH_BOW, "vba_search_by_bow", C, n_pairs, in, out, [h, &C](const SbBatch& B, unsigned g) {
        VBA_LAUNCH(k_search_bow, dim3(g), dim3(SB_NT), C.lds_bytes(), h->stream, B);
    });
}

// ORBmatcher::SearchForInitialization (src/ORBmatcher.cpp:477-595) for a batch of frame pairs: the host compacts the level-0
// keypoints of frame 1 into the query list while it packs; the claimer lists of a workgroup have their heads in dynamic LDS sized
// to the call's largest frame 2; steals, histogram, maxima, drop and the vbPrevMatched update run in the write-back
int search_for_initialization(Handle* h, int32_t n_pairs, vba_search_init_problem* const* in, vba_search_init_result* const* out) {
    vba_host::SearchInitCall C;
    return run_small(h, SIDE_SEARCH_INIT, "vba_search_for_initialization", C, n_pairs, in, out, [h, &C](const SiBatch& B, unsigned g) {
        VBA_LAUNCH(k_search_init, dim3(g), dim3(SI_NT), C.lds_bytes(), h->stream, B);
    });
}

// MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (src/MapPoint.cpp:336-413, :450-501) for a batch of
// point lists: the host sorts the points of the whole call into the item table while it describes the call, a workgroup takes one
// point of more than 256 observations or four smaller ones; the winner's descriptor is copied in the write-back
int mappoint_update(Handle* h, int32_t n_problems, vba_mappoint_problem* const* in, vba_mappoint_result* const* out) {
    vba_host::MapPointCall C;
    return run_small(h, SIDE_MAPPOINT, "vba_mappoint_update", C, n_problems, in, out,
                     [h](const MpBatch& B, unsigned g) { VBA_LAUNCH(k_mappoint_update, dim3(g), dim3(MP_NT), 0, h->stream, B); });
}

// what vba_debug_posegraph_system asks of a run: graph 0 stops after the solve of its first trial, and H, b, x come back
struct PgDebug { double *H, *b, *x; };

// Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4243-4552) between edge set-up and write-back, for a batch of independent
// graphs: k_posegraph_opt runs one workgroup per graph, k_posegraph_points moves the map points when there are any
int posegraph_run(Handle* h, int32_t n_graphs, vba_posegraph_problem* const* inout, vba_posegraph_result* const* out, PgDebug* dbg) {
    vba_host::PoseGraphCall C;
    C.debug = dbg != nullptr;
    const int rc = run_small(h, SIDE_POSEGRAPH, "vba_posegraph_optimize", C, n_graphs, inout, out, [&](const PgBatch& B, unsigned g) {
        VBA_LAUNCH(k_posegraph_opt, dim3(g), dim3(PG_NT), 0, h->stream, B);
        if (C.npt > 0 && !dbg) VBA_LAUNCH(k_posegraph_points, dim3((unsigned)((C.npt + 255) / 256)), dim3(256), 0, h->stream, B);
    });
    if (rc != 0 || !dbg || n_graphs == 0) return rc;
    // graph 0 as the kernel formed it: the envelope expanded to a dense symmetric matrix, b, x
    const PgBatch B = C.bind(h->side[SIDE_POSEGRAPH].dev.p);
    const vba_host::PoseGraphLayout& G = C.lay[0];
    const size_t nx = 7 * (size_t)G.n_free;
    std::vector<double> env(49 * (size_t)G.env_blocks);
    HIPCHK(h, hipMemcpy(env.data(), B.H, env.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(dbg->b, B.b, nx * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(dbg->x, B.x, nx * 8, hipMemcpyDeviceToHost));
    vba_host::expand_envelope(G, env.data(), dbg->H);
    return 0;
}

}  // namespace
