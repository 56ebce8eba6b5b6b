// vba_host_small.h -- host side of the library, part 5: the drivers of the small-problem entry points (vba_preintegrate,
// vba_pose_optimize, vba_sim3_optimize, vba_sim3_ransac, vba_triangulate, vba_two_view_init, vba_search_triangulation, vba_fuse, vba_posegraph_optimize).  Each lays its arena out once (vba_host_arena.h), packs the
// pinned staging block with the plain-C++ half of its topic (vba_host_pose.h, vba_host_sim3.h, vba_host_sim3_ransac.h,
// vba_host_triangulate.h, vba_host_two_view.h, vba_host_search_tri.h, vba_host_fuse.h, vba_host_posegraph.h), and does one
// H2D copy, one or two launches and one D2H copy on the handle's stream.  No entry point shares its arena with another.
#pragma once
#include "vba_host_pose.h"
#include "vba_host_sim3.h"
#include "vba_host_sim3_ransac.h"
#include "vba_host_triangulate.h"
#include "vba_host_two_view.h"
#include "vba_host_search_tri.h"
#include "vba_host_fuse.h"
#include "vba_host_posegraph.h"

namespace {
using vba_host::at;

// threads that pack the items of a vba_pose_optimize / vba_sim3_optimize / vba_sim3_ransac / vba_triangulate call
int small_pack_threads(int n_items) { return (n_items >= 256) ? std::max(1, std::min(8, host_threads())) : 1; }

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
    HIPCHK(h, h->preint.dev.ensure(L.total_bytes()));
    void* base = h->preint.dev.p;
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

int pose_optimize(Handle* h, int32_t n_frames, vba_frame_problem* const* inout, vba_frame_result* const* out) {
    if (n_frames <= 0 || !inout || !out) return fail(h, "vba_pose_optimize: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    size_t n_tot = 0;
    if (const char* m = vba_host::check_pose(n_frames, inout, out, n_tot)) return fail(h, std::string("vba_pose_optimize: ") + m);
    const vba_host::PoseArena A(n_frames, n_tot);
    HIPCHK(h, h->pose.ensure(A.L));
    void *hin = h->pose.in.p, *hout = h->pose.out.p, *base = h->pose.dev.p;
    FrameDesc* desc = at<FrameDesc>(hin, A.desc);
    vba_host::describe_pose(n_frames, inout, desc);   // offsets first, then the frames are packed by a few host threads
    std::atomic<int> bad_cov(0);
    host_parallel_for(h, n_frames, small_pack_threads(n_frames), [&](int f) {
        if (!vba_host::pack_frame(inout[f], desc[f], at<double>(hin, A.pw), at<double>(hin, A.uv), at<double>(hin, A.w))) bad_cov.store(1);
    });
    if (bad_cov.load()) return fail(h, "vba_pose_optimize: imu_cov_pvphi is singular or not finite");
    PoseBatch B;
    B.desc = at<FrameDesc>(base, A.desc); B.pw = at<double>(base, A.pw); B.uv = at<double>(base, A.uv); B.w = at<double>(base, A.w);
    B.out = at<FrameOut>(base, A.out); B.lvl = at<unsigned char>(base, A.lvl); B.err = at<double>(base, A.err);
    B.n_frames = n_frames;
    HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_pose_opt, dim3(n_frames), dim3(64), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hout, B.out, A.L.back_bytes(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const FrameOut* res = at<FrameOut>(hout, A.L.in_back(A.out));
    const unsigned char* lvl = at<unsigned char>(hout, A.L.in_back(A.lvl));
    for (int f = 0; f < n_frames; f++) vba_host::unpack_frame(inout[f], out[f], desc[f], res[f], lvl);
    return 0;
}

// Optimizer::OptimizeSim3 (src/Optimizer.cpp:4579-4785) between edge set-up and write-back, for a batch of independent loop
// candidates: k_sim3_opt runs one workgroup per candidate
int sim3_optimize(Handle* h, int32_t n_problems, vba_sim3_problem* const* inout, vba_sim3_result* const* out) {
    if (n_problems < 0 || (n_problems > 0 && (!inout || !out))) return fail(h, "vba_sim3_optimize: bad arguments");
    if (n_problems == 0) return 0;
    size_t n_tot = 0;
    bool want_chi2 = false;
    std::string err;
    if (vba_host::check_sim3(n_problems, inout, out, n_tot, want_chi2, err)) return fail(h, "vba_sim3_optimize: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::Sim3Arena A(n_problems, n_tot);
    const size_t b_back = A.download_bytes(want_chi2);
    HIPCHK(h, h->sim3.ensure(A.L, b_back));
    void *hin = h->sim3.in.p, *hout = h->sim3.out.p, *base = h->sim3.dev.p;
    Sim3Desc* desc = at<Sim3Desc>(hin, A.desc);
    vba_host::describe_sim3(n_problems, inout, desc);
    host_parallel_for(h, n_problems, small_pack_threads(n_problems), [&](int f) {
        vba_host::pack_sim3(inout[f], desc[f], at<double>(hin, A.p), at<double>(hin, A.uv), at<double>(hin, A.w));
    });
    Sim3Batch B;
    B.desc = at<Sim3Desc>(base, A.desc); B.p = at<double>(base, A.p); B.uv = at<double>(base, A.uv); B.w = at<double>(base, A.w);
    B.out = at<Sim3Out>(base, A.out); B.flag = at<unsigned char>(base, A.flag); B.c = at<double>(base, A.c);
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_sim3_opt, dim3(n_problems), dim3(64), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hout, B.out, b_back, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    const Sim3Out* res = at<Sim3Out>(hout, A.L.in_back(A.out));
    const unsigned char* flag = at<unsigned char>(hout, A.L.in_back(A.flag));
    const double* cc = at<double>(hout, A.L.in_back(A.c));
    for (int f = 0; f < n_problems; f++) vba_host::unpack_sim3(inout[f], out[f], desc[f], res[f], flag, cc);
    return 0;
}

// Sim3Solver::iterate (src/Sim3Solver.cpp:138-220) for the triples the caller drew, for a batch of independent loop candidates:
// k_sim3_ransac runs one workgroup per candidate
int sim3_ransac(Handle* h, int32_t n_problems, vba_sim3_ransac_problem* const* inout, vba_sim3_ransac_result* const* out) {
    if (n_problems < 0 || (n_problems > 0 && (!inout || !out))) return fail(h, "vba_sim3_ransac: bad arguments");
    if (n_problems == 0) return 0;
    size_t n_tot = 0, h_tot = 0;
    bool want_counts = false;
    std::string err;
    if (vba_host::check_sim3_ransac(n_problems, inout, out, n_tot, h_tot, want_counts, err)) return fail(h, "vba_sim3_ransac: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::RansacArena A(n_problems, n_tot, h_tot);
    const size_t b_back = A.download_bytes(want_counts);
    HIPCHK(h, h->ransac.ensure(A.L, b_back));
    void *hin = h->ransac.in.p, *hout = h->ransac.out.p, *base = h->ransac.dev.p;
    RansacDesc* desc = at<RansacDesc>(hin, A.desc);
    vba_host::describe_sim3_ransac(n_problems, inout, desc);
    host_parallel_for(h, n_problems, small_pack_threads(n_problems), [&](int f) {
        vba_host::pack_sim3_ransac(inout[f], desc[f], at<double>(hin, A.p), at<double>(hin, A.gate), at<int32_t>(hin, A.sample));
    });
    RansacBatch B;
    B.desc = at<RansacDesc>(base, A.desc); B.p = at<double>(base, A.p); B.gate = at<double>(base, A.gate); B.sample = at<int>(base, A.sample);
    B.out = at<RansacOut>(base, A.out); B.flag = at<unsigned char>(base, A.flag); B.cnt = at<int>(base, A.cnt); B.hyp = at<double>(base, A.hyp);
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_sim3_ransac, dim3(n_problems), dim3(RS_NT), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hout, B.out, b_back, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    const RansacOut* res = at<RansacOut>(hout, A.L.in_back(A.out));
    const unsigned char* flag = at<unsigned char>(hout, A.L.in_back(A.flag));
    const int32_t* cnt = at<int32_t>(hout, A.L.in_back(A.cnt));
    for (int f = 0; f < n_problems; f++) vba_host::unpack_sim3_ransac(inout[f], out[f], desc[f], res[f], flag, cnt);
    return 0;
}

// The per-match loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1358-1517) for a batch of keyframe pairs:
// k_triangulate runs one lane per match, every workgroup inside one pair.  A call without a single match launches nothing
int triangulate(Handle* h, int32_t n_pairs, vba_triangulate_problem* const* in, vba_triangulate_result* const* out) {
    if (n_pairs < 0 || (n_pairs > 0 && (!in || !out))) return fail(h, "vba_triangulate: bad arguments");
    if (n_pairs == 0) return 0;
    size_t n_tot = 0, l_tot = 0, n_blocks = 0;
    std::string err;
    if (vba_host::check_triangulate(n_pairs, in, out, n_tot, l_tot, n_blocks, err)) return fail(h, "vba_triangulate: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::TriArena A(n_pairs, n_tot, l_tot, n_blocks);
    HIPCHK(h, h->tri.ensure(A.L, A.L.back_bytes()));
    void *hin = h->tri.in.p, *hout = h->tri.out.p, *base = h->tri.dev.p;
    TriDesc* desc = at<TriDesc>(hin, A.desc);
    vba_host::describe_triangulate(n_pairs, in, desc, at<TriBlock>(hin, A.blk));
    host_parallel_for(h, n_pairs, small_pack_threads(n_pairs), [&](int f) {
        vba_host::pack_triangulate(in[f], desc[f], at<double>(hin, A.lev), at<double>(hin, A.uv), at<unsigned char>(hin, A.oct));
    });
    const long long launch0 = h->n_launch;
    if (n_blocks) {
        TriBatch B;
        B.desc = at<TriDesc>(base, A.desc); B.blk = at<TriBlock>(base, A.blk); B.lev = at<double>(base, A.lev); B.uv = at<double>(base, A.uv);
        B.oct = at<unsigned char>(base, A.oct); B.x3d = at<double>(base, A.x3d); B.reason = at<unsigned char>(base, A.reason);
        HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
        VBA_LAUNCH(k_triangulate, dim3((unsigned)n_blocks), dim3(TR_NT), 0, h->stream, B);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hout, B.x3d, A.L.back_bytes(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->prof.kernel_launches = h->n_launch - launch0;
    const double* x3d = at<double>(hout, A.L.in_back(A.x3d));
    const unsigned char* reason = at<unsigned char>(hout, A.L.in_back(A.reason));
    for (int f = 0; f < n_pairs; f++) vba_host::unpack_triangulate(out[f], desc[f], x3d, reason);
    return 0;
}

// Initializer::Initialize (src/Initializer.cpp:36-130) behind the drawing of the 8-sets, for a batch of frame pairs: k_two_view
// runs one workgroup per pair, one launch
int two_view_init(Handle* h, int32_t n_problems, vba_two_view_problem* const* in, vba_two_view_result* const* out) {
    if (n_problems < 0 || (n_problems > 0 && (!in || !out))) return fail(h, "vba_two_view_init: bad arguments");
    if (n_problems == 0) return 0;
    vba_host::TwoViewTotals T;
    std::string err;
    if (vba_host::check_two_view(n_problems, in, out, T, err)) return fail(h, "vba_two_view_init: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::TwoViewArena A(n_problems, T);
    const size_t b_back = A.download_bytes(T.want_scores);
    HIPCHK(h, h->tv.ensure(A.L, b_back));
    void *hin = h->tv.in.p, *hout = h->tv.out.p, *base = h->tv.dev.p;
    TvDesc* desc = at<TvDesc>(hin, A.desc);
    vba_host::describe_two_view(n_problems, in, desc);
    host_parallel_for(h, n_problems, small_pack_threads(n_problems), [&](int f) {
        vba_host::pack_two_view(in[f], desc[f], at<double>(hin, A.uv1), at<double>(hin, A.uv2), at<int32_t>(hin, A.match), at<int32_t>(hin, A.sets));
    });
    TvBatch B;
    B.desc = at<TvDesc>(base, A.desc); B.uv1 = at<double>(base, A.uv1); B.uv2 = at<double>(base, A.uv2); B.match = at<int>(base, A.match);
    B.sets = at<int>(base, A.sets); B.out = at<TvOut>(base, A.out); B.flag_h = at<unsigned char>(base, A.flag_h);
    B.flag_f = at<unsigned char>(base, A.flag_f); B.tri = at<unsigned char>(base, A.tri); B.x3d = at<double>(base, A.x3d);
    B.score_h = at<double>(base, A.score_h); B.score_f = at<double>(base, A.score_f); B.hyp_h = at<double>(base, A.hyp_h);
    B.hyp_f = at<double>(base, A.hyp_f); B.rt_state = at<unsigned char>(base, A.rt_state); B.rt_cos = at<double>(base, A.rt_cos);
    B.rt_x = at<double>(base, A.rt_x);
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_two_view, dim3(n_problems), dim3(TV_NT), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hout, B.out, b_back, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    const TvOut* res = at<TvOut>(hout, A.L.in_back(A.out));
    auto u8 = [&](size_t o) { return at<unsigned char>(hout, A.L.in_back(o)); };
    auto f64 = [&](size_t o) { return at<double>(hout, A.L.in_back(o)); };
    for (int f = 0; f < n_problems; f++)
        vba_host::unpack_two_view(out[f], desc[f], res[f], u8(A.flag_h), u8(A.flag_f), u8(A.tri), f64(A.x3d), f64(A.score_h), f64(A.score_f));
    return 0;
}

// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955, monocular) for a batch of keyframe pairs: the host does the node
// join while it packs, k_search_tri runs one workgroup per pair, one launch
int search_triangulation(Handle* h, int32_t n_pairs, vba_search_tri_problem* const* in, vba_search_tri_result* const* out) {
    if (n_pairs < 0 || (n_pairs > 0 && (!in || !out))) return fail(h, "vba_search_triangulation: bad arguments");
    if (n_pairs == 0) return 0;
    vba_host::SearchTriTotals T;
    std::string err;
    if (vba_host::check_search_tri(n_pairs, in, out, T, err)) return fail(h, "vba_search_triangulation: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::SearchTriArena A(n_pairs, T);
    HIPCHK(h, h->st.ensure(A.L, A.L.back_bytes()));
    void *hin = h->st.in.p, *hout = h->st.out.p, *base = h->st.dev.p;
    StDesc* desc = at<StDesc>(hin, A.desc);
    vba_host::describe_search_tri(n_pairs, in, desc);
    host_parallel_for(h, n_pairs, small_pack_threads(n_pairs), [&](int f) {
        vba_host::pack_search_tri(in[f], desc[f], at<StKey>(hin, A.key1), at<StKey>(hin, A.key2), at<StQuery>(hin, A.query), at<int32_t>(hin, A.feat),
                                  at<double>(hin, A.lev));
    });
    StBatch B;
    B.desc = at<StDesc>(base, A.desc); B.key1 = at<StKey>(base, A.key1); B.key2 = at<StKey>(base, A.key2); B.query = at<StQuery>(base, A.query);
    B.feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev); B.out = at<StOut>(base, A.out); B.match12 = at<int>(base, A.match12);
    B.best_dist = at<unsigned char>(base, A.best_dist); B.state = at<unsigned char>(base, A.state);
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_search_tri, dim3(n_pairs), dim3(ST_NT), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hout, B.out, A.L.back_bytes(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    const StOut* res = at<StOut>(hout, A.L.in_back(A.out));
    for (int f = 0; f < n_pairs; f++)
        vba_host::unpack_search_tri(out[f], desc[f], res[f], at<int32_t>(hout, A.L.in_back(A.match12)), at<unsigned char>(hout, A.L.in_back(A.best_dist)),
                                    at<unsigned char>(hout, A.L.in_back(A.state)));
    return 0;
}

// The search half of both ORBmatcher::Fuse overloads (src/ORBmatcher.cpp:958-1254, monocular) for a batch of (keyframe, point list)
// problems: the host lays out the tile table while it packs, k_fuse runs one workgroup per tile of 256 points, one launch
int fuse(Handle* h, int32_t n_problems, vba_fuse_problem* const* in, vba_fuse_result* const* out) {
    if (n_problems < 0 || (n_problems > 0 && (!in || !out))) return fail(h, "vba_fuse: bad arguments");
    if (n_problems == 0) return 0;
    vba_host::FuseTotals T;
    std::string err;
    if (vba_host::check_fuse(n_problems, in, out, T, err)) return fail(h, "vba_fuse: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    const vba_host::FuseArena A(n_problems, T);
    HIPCHK(h, h->fu.ensure(A.L, A.L.back_bytes()));
    void *hin = h->fu.in.p, *hout = h->fu.out.p, *base = h->fu.dev.p;
    FuDesc* desc = at<FuDesc>(hin, A.desc);
    const size_t n_tiles = vba_host::describe_fuse(n_problems, in, desc, at<FuTile>(hin, A.tile));
    host_parallel_for(h, n_problems, small_pack_threads(n_problems), [&](int f) {
        vba_host::pack_fuse(in[f], desc[f], at<FuKey>(hin, A.key), at<FuPoint>(hin, A.pt), at<int32_t>(hin, A.cell), at<int32_t>(hin, A.feat),
                            at<double>(hin, A.lev));
    });
    FuBatch B;
    B.desc = at<FuDesc>(base, A.desc); B.tile = at<FuTile>(base, A.tile); B.key = at<FuKey>(base, A.key); B.pt = at<FuPoint>(base, A.pt);
    B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev);
    B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist); B.level = at<signed char>(base, A.level);
    B.uv = at<double>(base, A.uv); B.state = at<unsigned char>(base, A.state);
    const long long launch0 = h->n_launch;
    if (n_tiles > 0) {   // a call whose problems all have no points has nothing to search
        HIPCHK(h, hipMemcpyAsync(base, hin, A.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
        VBA_LAUNCH(k_fuse, dim3((unsigned)n_tiles), dim3(FU_NT), 0, h->stream, B);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hout, B.best_idx, A.L.back_bytes(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->prof.kernel_launches = h->n_launch - launch0;
    for (int f = 0; f < n_problems; f++)
        vba_host::unpack_fuse(out[f], desc[f], at<int32_t>(hout, A.L.in_back(A.best_idx)), at<uint16_t>(hout, A.L.in_back(A.best_dist)),
                              at<int8_t>(hout, A.L.in_back(A.level)), at<double>(hout, A.L.in_back(A.uv)), at<unsigned char>(hout, A.L.in_back(A.state)));
    return 0;
}

// what vba_debug_posegraph_system asks of a run: graph 0 stops after the solve of its first trial, and H, b, x come back
struct PgDebug { double *H, *b, *x; };

// Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4243-4552) between edge set-up and write-back, for a batch of independent
// graphs: the host validates every graph and lays out its envelope (vba_host_posegraph.h), k_posegraph_opt runs one workgroup per
// graph, k_posegraph_points moves the map points when there are any
int posegraph_run(Handle* h, int32_t n_graphs, vba_posegraph_problem* const* inout, vba_posegraph_result* const* out, PgDebug* dbg) {
    if (n_graphs < 0 || (n_graphs > 0 && (!inout || !out))) return fail(h, "vba_posegraph_optimize: bad arguments");
    if (n_graphs == 0) return 0;
    vba_host::PoseGraphCall C;
    std::string err;
    if (vba_host::describe_posegraph(n_graphs, inout, out, dbg != nullptr, C, err)) return fail(h, "vba_posegraph_optimize: " + err);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->pg.ensure(C.L));
    char* hin = at<char>(h->pg.in.p, 0);
    void *hout = h->pg.out.p, *base = h->pg.dev.p;
    std::memcpy(hin + C.o_desc, C.desc.data(), sizeof(PgDesc) * (size_t)n_graphs);
    for (int g = 0; g < n_graphs; g++) vba_host::pack_posegraph(C, g, inout[g], hin);
    PgBatch B;
    auto d = [base](size_t o) { return at<double>(base, o); };
    auto i = [base](size_t o) { return at<int>(base, o); };
    B.desc = at<PgDesc>(base, C.o_desc);
    B.out = at<PgOut>(base, C.o_out);
    B.Sin = d(C.o_Sin); B.meas = d(C.o_meas); B.ei = i(C.o_ei); B.ej = i(C.o_ej); B.free_of = i(C.o_free);
    B.vert_of = i(C.o_vert); B.first = i(C.o_first); B.last_row = i(C.o_last); B.row_off = i(C.o_roff); B.inc_begin = i(C.o_incb);
    B.inc = i(C.o_inc); B.pair_lo = i(C.o_plo); B.pair_hi = i(C.o_phi); B.pair_begin = i(C.o_pb); B.pair_edge = i(C.o_pe);
    B.pt_in = d(C.o_pt); B.pt_ref = i(C.o_ref);
    B.S = d(C.o_S); B.Sbk = d(C.o_Sbk); B.err = d(C.o_err); B.J = d(C.o_J); B.H = d(C.o_H); B.F = d(C.o_F); B.Ld = d(C.o_Ld);
    B.b = d(C.o_b); B.w = d(C.o_w); B.y = d(C.o_y); B.x = d(C.o_x); B.pt_out = d(C.o_pto);
    B.n_pt_total = (long long)C.npt;
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, C.L.upload_bytes(), hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_posegraph_opt, dim3(n_graphs), dim3(PG_NT), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    if (C.npt > 0 && !dbg) {
        VBA_LAUNCH(k_posegraph_points, dim3((unsigned)((C.npt + 255) / 256)), dim3(256), 0, h->stream, B);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(hout, B.out, C.L.back_bytes(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    if (dbg) {   // graph 0 as the kernel formed it: the envelope expanded to a dense symmetric matrix, b, x
        const vba_host::PoseGraphLayout& L = C.lay[0];
        const size_t n = 7 * (size_t)L.n_free;
        std::vector<double> env(49 * (size_t)L.env_blocks);
        HIPCHK(h, hipMemcpy(env.data(), B.H, env.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(dbg->b, B.b, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(dbg->x, B.x, n * 8, hipMemcpyDeviceToHost));
        vba_host::expand_envelope(L, env.data(), dbg->H);
        return 0;
    }
    const PgOut* res = at<PgOut>(hout, C.L.in_back(C.o_out));
    const double* Sf = at<double>(hout, C.L.in_back(C.o_S));
    const double* pf = at<double>(hout, C.L.in_back(C.o_pto));
    for (int g = 0; g < n_graphs; g++) vba_host::unpack_posegraph(inout[g], out[g], C.desc[g], res[g], Sf, pf);
    return 0;
}

}  // namespace
